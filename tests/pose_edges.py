"""Shared by the pose-edge tests (tests/ only): the rotations at which the kernels' rotation frame changes and scenes that start there.

Every kernel that differentiates the residual with respect to the rotation picks one of two frames by rot . rot > DBL_EPSILON
(csrc/sba_rotation.hpp): the general one (a = -d1 R x1, J = J_l(w), an 11-term series below theta^2 = 0.25, closed forms above) and
the small-angle one (R = I + [w]x, a = -d1 x1, J = I).  POSES holds one rotation on either side of every switch, the threshold
itself, and rotations near and beyond pi."""
from functools import lru_cache

import numpy as np

from spherical_bundle_adjuster_amd import synthetic

_U = np.array([1.8, -1.9, 1.7]) / np.linalg.norm([1.8, -1.9, 1.7])
_ROOT_EPS = 2.0 ** -26                                  # _ROOT_EPS ** 2 == DBL_EPSILON exactly

POSES = {
    "zero": np.zeros(3),                                # small frame, B = I
    "below_eps": np.array([3e-9, -2e-9, 1e-9]),         # small frame, B = (I + [w]x)^-1 != I
    "at_eps": np.array([_ROOT_EPS, 0.0, 0.0]),          # theta^2 == DBL_EPSILON: still the small frame
    "next": np.array([np.nextafter(_ROOT_EPS, 1.0), 0.0, 0.0]),     # the first general-frame rotation
    "tiny": np.array([2e-8, -2e-8, 1e-8]),              # general frame where closed forms cancel
    "series": 0.4999 * _U,                              # the last rotation of the series (theta^2 < 0.25)
    "closed": 0.5001 * _U,                              # the first of the closed forms
    "near_pi": 3.1 * _U,
    "past_pi": 4.0 * _U,
}
NAMES = tuple(POSES)
SMALL_FRAME = tuple(k for k, w in POSES.items() if float(w @ w) <= np.finfo(np.float64).eps)
NOISY_ORACLE = ("next", "tiny")                         # the oracle's dual-number Jacobian carries eps / theta of noise there
SEED = 4106

# the mixed batch: one pair per pose in the order of POSES, an empty pair in the middle; first rows both even and odd
BATCH_SIZES = (257, 64, 65, 63, 0, 513, 65, 257, 64, 129)
BATCH_POSES = NAMES[:4] + (None,) + NAMES[4:]
# solves that leave the small frame after their first accepted step: (pose, n, seed)
SOLVE_SCENES = (("zero", 257, SEED), ("below_eps", 300, SEED), ("zero", 300, SEED + 1), ("below_eps", 257, SEED + 1))
SOLVE_CLOSED = (("closed", 200, SEED + 2), ("closed", 129, SEED + 1))


# Smallest sin^2 of the angle between R(rot_init) x1 and x2 that a scene holds.  A match's 2 x 2 depth block has condition 4 / sin^2,
# so float64 forms its share W U^-1 W^T of the reduced system with an error of about (4 / sin^2) eps w d1^2.  Held to a quarter of
# REL_TOL_F64 of max |V| in the smallest scene used (63 matches, d1 <= 20: d1^2 / max |V| <= 0.08) this asks for sin^2 >= 1.4e-4.
# Measured without the rule: error * sin^2 up to 1e-5 of the bound, 4.3 times the bound at sin^2 = 2.2e-6.
MIN_SIN2 = 1e-4


def _draw(rng, m, R, t):
    """m matches in the shape of synthetic.full_rt: sigma = 1e-3, 5 % outliers, depths U(2, 20)."""
    X = rng.standard_normal((m, 3))
    X = X / np.linalg.norm(X, axis=1, keepdims=True) * rng.uniform(2.0, 20.0, size=(m, 1))
    d1 = np.linalg.norm(X, axis=1)
    Y = X @ R.T - t
    d2 = np.linalg.norm(Y, axis=1)
    x2 = Y / d2[:, None] + 1e-3 * rng.standard_normal((m, 3))
    out = rng.random(m) < 0.05
    x2[out] = rng.standard_normal((int(out.sum()), 3))
    return X / d1[:, None], x2 / np.linalg.norm(x2, axis=1, keepdims=True), np.stack([d1, d2], axis=1)


@lru_cache(maxsize=None)
def _scene(name, n, seed, min_sin2):
    rng = np.random.default_rng(seed)
    pose = POSES[name] if name is not None else np.zeros(3)
    axis = rng.standard_normal(3)
    w = pose + axis / np.linalg.norm(axis) * np.deg2rad(3.0)
    R, R0 = synthetic.rodrigues(w), synthetic.rodrigues(pose)
    t = rng.standard_normal(3)
    t /= np.linalg.norm(t)
    t0 = t + 0.1 * rng.standard_normal(3)
    t0 /= np.linalg.norm(t0)
    x1, x2, d12 = _draw(rng, n, R, t)
    while True:                                         # nearly parallel rays at the start are drawn again
        bad = np.flatnonzero(1.0 - np.sum((x1 @ R0.T) * x2, axis=1) ** 2 < min_sin2)
        if len(bad) == 0:
            break
        x1[bad], x2[bad], d12[bad] = _draw(rng, len(bad), R, t)
    c = synthetic.Correspondences(np.ascontiguousarray(x1), np.ascontiguousarray(x2), d12, w, t, pose.copy(), t0)
    for a in (c.x1, c.x2, c.d12, c.rot_true, c.tran_true, c.rot_init, c.tran_init):
        a.setflags(write=False)                         # computed once, shared, left unchanged
    return c


def scene_at(pose, n, seed=SEED, min_sin2=None):
    """A two-view scene in the shape of synthetic.full_rt (sigma = 1e-3, 5 % outliers, depths U(2, 20), exact depths) whose true
    rotation is POSES[pose] + 3 degrees about a random axis and whose start is rot_init = POSES[pose] itself: the rotation under
    test is an ordinary start point, 3 degrees off, and both Huber branches are populated.  pose None: rot_init = 0 (for n = 0).

    A match whose rays are nearly parallel at the start (sin^2 < MIN_SIN2) is drawn again.  Its 2 x 2 depth block has condition
    4 / sin^2, and float64 cannot form its share W U^-1 W^T of the reduced system to REL_TOL_F64 of max |V|: on such a scene the
    float64 restatement of the reference itself misses the bounds these scenes are used with, which do not scale with the
    per-match condition (tests/test_pose_edges_reference_cpu.py shows both: scene_at("near_pi", 64, min_sin2=0) holds a match with
    sin^2 = 2.2e-6, and the float64 dense inverse misses check_against's camera bound 2.2 times over against long double; with the
    rule every float64 restatement meets every bound four times over).  min_sin2: another cut, 0 for none."""
    return _scene(pose, int(n), int(seed), MIN_SIN2 if min_sin2 is None else float(min_sin2))


def planes(c, f32):
    """What the planes hold: f32 planes are the f32-rounded inputs."""
    if not f32:
        return c.x1, c.x2
    return c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)


def batch_scenes():
    return [scene_at(name, n) for name, n in zip(BATCH_POSES, BATCH_SIZES)]


def solve_scenes(with_closed=False):
    return [scene_at(*s) for s in SOLVE_SCENES + (SOLVE_CLOSED if with_closed else ())]


def cat(cs):
    """offsets, x1, x2, d12, rot, tran of a batch of scenes in the layout Batch.upload takes."""
    off = np.concatenate([[0], np.cumsum([len(c.x1) for c in cs])]).astype(np.uint64)
    x1 = np.concatenate([c.x1 for c in cs]).reshape(-1, 3)
    x2 = np.concatenate([c.x2 for c in cs]).reshape(-1, 3)
    d12 = np.concatenate([c.d12 for c in cs]).reshape(-1, 2)
    return off, x1, x2, d12, np.stack([c.rot_init for c in cs]), np.stack([c.tran_init for c in cs])
