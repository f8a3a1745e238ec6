"""Shared by the CPU and GPU tests of the batched 8-point guess (import only): the scenes, the sweep of (trials, fraction,
seed), the harness call that lists every candidate of every trial, and a plain restatement of the consensus pick
(csrc/sba_epipolar.hpp consensus_pick; csrc/sba_epipolar.hip batch_guess_kernel, step 4).

The scenes are chosen for the NUMBER OF VALID CANDIDATES r they give: the kernel's consensus takes other paths at r = 0, 1,
2..5 (lo, hi and the number of candidate groups change), at every multiple of 64 (key slots per lane), at odd r (padding to
an even count) and at r = 256 (the full buffer).  A rotation whose Euler angles all stay below 1.57 for BOTH decompositions
of the essential matrix doubles the count; rotations near 180 degrees leave few or none."""
import ctypes as C
from typing import NamedTuple

import numpy as np

from spherical_bundle_adjuster_amd import synthetic
from test_initial_guess_cpu import _p, harness


class Scene(NamedTuple):
    name: str
    w: tuple          # angle-axis of the true rotation
    n: int            # matches
    noise: float      # sigma of the noise added to x2
    outliers: float   # share of x2 replaced by uniform points
    seed: int


W2 = (1.708, 0.293, -1.334)      # both decompositions valid: r = 2 * trials on clean data


def _axis(deg, axis):
    a = np.asarray(axis, dtype=np.float64)
    return tuple(np.deg2rad(deg) * a / np.linalg.norm(a))


# Clean small rotations (r = trials) from 9 matches -- five occupied groups, every trial grows to 8 matches -- to past the
# 1024-match step of the moments pass; W2 with this translation: both decompositions valid, and with noise a few trials
# lose one (odd counts up to 255); outliers: anything between trials / 2 and trials + 1; rotations of 120 to 179 degrees:
# none or a handful of candidates however many trials run.
SCENES = [
    Scene("clean_9", _axis(20, (1, 2, 3)), 9, 1e-4, 0.0, 1),
    Scene("clean_40", _axis(12, (-1, 0.5, 2)), 40, 2e-4, 0.0, 2),
    Scene("clean_300", _axis(25, (1, 2, 3)), 300, 1e-3, 0.0, 3),
    Scene("clean_1025", _axis(8, (0, 1, -1)), 1025, 3e-3, 0.0, 4),
    Scene("clean_1100", _axis(35, (2, -1, 1)), 1100, 3e-3, 0.0, 5),
    Scene("both_clean", W2, 300, 1e-3, 0.0, 2),
    Scene("both_noise2", W2, 300, 2e-2, 0.0, 2),
    Scene("both_noise3", W2, 300, 3e-2, 0.0, 2),
    Scene("both_1000", W2, 1000, 1e-2, 0.0, 2),
    Scene("out30_100", _axis(20, (1, 2, 3)), 100, 1e-3, 0.3, 1),
    Scene("out50_100", _axis(20, (1, 2, 3)), 100, 1e-3, 0.5, 1),
    Scene("out70_100", _axis(20, (1, 2, 3)), 100, 1e-3, 0.7, 1),
    Scene("out70_100b", _axis(20, (1, 2, 3)), 100, 1e-3, 0.7, 2),
    Scene("out100_100", _axis(20, (1, 2, 3)), 100, 1e-3, 1.0, 0),
    Scene("out100_600", _axis(20, (1, 2, 3)), 600, 1e-3, 1.0, 1),
    Scene("out30_600", _axis(20, (1, 2, 3)), 600, 1e-3, 0.3, 2),
    Scene("out50_600", _axis(20, (1, 2, 3)), 600, 1e-3, 0.5, 1),
    Scene("none_158", _axis(157.6, (-0.13, 0.64, 0.1)), 200, 1e-3, 0.0, 0),
    Scene("none_122", _axis(121.7, (1.37, -0.67, 0.35)), 64, 1e-3, 0.0, 5),
    Scene("few_138", _axis(138.4, (0.45, -0.54, 0.58)), 60, 1e-2, 0.0, 1),
    Scene("few_152", _axis(152.4, (0.29, 0.03, 0.55)), 60, 3e-2, 0.0, 2),
    Scene("few_150", _axis(150.1, (0.1, 0.04, -0.51)), 60, 3e-2, 0.0, 11),
    Scene("few_135", _axis(134.5, (0.19, -1.63, -1.2)), 60, 3e-2, 0.0, 20),
    Scene("few_145", _axis(144.8, (0.47, -1.03, 0.67)), 60, 3e-2, 0.0, 29),
    Scene("few_139", _axis(138.5, (-0.51, -0.35, 0.53)), 200, 3e-2, 0.0, 32),
    Scene("some_170", _axis(170.0, (-0.9, -0.39, 1.63)), 60, 3e-2, 0.0, 38),
]

TRIALS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 80, 96, 97, 98, 127, 128)
SEEDS = (3, 11)
# fraction 0.25 (the reference's) at every trial count; 1.0: every trial draws every group, so all candidates are identical and
# only the index orders the keys; 0.5; 0.02: one group, grown to 8 matches
SWEEP = [(tr, 0.25, sd) for tr in TRIALS for sd in SEEDS] + \
        [(tr, fr, sd) for fr in (1.0, 0.5, 0.02) for tr in (5, 97, 128) for sd in SEEDS]

# the candidate counts the sweep must reach, and the ranges it must reach with both parities
COUNTS_NEEDED = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 256)
COUNT_RANGES = ((5, 64), (64, 128), (128, 192), (192, 256))       # (lo, hi]


def coverage_gaps(counts_nonempty):
    """counts_nonempty: the candidate counts seen on the non-empty scenes.  Returns what is missing (empty: all reached)."""
    seen = set(int(c) for c in counts_nonempty)
    gaps = [c for c in COUNTS_NEEDED if c not in seen]
    for lo, hi in COUNT_RANGES:
        for parity in (0, 1):
            if not any(lo < c <= hi and c % 2 == parity for c in seen):
                gaps.append(("odd" if parity else "even", lo, hi))
    return gaps


def make_scene(s: Scene):
    """x1, x2 (n, 3): the geometry of synthetic.full_rt with a GIVEN rotation."""
    rng = np.random.default_rng([s.seed, 77])
    R = synthetic.rodrigues(np.asarray(s.w, dtype=np.float64))
    t = synthetic._unit(rng.standard_normal(3))
    X = synthetic._sphere(rng, s.n) * rng.uniform(2.0, 20.0, size=(s.n, 1))
    x1 = synthetic._unit(X)
    x2 = synthetic._unit(X @ R.T - t)
    if s.noise > 0:
        x2 = synthetic._unit(x2 + s.noise * rng.standard_normal((s.n, 3)))
    if s.outliers > 0:
        out = rng.random(s.n) < s.outliers
        x2[out] = synthetic._sphere(rng, int(out.sum()))
    return np.ascontiguousarray(x1), np.ascontiguousarray(x2)


def candidates(groups, trials, fraction, seed):
    """Every candidate of every trial from the product's own per-trial code (epi::group_occupancy, epi::group_trial), and
    epi::consensus_pick on the valid ones.  Returns euler (2 trials, 3) f32, tran (2 trials, 3) f32, valid (2 trials,) bool,
    avg (r,) the product's trimmed means, pick (index among the valid ones, -1: none)."""
    h = harness()
    h.harness_guess_candidates.restype = C.c_int
    g = np.ascontiguousarray(groups, dtype=np.float64)
    assert g.shape == (64, 45)
    e = np.zeros((2 * trials, 3), np.float32); t = np.zeros((2 * trials, 3), np.float32)
    v = np.zeros(2 * trials, np.int32); avg = np.zeros(2 * trials); nc = C.c_int(0)
    pick = h.harness_guess_candidates(_p(g), C.c_int(trials), C.c_double(fraction), C.c_ulonglong(seed), _p(e), _p(t), _p(v), _p(avg),
                                      C.byref(nc))
    valid = v.astype(bool)
    assert nc.value == int(valid.sum())
    return e, t, valid, avg[:nc.value].copy(), pick


def consensus_reference(euler):
    """The consensus pick restated (reference .cpp:162-180).  euler: (r, 3) float32, the valid candidates in order.
    Squared distances in float32 exactly as the code forms them, (dx*dx + dy*dy) + dz*dz; square roots in double; a full
    stable sort of every row; the entries [int(0.2 r), int(0.8 r)) added in ascending order; one division (0 / 0 = NaN for
    r = 1).  The pick is the first minimum under `avg < best`: a NaN never replaces and is never replaced.
    Returns (pick, avgs); (-1, empty) for r = 0."""
    e = np.ascontiguousarray(euler, dtype=np.float32).reshape(-1, 3)
    r = len(e)
    if r == 0:
        return -1, np.zeros(0)
    dx = e[:, None, 0] - e[None, :, 0]
    dy = e[:, None, 1] - e[None, :, 1]
    dz = e[:, None, 2] - e[None, :, 2]
    d2 = (dx * dx + dy * dy) + dz * dz
    assert d2.dtype == np.float32
    d = np.sort(np.sqrt(d2.astype(np.float64)), axis=1, kind="stable")
    lo, hi = int(r * 0.2), int(r * 0.8)
    avgs = np.empty(r)
    if hi > lo:
        avgs[:] = np.add.accumulate(d[:, lo:hi], axis=1)[:, -1] / float(hi - lo)      # ascending, one add at a time
    else:
        avgs[:] = float("nan")                                                         # 0 / 0
    best, best_d = 0, avgs[0]
    for i in range(1, r):
        if avgs[i] < best_d:
            best, best_d = i, avgs[i]
    return best, avgs


# Device and host trials run the same source; they differ only in the one libm call of a trial (double atan2, rounded to
# float): at most 1 ulp <= 1.2e-7 per angle (|angle| < pi), hence at most 2 * sqrt(3) * 1.2e-7 ~ 4.2e-7 per distance and per
# trimmed mean, and a gap between two means can close by twice that, 8.4e-7.
DECIDED_GAP = 1e-6


def decided(avgs):
    """True when last-bit differences in the angles cannot change the pick: r <= 2 (r = 1: one candidate; r = 2: both means
    are the same distance), all means equal, or the smallest mean below every other by more than DECIDED_GAP."""
    a = np.asarray(avgs, dtype=np.float64)
    if len(a) <= 2 or (a == a[0]).all():
        return True
    s = np.sort(a)
    return bool(s[1] - s[0] > DECIDED_GAP)


def threshold_clear(euler_all):
    """True when no candidate, valid or rejected, has max |angle| within 1e-5 of the validity threshold 1.57: a last-bit
    difference in an angle then cannot change which candidates are valid."""
    m = np.abs(np.asarray(euler_all, dtype=np.float64)).reshape(-1, 3).max(axis=1)
    return bool((np.abs(m - 1.57) > 1e-5).all())
