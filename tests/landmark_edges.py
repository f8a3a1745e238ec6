"""Shared by the landmark-edge tests (tests/ only): the priors, bearings and geometries that the seeded scenes of the landmark-map
tests never draw, as a named list of cases, and the scene that holds a row of each.

The scene is an ordinary solve scene (tests/landmark_register_reference.py's recipe) of n landmarks, so the pose is determined by
the ordinary rows, in which the rows rows(n) are replaced.  A replaced row's bearing y is chosen first, the true landmark is placed
on its ray, X = R^T (t + d y) with d in [1, 5] unless the case says otherwise, and the prior mean is drawn from the case's covariance
around that truth with a seeded generator.  With e the unit ray in the world frame and a1, a2 two unit vectors across it:

    zero         Sigma = 0                                        a fixed landmark
    depth_only   sd^2 e e^T                                       rank 1
    across_only  sl^2 (a1 a1^T + a2 a2^T)                         rank 2
    one_across   sl^2 a1 a1^T                                     rank 1 across the ray
    cond_1e8     sd^2 e e^T + sl^2 (a1 a1^T + a2 a2^T), sd^2 / sl^2 = 1e8
    cond_1e12    the same with 1e12
    tiny, vague  the ordinary covariance (resection_weighted_reference.landmark_cov) times 1e-12 and 1e+6

sd = SD |X - centre|, and sl = SL |X - centre| where the case does not fix the ratio.  The bearing cases (an ordinary prior) are the
six axis directions, an axis with -0.0 in the other two components, every sign variant of (1, 1, 0), (0, 1, 1), (1, 0, 1), (1, 1, 1)
unnormalised, so that the ties are exact, (2, 1, 1), (1, 2, 1), (1, 1, 2), whose tie is between the two SMALLEST components, each tie
also with one tied component one ulp up and one ulp down, and the lengths 1e-3 and 1e+3.  The geometry cases: d = 1e-2 and d = 1e+4
(the ordinary covariance grows with |X|^2 by its recipe).  Every prior kind but `zero` and both geometry kinds come REPEAT times,
from different seeds."""
from dataclasses import dataclass
from functools import lru_cache
from itertools import product

import numpy as np

import landmark_register_reference as lr
import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr

SD, SL = 5e-2, 2e-3                  # depth and lateral standard deviations of the built priors, relative to the distance
SIZES = ((513, None), (1537, "1"))   # (n, SBA_RESECT_GRID): the sizes of the planted-row tests
PRIORS = ("zero", "depth_only", "across_only", "one_across", "cond_1e8", "cond_1e12", "tiny", "vague")
CONDITION = {"cond_1e8": 1e8, "cond_1e12": 1e12}
SCALE = {"tiny": 1e-12, "vague": 1e+6}
REPEAT = 8                           # rows of every prior kind but `zero` and of every geometry kind, drawn from different seeds


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                          # the kind the cap of the qualification counts by
    prior: str = "ordinary"
    y: tuple | None = None             # the bearing as given, None: a seeded direction with a length in [0.5, 2]
    length: float | None = None        # of a seeded direction
    d: float | None = None             # the depth along y, None: seeded in [1, 5]
    tie: str | None = None             # the tie this bearing is or neighbours
    moved: int = 0                     # -1, 0, +1 ulp


def _sign_variants(v):
    out = []
    for s in product((1.0, -1.0), repeat=3):
        w = tuple(a * b for a, b in zip(s, v))
        if w not in out:
            out.append(w)
    return out


def _fmt(v):
    return "(" + ",".join(f"{a:+g}" for a in v) + ")"


def _cases():
    cs = [Case(p, p, prior=p) for p in PRIORS]
    more = lambda c: [Case(f"{c.name} #{k}", c.kind, prior=c.prior, d=c.d) for k in range(2, REPEAT + 1)]
    for k, ax in enumerate("xyz"):
        for sg in (1.0, -1.0):
            v = [0.0, 0.0, 0.0]
            v[k] = sg
            cs.append(Case(f"axis {'+' if sg > 0 else '-'}{ax}", "axis", y=tuple(v)))
        v = [-0.0, -0.0, -0.0]
        v[k] = 1.0
        cs.append(Case(f"axis +{ax} negative zeros", "negative_zero", y=tuple(v)))
    ties = []
    for base in ((1.0, 1.0, 0.0), (0.0, 1.0, 1.0), (1.0, 0.0, 1.0), (1.0, 1.0, 1.0)):
        ties += [(v, "tie") for v in _sign_variants(base)]
    ties += [(v, "tie_of_smallest") for v in ((2.0, 1.0, 1.0), (1.0, 2.0, 1.0), (1.0, 1.0, 2.0))]
    for v, kind in ties:
        j = min(i for i in range(3) if abs(v[i]) == 1.0)       # the first tied component is the one moved
        for moved in (0, 1, -1):
            w = list(v)
            if moved:
                w[j] = float(np.nextafter(v[j], np.sign(v[j]) * (np.inf if moved > 0 else 0.0)))
            cs.append(Case(f"{kind} {_fmt(v)}" + ("" if not moved else f" [{j}] {moved:+d} ulp"), kind, y=tuple(w), tie=_fmt(v), moved=moved))
    cs += [Case("length 1e-3", "length", length=1e-3), Case("length 1e+3", "length", length=1e+3)]
    cs += [Case("near", "near", d=1e-2), Case("far", "far", d=1e+4)]
    # the kinds above whose float64 error is one draw of a large rounding error get REPEAT rows, so that the worst of a kind is the
    # worst of several draws; they go last and so take rows of the spread
    for c in [c for c in cs if c.prior not in ("ordinary", "zero") or c.d is not None]:
        cs += more(c)
    return tuple(cs)


CASES = _cases()
KINDS = tuple(dict.fromkeys(c.kind for c in CASES))
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def rows(n):
    """The row of every case: where lanes, waves and blocks meet first (0 and 1 are one lane's pair, 126 and 127 the last pair of
    wave 0, 128 the first of wave 1, 510 .. 513 around the block edge, n - 1 the lane of an odd n whose second slot is padding),
    the rest spread evenly over what remains."""
    first = [0, 1, 126, 127, 128, 510, 511, 512] + ([513] if n > 514 else []) + [n - 1]
    first = list(dict.fromkeys(first))
    rest = [i for i in range(n) if i not in set(first)]
    need = len(CASES) - len(first)
    step = len(rest) / need
    spread = [rest[int((k + 0.5) * step)] for k in range(need)]
    out = first + spread
    assert len(set(out)) == len(CASES) and max(out) < n
    # CASES starts with the priors and the axis bearings: they take the meeting points
    return dict(zip((c.name for c in CASES), out))


def _across(e, rng):
    a1 = np.cross(e, rng.standard_normal(3))
    a1 /= np.linalg.norm(a1)
    a2 = np.cross(e, a1)
    return a1, a2 / np.linalg.norm(a2)


def _rows6(S):
    return np.array([S[0, 0], S[1, 1], S[2, 2], S[0, 1], S[0, 2], S[1, 2]])


@dataclass(frozen=True)
class Scene:
    name: str
    X: np.ndarray          # (n, 3) prior landmarks, as given to set()
    cov: np.ndarray        # (n, 6) as given to set() with cov_scale 1
    y: np.ndarray          # (n, 3) bearings
    truth_X: np.ndarray
    truth_rot: np.ndarray  # the pose the edge rows were placed at
    truth_tran: np.ndarray
    rot: np.ndarray        # the evaluation pose: the truth, or POSES[pose_name] 0.2 degrees off it
    tran: np.ndarray
    rot_ref: np.ndarray    # the freeze pose, lr.FREEZE_OFFSET away from the evaluation pose
    tran_ref: np.ndarray
    rot0: np.ndarray       # the solve's start
    tran0: np.ndarray
    bearing_sigma: float   # of the solve
    rows: dict             # case name -> row
    grid_one: bool = False

    def edge_rows(self):
        return np.array(sorted(self.rows.values()), dtype=np.int64)

    def names(self):
        """Row -> case name."""
        return {i: k for k, i in self.rows.items()}


@lru_cache(maxsize=None)
def scene(n, pose_name=None):
    """pose_name None: the truth is the solve scene's own pose, which is also the evaluation pose.  Otherwise the truth is 0.2
    degrees off pose_edges.POSES[pose_name] and the evaluation pose is POSES[pose_name] itself, as in the register tests' scenes."""
    seed = 27000 + n
    if pose_name is None:
        base = rr.make_scene(n, seed, noise=1e-3)
        rot_eval = base.rot.copy()
    else:
        rot_eval = pose_edges.POSES[pose_name].copy()
        base = rr.make_scene(n, seed, noise=1e-3, rot=rot_eval + np.deg2rad(0.2) * wr.EDGE_AXIS)
    cov, root = wr.landmark_cov(base.X, seed)
    rng = np.random.default_rng(seed + 31337)
    X = base.X + np.einsum("iab,ib->ia", root, rng.standard_normal((n, 3)))
    truth_X, y, cov = base.X.copy(), base.y.copy(), cov.copy()
    R = rr.rotmat(base.rot, np.float64)
    centre = R.T @ base.tran                                   # the frame's centre in the world: c = -R X + t = 0
    where = rows(n)
    for c in CASES:
        i = where[c.name]
        if c.y is not None:
            yi = np.array(c.y)
        else:
            yi = rr._unit(rng.standard_normal(3)) * (rng.uniform(0.5, 2.0) if c.length is None else c.length)
        d = rng.uniform(1.0, 5.0) if c.d is None else c.d
        Xt = R.T @ (base.tran + d * yi)
        dist = np.linalg.norm(Xt - centre)
        e = R.T @ (yi / np.linalg.norm(yi))
        a1, a2 = _across(e, rng)
        sd, sl = SD * dist, SL * dist
        z = rng.standard_normal(3)
        if c.prior in ("ordinary", "tiny", "vague"):
            c6, rt = wr.landmark_cov(Xt[None], seed + 1000 + i)
            f = SCALE.get(c.prior, 1.0)
            Sg, draw = f * wr.full(c6, np.float64)[0], np.sqrt(f) * (rt[0] @ z)
        elif c.prior == "zero":
            Sg, draw = np.zeros((3, 3)), np.zeros(3)
        elif c.prior == "depth_only":
            Sg, draw = sd * sd * np.outer(e, e), sd * z[0] * e
        elif c.prior == "across_only":
            Sg, draw = sl * sl * (np.outer(a1, a1) + np.outer(a2, a2)), sl * (z[1] * a1 + z[2] * a2)
        elif c.prior == "one_across":
            Sg, draw = sl * sl * np.outer(a1, a1), sl * z[1] * a1
        else:
            sl = sd / np.sqrt(CONDITION[c.prior])
            Sg, draw = sd * sd * np.outer(e, e) + sl * sl * (np.outer(a1, a1) + np.outer(a2, a2)), sd * z[0] * e + sl * (z[1] * a1 + z[2] * a2)
        truth_X[i], y[i], cov[i], X[i] = Xt, yi, _rows6(0.5 * (Sg + Sg.T)), Xt + draw
    truth = rr.Scene(truth_X, y, base.rot, base.tran, base.depth)
    rot0, tran0 = rr.start_near(truth, seed, lr.START_ROT, lr.START_TRAN)
    dr, dt = rr._unit(rng.standard_normal(3)), rr._unit(rng.standard_normal(3))
    for a in (X, y, cov, truth_X):
        a.setflags(write=False)
    return Scene(f"edges n={n} {pose_name}", X, cov, y, truth_X, base.rot.copy(), base.tran.copy(), rot_eval, base.tran.copy(),
                 rot_eval + lr.FREEZE_OFFSET * dr, base.tran + lr.FREEZE_OFFSET * dt, rot0, tran0, 1e-3, where, n == 1537)


def subset(s):
    """The indexed form: the edge rows and every fourth other row, strictly increasing."""
    n = len(s.X)
    return np.array(sorted(set(s.rows.values()) | set(range(0, n, 4))), dtype=np.int64)


def forms(s):
    return (("dense", None), ("indexed", subset(s)))


def product_branch(y):
    """The k of csrc/sba_resection_weighted.hpp's resect_weight_basis for one bearing: the first smallest |y_k|."""
    a = np.abs(np.asarray(y, dtype=np.float64))
    return 0 if a[0] <= a[1] and a[0] <= a[2] else (1 if a[1] <= a[2] else 2)
