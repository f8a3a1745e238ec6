"""Shared by the match-edge tests (tests/ only): the matches that no seeded two-view scene draws, as a named list of cases, the scenes
that hold rows of one kind each, and the exact scene.

synthetic.full_rt and pose_edges.scene_at draw unit bearings, depths in U(2, 20) and 1e-3 of noise, and scene_at draws a match
again whose rays are nearly parallel.  The cases here are what they leave out (R0: the rotation at the evaluation pose):

    parallax   parallel         x2 = normalise(fl(R0 x1))
               antiparallel     x2 = -normalise(fl(R0 x1))
               weak_1e-6, weak_1e-10, weak_1e-14: sin^2 of the angle between R0 x1 and x2
    depth      d1_zero, d2_zero, both_zero (evaluated at 0.9 t: e == t there, and |t|^2 == 1 is delta^2 itself)
               near, far        both depths 1e-6, 1e+6 (times 1 + U(-0.1, 0.1))
               far_parallel     parallel rays, d1 = 1e+6, d2 - d1 in +-U(0.5, 2): the d-only block with underflowed regularisers
               negative         d1 = d2 = -1, outside the d-only bound
    bearing    axis             x1 one of the six axis directions, in turn
               negative_zero    x1 an axis with -0.0 in the other two components
               length_1e-3, length_1e+3: |x1|, with d1 divided by it, so that the geometry stays the ordinary one
    residual   zero, at_delta, at_delta_+1ulp, at_delta_-1ulp: the exact scene only (below)

A parallax row has d1 in U(2, 17) (up to there (c lambda exp(-c d))^2 is above an ulp of 1 and the d-only block stays regular at
any radius; from 18.4 on it is exactly singular at radius 1e16, which is `far_parallel`'s case) and d2 - d1 in U(-0.5, 0.5): e = (d2 - d1) u + t then has a squared norm between 0.25 and 2.25,
both Huber classes.  Every other row is an ordinary match (a point at U(2, 20) seen from both cameras, 1e-3 of noise) in which the
case replaces what it names.  The first row of a `parallel` or `far_parallel` scene has x1 = x2 = an axis direction and d2 - d1 =
0.25, the axis being the one whose R0 x1 points most against t, so that |e|^2 <= 1.0625 - 0.5 / sqrt(3) < 1 and the row is an inlier:
at rot = 0 its depth block is w [[1, -1], [-1, 1]] with w = 1 in any order of operations, Jacobi-scaled to
[[0.25, -0.25], [-0.25, 0.25]], and fma(0.25, 1 / radius, 0.25) == 0.25 from radius 1e16 on -- the exactly singular block is there
whatever the other rows round to.

One scene per kind: scene(kind, pose, n, rep) is pose_edges.scene_at(pose, n, SEED + rep) with the rows rows(n) replaced by rows of
that kind, drawn from a generator seeded by (kind, pose, n, rep); rep < REPEAT.  Most outputs are sums: with one kind per scene a
failing sum names its kind, and a `far` row does not swamp every other kind.  scene("ordinary", ...) is the scene_at scene itself.

The exact scene: rot = 0 (R = I in the small frame), bearings on the axes, depths multiples of 1/8, t = (0.5, 0.25, -0.25) and
delta = 0.75, so that every e and s, and with the loss off every entry of the three modes' packs, is a dyadic rational far below
2^53 / 2^-30: any order of summation gives the same bytes, and the reference is integer arithmetic (exact_terms).  Its `residual`
rows: e == 0; s == delta^2 exactly (e = (0.5, 0.25, 0.5), s = 0.5625); and s one ulp either side of it, by one depth moved one ulp
(exact_scene says why s then rounds to the neighbour of delta^2 in any order of operations, fused or not)."""
from dataclasses import dataclass
from fractions import Fraction
from functools import lru_cache
import zlib

import numpy as np

import pose_edges as pe
from spherical_bundle_adjuster_amd import synthetic

REPEAT = 4                            # scenes of every kind, from different seeds
SIZES = (513, 4099)                   # one block of either small-problem driver; the launch path (> 4096)
POSES = ("closed", "zero")            # the general rotation frame and the small one
N_EDGE = 24                           # edge rows of a scene
SEED = 5200
BATCH_SIZES = (257, 513, 0, 65, 1025)
BATCH_EDGE_PAIRS = (1, 3)
BATCH_POSES = ("closed", "zero", None, "closed", "zero")

PARALLAX = ("parallel", "antiparallel", "weak_1e-6", "weak_1e-10", "weak_1e-14")
DEPTH = ("d1_zero", "d2_zero", "both_zero", "near", "far", "far_parallel", "negative")
BEARING = ("axis", "negative_zero", "length_1e-3", "length_1e+3")
RESIDUAL = ("zero", "at_delta", "at_delta_+1ulp", "at_delta_-1ulp")
WEAK = {"weak_1e-6": 1e-6, "weak_1e-10": 1e-10, "weak_1e-14": 1e-14}
LENGTH = {"length_1e-3": 1e-3, "length_1e+3": 1e+3}


@dataclass(frozen=True)
class Case:
    name: str
    kind: str                          # parallax, depth, bearing, residual
    scenes: str                        # "kind": one scene per kind; "exact": rows of the exact scene


CASES = tuple([Case(k, "parallax", "kind") for k in PARALLAX] + [Case(k, "depth", "kind") for k in DEPTH] +
              [Case(k, "bearing", "kind") for k in BEARING] + [Case(k, "residual", "exact") for k in RESIDUAL])
BY_NAME = {c.name: c for c in CASES}
KINDS = tuple(c.name for c in CASES if c.scenes == "kind")          # what scene() takes, besides "ordinary"
PARALLEL_KINDS = ("parallel", "antiparallel", "far_parallel")      # sin^2 == 0 up to the rounding of R0 x1


def rows(n, count=N_EDGE):
    """Where lanes, waves and blocks meet first (0 and 1 are one lane's pair, 126 and 127 the last pair of wave 0, 128 the first of
    wave 1, 510 .. 513 around the block edge, n - 1 the lane of an odd n whose second slot is padding), the rest spread evenly."""
    first = [i for i in (0, 1, 126, 127, 128, 510, 511, 512, 513) if i < n - 1] + [n - 1]
    first = list(dict.fromkeys(first))[:count]
    rest = [i for i in range(n) if i not in set(first)]
    need = count - len(first)
    spread = [rest[int((k + 0.5) * len(rest) / need)] for k in range(need)] if need > 0 else []
    out = np.array(sorted(first + spread), dtype=np.int64)
    assert len(set(out.tolist())) == min(count, n) and out.max() < n
    return out


@dataclass
class Scene(synthetic.Correspondences):
    kind: str = "ordinary"
    rows: np.ndarray = None            # the replaced rows
    name: str = ""
    pose: str = None
    rep: int = 0


_AXES = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]], dtype=np.float64)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _edge_rows(kind, base, m, rng, axis_row=True):
    """m rows of `kind` for the scene `base`: x1, x2, d12."""
    R, R0, t = synthetic.rodrigues(base.rot_true), synthetic.rodrigues(base.rot_init), base.tran_true
    X = _unit(rng.standard_normal((m, 3))) * rng.uniform(2.0, 20.0, size=(m, 1))
    x1 = X / np.linalg.norm(X, axis=1, keepdims=True)
    if kind == "axis":
        x1 = _AXES[np.arange(m) % 6].copy()
    elif kind == "negative_zero":
        x1 = np.full((m, 3), -0.0)
        x1[np.arange(m), np.arange(m) % 3] = 1.0
    d1 = np.linalg.norm(X, axis=1)
    X = x1 * d1[:, None]
    Y = X @ R.T - t
    d2 = np.linalg.norm(Y, axis=1)
    x2 = _unit(Y / d2[:, None] + 1e-3 * rng.standard_normal((m, 3)))
    if kind in PARALLAX or kind == "far_parallel":
        u = _unit(x1 @ R0.T)
        if kind == "antiparallel":
            x2 = -u
        elif kind in WEAK:
            p = _unit(np.cross(u, rng.standard_normal((m, 3))))
            sn = np.sqrt(WEAK[kind])
            x2 = _unit(np.sqrt(1.0 - WEAK[kind]) * u + sn * p)
        else:
            x2 = u
        d1 = rng.uniform(2.0, 17.0, size=m)                    # exp(-2 d) >= 1.7e-15: the d-only regularisers do not underflow
        d2 = d1 + rng.uniform(-0.5, 0.5, size=m)
        if kind == "far_parallel":
            d1 = np.full(m, 1e6)
            d2 = d1 + rng.uniform(0.5, 2.0, size=m) * rng.choice([-1.0, 1.0], size=m)
        if kind in ("parallel", "far_parallel") and axis_row:   # the row that is singular in any arithmetic at rot = 0
            x1[0] = _AXES[int(np.argmin(_AXES @ R0.T @ base.tran_init))]
            x2[0] = _unit(R0 @ x1[0])
            d2[0] = d1[0] + 0.25
    elif kind == "d1_zero":
        d1 = np.zeros(m)
    elif kind == "d2_zero":
        d2 = np.zeros(m)
    elif kind == "both_zero":
        d1, d2 = np.zeros(m), np.zeros(m)
    elif kind in ("near", "far"):
        f = 1e-6 if kind == "near" else 1e6
        d1, d2 = f * (1.0 + rng.uniform(-0.1, 0.1, size=m)), f * (1.0 + rng.uniform(-0.1, 0.1, size=m))
    elif kind == "negative":
        d1, d2 = np.full(m, -1.0), np.full(m, -1.0)
    elif kind in LENGTH:
        x1, d1 = x1 * LENGTH[kind], d1 / LENGTH[kind]
    elif kind not in ("axis", "negative_zero"):
        raise KeyError(kind)
    return x1, x2, np.stack([d1, d2], axis=1)


def _frozen(s):
    for a in (s.x1, s.x2, s.d12, s.rot_true, s.tran_true, s.rot_init, s.tran_init, s.rows):
        a.setflags(write=False)                                 # computed once, shared, left unchanged
    return s


@lru_cache(maxsize=None)
def scene(kind, pose, n, rep=0, revert=(), axis_row=True):
    """revert: edge rows (indices into the scene) that keep the ordinary match -- the rows a combination drops.  axis_row False:
    the first row of a `parallel` or `far_parallel` scene is a seeded one like the others; which blocks are then exactly singular
    at radius 1e16 depends on how |x1|^2 rounds (about half of them are), and the determinant a * a - a * a of such a block has an
    inexact product: exactly 0 only if both products round alike."""
    base = pe.scene_at(pose, n, SEED + rep)
    where = rows(n)
    x1, x2, d12 = base.x1.copy(), base.x2.copy(), base.d12.copy()
    if kind != "ordinary":
        rng = np.random.default_rng([SEED, zlib.crc32(f"{kind} {pose}".encode()), n, rep])
        e1, e2, ed = _edge_rows(kind, base, len(where), rng, axis_row)
        keep = np.array([i not in revert for i in where])
        x1[where[keep]], x2[where[keep]], d12[where[keep]] = e1[keep], e2[keep], ed[keep]
    # e == t on a `both_zero` row, and |t|^2 == 1 == delta^2 up to rounding: those scenes are evaluated at 0.9 t
    tran = base.tran_init * (0.9 if kind == "both_zero" else 1.0)
    return _frozen(Scene(x1, x2, d12, base.rot_true, base.tran_true, base.rot_init.copy(), tran, kind, where,
                         f"{kind} pose={pose} n={n} rep={rep}", pose, rep))


def scenes(kind, sizes=SIZES):
    return [scene(kind, pose, n, rep) for pose in POSES for n in sizes for rep in range(REPEAT)]


def sin2(c, f32=False):
    """sin^2 of the angle between R0 x1 and x2 per row, float64, from what the planes hold."""
    a1, a2 = pe.planes(c, f32)
    u = a1 @ synthetic.rodrigues(c.rot_init).T
    cr = np.cross(u, a2)
    with np.errstate(all="ignore"):
        return np.sum(cr * cr, axis=1) / (np.sum(u * u, axis=1) * np.sum(a2 * a2, axis=1))


def batch(kind, rep=0):
    """The scenes of the batch BATCH_SIZES: rows of `kind` in pairs 1 and 3, ordinary neighbours ("ordinary": ordinary rows
    everywhere, the same neighbours)."""
    out = []
    for g, (n, pose) in enumerate(zip(BATCH_SIZES, BATCH_POSES)):
        if n == 0:
            out.append(pe.scene_at(None, 0, SEED))
        else:
            out.append(scene(kind if g in BATCH_EDGE_PAIRS else "ordinary", pose, n, rep))
    return out


# ---- the exact scene -------------------------------------------------------------------------------------------------------------
EXACT_DELTA = 0.75
EXACT_TRAN = np.array([0.5, 0.25, -0.25])
EXACT_ROT = np.zeros(3)


@lru_cache(maxsize=None)
def exact_scene(n, ulp_rows=True):
    """-> Scene (kind "exact") and {residual case name: rows}.  Ordinary rows: x1, x2 axes, d1, d2 multiples of 1/8 in [0, 4].
    `zero`: x1 = 4 t, d1 = 0.25, d2 = 0, so e == 0.  The other three: x1 = +x, d1 = 0, x2 = +z, e = (0.5, 0.25, d2 - 0.25):
    s == 0.5625 at d2 = 0.75, and with d2 one ulp (2^-53) up or down e2 = 0.5 +- 2^-53 is representable, e2^2 = 0.25 +- 2^-53 +
    2^-106 and s = 0.5625 +- 2^-53 (+ 2^-106) round to 0.5625 +- 2^-53, fused or not, in any order.  ulp_rows False: those rows
    hold `at_delta` instead, and every sum of the scene is exact."""
    rng = np.random.default_rng([SEED, 99, n])
    x1 = _AXES[rng.integers(6, size=n)].copy()
    x2 = _AXES[rng.integers(6, size=n)].copy()
    d12 = rng.integers(0, 33, size=(n, 2)) / 8.0
    where = rows(n)
    names = {}
    for j, i in enumerate(where):
        name = RESIDUAL[j % 4]
        names.setdefault(name, []).append(int(i))
        if name == "zero":
            x1[i], x2[i], d12[i] = EXACT_TRAN * 4.0, (0.0, 0.0, 1.0), (0.25, 0.0)
        else:
            x1[i], x2[i] = (1.0, 0.0, 0.0), (0.0, 0.0, 1.0)
            moved = 0.75 if name == "at_delta" or not ulp_rows else float(np.nextafter(0.75, np.inf if name.endswith("+1ulp") else -np.inf))
            d12[i] = (0.0, moved)
    s = Scene(x1, x2, d12, EXACT_ROT.copy(), EXACT_TRAN.copy(), EXACT_ROT.copy(), EXACT_TRAN.copy(), "exact", where, f"exact n={n}")
    return _frozen(s), {k: np.array(v) for k, v in names.items()}


def exact_terms(c, delta):
    """Integer arithmetic: per row e (Fractions, (n, 3)), s and the class s > delta^2; the three modes' explicit packs with the
    loss off as Fractions (rot = 0: A = -[a]x with a = -d1 x1, so A = [d1 x1]x)."""
    F = Fraction
    n = len(c.x1)
    e, s, out = [], [], []
    d2_ = F(delta) * F(delta)
    packs = {m: [F(0)] * 24 for m in (0, 1, 2)}
    for i in range(n):
        X = [F(float(c.d12[i, 0])) * F(float(v)) for v in c.x1[i]]
        Y = [F(float(c.d12[i, 1])) * F(float(v)) for v in c.x2[i]]
        ei = [Y[k] - X[k] + F(float(c.tran_init[k])) for k in range(3)]
        si = sum(v * v for v in ei)
        e.append(ei); s.append(si); out.append(delta > 0 and si > d2_)
        # A[r][j] = d e_r / d w_j = -(e_j x X)_r ... e = -(I + [w]x) X + ..., d/dw_j (-[w]x X) = -(e_j x X) = (X x e_j)
        A = [[F(0)] * 3 for _ in range(3)]
        for j in range(3):
            ej = [F(1 if k == j else 0) for k in range(3)]
            cr = [X[1] * ej[2] - X[2] * ej[1], X[2] * ej[0] - X[0] * ej[2], X[0] * ej[1] - X[1] * ej[0]]
            for r in range(3):
                A[r][j] = cr[r]
        p = [F(0)] * 24
        k = 0
        for a in range(3):
            for b in range(a, 3):
                p[k] = sum(A[r][a] * A[r][b] for r in range(3)); k += 1
        for a in range(3):
            for cc in range(3):
                p[6 + 3 * a + cc] = A[cc][a]
            p[16 + a] = sum(A[r][a] * ei[r] for r in range(3))
            p[19 + a] = ei[a]
        p[15], p[22] = F(1), si / 2
        for m, slots in ((0, list(range(6)) + [16, 17, 18, 22]), (1, [15, 19, 20, 21, 22]), (2, list(range(23)))):
            for q in slots:
                packs[m][q] += p[q]
    return e, s, np.array(out), packs


def exact_floats(fr):
    """Fractions -> float64, asserting that every one is representable."""
    out = np.array([float(v) for v in fr])
    assert all(Fraction(float(v)) == v for v in fr), "an entry of the exact scene is not representable"
    return out
