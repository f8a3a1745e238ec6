"""Shared by the landmark-edge tests (tests/ only): the qualification of tests/landmark_edges.py's rows and the per-row bounds.

The reference of every pass is the long-double form with M = Q (Q^T S Q)^-1 Q^T (landmark_register_reference.PROJECTED,
landmark_fusion_reference.fuse(projected=True)): it holds for a singular S.  float64 numpy in the product's formulation is compared
with it per row; its worst error on the rows of a kind is what float64 can do there, and 8 times that is what the host code and
the device are held to on those rows -- but never less than 8 times its worst error on the ORDINARY rows: numpy's own arithmetic
on an axis bearing is exact in places where another order of operations or a fused multiply-add is not, and a kind is not held
tighter than the rows around it.  That is never looser than the rule of DESIGN.md sections 3.20 to 3.24, 8 times the worst over
every row of every case.  On a row whose block across the ray is nearly singular, or that lies 1e4 units away, float64's error is a
few large roundings, not a sum of many, and one draw of it can be a hundred times smaller than the next; so the worst of a kind is
pooled over more draws of float64 numpy's own error on the same kind of row: REPEAT rows per kind (tests/landmark_edges.py), both
sizes, both forms, the poses of a pass, the frames of a sequence.

A row is DROPPED from a (pass, bearing_sigma) combination, by name and with the reason, when the classes cannot be demanded equal:
a pivot of the 2 x 2 block across the ray (c11, or d = c22 - c12^2 / c11, in the product's own basis) is below PIVOT times the size
of its terms, an eliminated depth is within MARGIN of 0, or a chi2 is within MARGIN relative of the gate or of delta^2, or float64
numpy itself classifies the row differently.  A dropped row gets a zero bearing in that combination, which every implementation
skips.  The row with Sigma = 0 at bearing_sigma = 0 has S = 0 exactly in any arithmetic: it is never dropped and must be SKIPPED."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import landmark_edges as le
import landmark_fusion_reference as lf
import landmark_register_reference as lr
import landmark_register_robust_reference as rb
import resection_reference as rr
import resection_weighted_reference as wr

LD = lr.LD
EPS = float(np.finfo(np.float64).eps)
PIVOT = 1024 * EPS                   # float64 forms a pivot to about 30 eps of its terms (two 3 x 3 products and a quadratic form)
MARGIN = lr.MARGIN
BEARING_SIGMAS = lr.BEARING_SIGMAS
CAP = 1.0 / 8.0                      # of the edge rows may be dropped from one combination
SKIPPED, BEHIND, GATED, FUSED = lf.SKIPPED, lf.BEHIND, lf.GATED, lf.FUSED


# ---- per row: pivots, errors, bounds ---------------------------------------------------------------------------------------------
def pivots(S, Sg, y):
    """(c11, d) of the product's basis over the size of their terms, long double, per row; exact: S == 0."""
    S, Sg, y = np.asarray(S, dtype=LD), np.asarray(Sg, dtype=LD), np.asarray(y, dtype=LD)
    with np.errstate(all="ignore"):
        b1, b2 = wr.basis(y)
        c11 = np.einsum("ia,iab,ib->i", b1, S, b1)
        c12 = np.einsum("ia,iab,ib->i", b1, S, b2)
        c22 = np.einsum("ia,iab,ib->i", b2, S, b2)
        d = c22 - c12 * c12 / c11
        size = np.sqrt(np.sum(S * S, axis=(1, 2))) + np.sqrt(np.sum(Sg * Sg, axis=(1, 2)))
        p1 = c11 / (np.sum(b1 * b1, axis=1) * size)
        p2 = d / (np.sum(b2 * b2, axis=1) * size)
    zero = ~S.astype(np.float64).any(axis=(1, 2))
    return p1.astype(np.float64), p2.astype(np.float64), zero


def _register_S(X, cov, y, noise2, rot, tran):
    R = rr.rotmat(rot, LD)
    Sg = wr.full(cov, LD)
    with np.errstate(all="ignore"):
        S = R[None] @ Sg @ R.T[None] + np.asarray(noise2, dtype=LD)[:, None, None] * np.eye(3, dtype=LD)[None]
        _, dstar, _, _, _ = rr.per_match(X, y, rot, tran, LD)
    return S, Sg, dstar


def row_errors(got_X, got_cov, got_chi2, ref, prior_X, prior_cov):
    """(n, 3): X+ relative to |X|, Sigma+ relative to the largest entry of the prior Sigma row, chi2 relative to max(chi2, 1) --
    landmark_fusion_reference.errors per row; 0 where the measure does not apply."""
    n = len(ref.cls)
    out = np.zeros((n, 3))
    f, live = ref.cls == FUSED, ref.cls != SKIPPED
    with np.errstate(all="ignore"):
        nX = np.sqrt(np.sum(np.asarray(prior_X, dtype=LD) ** 2, axis=1))
        ex = np.abs(np.asarray(got_X, dtype=LD) - ref.X).max(axis=1) / nX
        sc = np.maximum(np.abs(np.asarray(prior_cov, dtype=LD)).max(axis=1), LD(1e-300))
        ec = np.abs(np.asarray(got_cov, dtype=LD) - ref.cov).max(axis=1) / sc
        es = np.abs(np.asarray(got_chi2, dtype=LD) - ref.chi2) / np.maximum(ref.chi2, 1)
    out[f, 0], out[f, 1], out[live, 2] = ex[f].astype(np.float64), ec[f].astype(np.float64), es[live].astype(np.float64)
    return out


def kinds_of(s, rows):
    """Per row of `rows` (indices into the scene): the case kind, 'ordinary' elsewhere."""
    names = s.names()
    return np.array([le.BY_NAME[names[i]].kind if i in names else "ordinary" for i in rows])


def by_kind(err, kinds):
    """kind -> the worst (k,) errors of its rows."""
    return {k: err[kinds == k].max(axis=0) for k in dict.fromkeys(kinds)}


def pool(qs):
    """kind -> float64 numpy's worst (k,) errors over the rows of that kind in every qualified case of `qs`."""
    out = {}
    for q in qs:
        for k, v in by_kind(q.err, q.kinds).items():
            out[k] = np.maximum(out.get(k, 0.0), v)
    return out


def row_bounds(kinds, pooled):
    """(n, k) bounds: 8 times the pooled worst of the row's kind, at least 8 times the pooled worst of the ordinary rows."""
    floor = pooled["ordinary"]
    return np.stack([8.0 * np.maximum(pooled.get(k, floor), floor) for k in kinds])


@dataclass
class Qualified:
    y: np.ndarray          # the bearings of the rows, zero where dropped
    dropped: dict          # case name -> reason
    ref: object            # the long-double reference on y
    err: np.ndarray        # float64 numpy's per-row (or per-sum) errors against it
    kinds: np.ndarray      # per row
    bounds: np.ndarray     # the case's own row_bounds(kinds, pool([self])), or 8 * err of the sums; the tests pool wider
    got: object = None     # float64 numpy in the product's formulation on y


def _drop(s, rows, y, fails):
    """fails: list of (mask over rows, reason).  -> y with the failing EDGE rows zeroed, name -> reason; an ordinary row that
    fails is an error of the scene."""
    names = s.names()
    y = np.array(y, dtype=np.float64)
    dropped = {}
    for mask, reason in fails:
        for j in np.flatnonzero(mask):
            i = int(rows[j])
            assert i in names, f"{s.name}: ordinary row {i} fails: {reason}"
            dropped.setdefault(names[i], reason)
            y[j] = 0.0
    return y, dropped


def _pivot_fails(S, Sg, y, dstar):
    p1, p2, zero = pivots(S, Sg, y)
    with np.errstate(invalid="ignore"):
        small = ~zero & np.isfinite(p1) & ~((p1 > PIVOT) & (p2 > PIVOT))
        near0 = np.isfinite(dstar.astype(np.float64)) & (np.abs(dstar) <= MARGIN)
    return [(small, f"a pivot of the block across the ray is below {PIVOT:.1e} of its terms"), (near0, "d* within 1e-9 of 0")]


def _near(chi2, bound):
    with np.errstate(invalid="ignore"):
        c = np.asarray(chi2, dtype=LD)
        return np.isfinite(c.astype(np.float64)) & (np.abs(c - bound) <= MARGIN * bound)


def _rows(s, idx):
    rows = np.arange(len(s.X)) if idx is None else np.asarray(idx)
    return rows, s.X[rows], s.cov[rows], s.y[rows]


# ---- the fuse --------------------------------------------------------------------------------------------------------------------
def fuse_at(X, cov, y, rot, tran, bs, pose_cov, s, rows, gate=lf.GATE):
    """Qualify one fuse of the rows (X, cov, y) at (rot, tran)."""
    with np.errstate(all="ignore"):
        Sg, S, _, _, dstar = lf._prior_cov_S(np.asarray(X, dtype=LD), np.asarray(cov, dtype=LD), np.asarray(y, dtype=LD), rot, tran, bs, pose_cov, LD)
        fails = _pivot_fails(S, Sg, y, dstar)
        ref = lf.fuse(X, cov, y, rot, tran, bs, gate, pose_cov, projected=True)
        b = lf.fuse_basis(X, cov, y, rot, tran, bs, gate, pose_cov)
    fails += [(_near(ref.chi2, gate), "chi2 within 1e-9 of the gate"), (ref.cls != b.cls, "float64 numpy classifies it differently")]
    y2, dropped = _drop(s, rows, y, fails)
    with np.errstate(all="ignore"):
        ref = lf.fuse(X, cov, y2, rot, tran, bs, gate, pose_cov, projected=True)
        b = lf.fuse_basis(X, cov, y2, rot, tran, bs, gate, pose_cov)
    assert np.array_equal(ref.cls, b.cls)

    err = row_errors(b.X, b.cov, b.chi2, ref, X, cov)
    kinds = kinds_of(s, rows)
    return Qualified(y2, dropped, ref, err, kinds, row_bounds(kinds, by_kind(err, kinds)), b)


@lru_cache(maxsize=None)
def _fuse(n, bs, with_pose_cov, indexed):
    s = le.scene(n)
    rows, X, cov, y = _rows(s, le.subset(s) if indexed else None)
    return fuse_at(X, cov, y, s.rot, s.tran, bs, lf.POSE_COV_FULL if with_pose_cov else None, s, rows)


def fuse(n, bs, with_pose_cov, indexed):
    return _fuse(n, bs, bool(with_pose_cov), bool(indexed))


# ---- the freeze and one evaluation -----------------------------------------------------------------------------------------------
@dataclass
class QualifiedEval(Qualified):
    noise: np.ndarray = None       # long double, frozen at the scene's reference pose
    cls: np.ndarray = None         # the freeze's classes
    noise64: np.ndarray = None     # float64 numpy's


def _freeze_fails(s, rows, X, cov, y, bs, rot_ref, tran_ref):
    with np.errstate(all="ignore"):
        _, dref, _, _, _ = rr.per_match(X, y, rot_ref, tran_ref, LD)
        s2 = LD(bs) ** 2 * dref * dref * np.sum(np.asarray(y, dtype=LD) ** 2, axis=1)
        s2 = np.where(np.isfinite(s2.astype(np.float64)), s2, LD(0))
        S, Sg, dstar = _register_S(X, cov, y, s2, rot_ref, tran_ref)
    return _pivot_fails(S, Sg, y, dstar), s2


def evaluation(s, bs, idx=None, delta=None, rot=None, tran=None, rot_ref=None, tran_ref=None, gate=None, state=None):
    """Qualify the freeze at (rot_ref, tran_ref) and one evaluation at (rot, tran) -- by default the scene's; delta: the robust pass;
    gate: also the write-back's chi2 against it; state: (X, cov, y) of every row instead of the scene's own, a handle's state in a
    sequence.  err and bounds: (H, g, cost)."""
    rows, X, cov, y = _rows(s, idx)
    if state is not None:
        X, cov, y = state
    rot, tran = (s.rot, s.tran) if rot is None else (rot, tran)
    rot_ref, tran_ref = (s.rot_ref, s.tran_ref) if rot_ref is None else (rot_ref, tran_ref)
    fails, s2 = _freeze_fails(s, rows, X, cov, y, bs, rot_ref, tran_ref)
    with np.errstate(all="ignore"):
        S, Sg, dstar = _register_S(X, cov, y, s2, rot, tran)
        fails += _pivot_fails(S, Sg, y, dstar)
        noise, cls = lr.freeze(X, cov, y, rot_ref, tran_ref, bs, basis=lr.PROJECTED)
        nb, cb = lr.freeze(X, cov, y, rot_ref, tran_ref, bs, np.float64, basis=True)
        chi2, used = rb.chi2_at(X, cov, y, noise, rot, tran, basis=lr.PROJECTED)
    fails.append((cls != cb, "float64 numpy's freeze classifies it differently"))
    for bound, what in ((None if delta is None else delta * delta, "delta^2"), (gate, "the gate")):
        if bound is not None and np.isfinite(bound):
            fails.append((used & _near(chi2, bound), f"chi2 within 1e-9 of {what}"))
    y2, dropped = _drop(s, rows, y, fails)
    with np.errstate(all="ignore"):
        noise, cls = lr.freeze(X, cov, y2, rot_ref, tran_ref, bs, basis=lr.PROJECTED)
        nb, cb = lr.freeze(X, cov, y2, rot_ref, tran_ref, bs, np.float64, basis=True)
        assert np.array_equal(cls, cb), s.name
        if delta is None:
            ref = lr.evaluate(X, cov, y2, noise, rot, tran, basis=lr.PROJECTED)
            got = lr.evaluate(X, cov, y2, nb, rot, tran, np.float64, basis=True)
        else:
            ref = rb.evaluate(X, cov, y2, noise, rot, tran, delta, basis=lr.PROJECTED)
            got = rb.evaluate(X, cov, y2, nb, rot, tran, delta, np.float64, basis=True)
            assert got.n_outlier == ref.n_outlier, s.name
    assert (got.n_used, got.n_behind) == (ref.n_used, ref.n_behind), s.name

    err = np.array(lr.eq_errors(got, ref))
    return QualifiedEval(y2, dropped, ref, err, kinds_of(s, rows), 8.0 * err, got, noise, cls, nb)


@lru_cache(maxsize=None)
def eval_bounds(bs, robust):
    """8 times float64 numpy's worst (H, g, cost) errors over every evaluation of this bearing_sigma and loss: both sizes, the
    poses of landmark_register_robust_reference.POSE_NAMES, dense and indexed.  The sums are dominated by their worst-conditioned
    rows, whose error is one draw of a large rounding error per evaluation; the worst of these draws is what one more is held to."""
    worst = np.zeros(3)
    for n, _ in le.SIZES:
        for pose in rb.POSE_NAMES:
            s = le.scene(n, pose)
            for _, idx in le.forms(s):
                worst = np.maximum(worst, evaluation(s, bs, idx, rb.DELTA if robust else None).err)
    return 8.0 * worst


@lru_cache(maxsize=None)
def fuse_pool(bs, with_pose_cov):
    """float64 numpy's worst errors per kind over the fuses of both sizes and both forms."""
    return pool([fuse(n, bs, with_pose_cov, indexed) for n, _ in le.SIZES for indexed in (False, True)])


# ---- the write-back --------------------------------------------------------------------------------------------------------------
@dataclass
class QualifiedPost(Qualified):
    pose_cov_err: float = 0.0
    noise: np.ndarray = None
    noise64: np.ndarray = None


def posterior(s, bs, idx=None, delta=None, gate=None, rot=None, tran=None, rot_ref=None, tran_ref=None, state=None):
    """Qualify the write-back at (rot, tran) with the noise frozen at (rot_ref, tran_ref).  delta: the robust pass; state as for
    `evaluation`."""
    rows, X, cov, _ = _rows(s, idx)
    if state is not None:
        X, cov, _ = state
    gate = (lr.GATE if delta is None else rb.GATE) if gate is None else gate
    q = evaluation(s, bs, idx, delta, rot, tran, rot_ref, tran_ref, gate, state)
    rot, tran = (s.rot, s.tran) if rot is None else (rot, tran)
    rot_ref, tran_ref = (s.rot_ref, s.tran_ref) if rot_ref is None else (rot_ref, tran_ref)
    y2 = q.y
    with np.errstate(all="ignore"):
        noise, _ = lr.freeze(X, cov, y2, rot_ref, tran_ref, bs, basis=lr.PROJECTED)
        nb, _ = lr.freeze(X, cov, y2, rot_ref, tran_ref, bs, np.float64, basis=True)
        if delta is None:
            ref = lr.posterior(X, cov, y2, noise, rot, tran, gate, basis=lr.PROJECTED)
            b = lr.posterior(X, cov, y2, nb, rot, tran, gate, np.float64, basis=True)
        else:
            ref = rb.posterior(X, cov, y2, noise, rot, tran, delta, gate, basis=lr.PROJECTED)
            b = rb.posterior(X, cov, y2, nb, rot, tran, delta, gate, np.float64, basis=True)
    assert np.array_equal(ref.cls, b.cls), (s.name, np.flatnonzero(ref.cls != b.cls))

    err = row_errors(b.X, b.cov, b.chi2, ref, X, cov)
    sd = np.sqrt(np.diag(ref.pose_cov))
    ep = float((np.abs(np.asarray(b.pose_cov, dtype=LD) - ref.pose_cov) / (sd[:, None] * sd[None, :])).max())
    kinds = kinds_of(s, rows)
    return QualifiedPost(y2, q.dropped, ref, err, kinds, row_bounds(kinds, by_kind(err, kinds)), b, ep, noise, nb)


def check_cap(dropped, what):
    """No more than CAP of the edge rows dropped from one combination."""
    assert len(dropped) <= CAP * len(le.CASES), f"{what}: {len(dropped)} of {len(le.CASES)} edge rows dropped: {dropped}"


def dropped_kinds(dropped):
    return {le.BY_NAME[k].kind for k in dropped}


# ---- six frames in sequence ------------------------------------------------------------------------------------------------------
SEQUENCE_BEARING_SIGMA = 1e-3        # with no bearing noise in the model a fused landmark has no variance left across its ray
SEQUENCE_FRAMES = 6


@lru_cache(maxsize=None)
def sequence(n):
    """Frames (bearings, rot, tran) onto le.scene(n): the scene's own pose and bearings first, then five seeded poses, each 0.1 to
    0.3 rad and 0.3 units from the one before, that see every TRUE landmark with bearing noise 1e-3 and the lengths of frame 0."""
    s = le.scene(n)
    rng = np.random.default_rng(61000 + n)
    frames = [(np.array(s.y), s.rot.copy(), s.tran.copy())]
    length = np.linalg.norm(s.y, axis=1, keepdims=True)
    rot, tran = s.truth_rot.copy(), s.truth_tran.copy()
    for _ in range(SEQUENCE_FRAMES - 1):
        rot = rot + rng.uniform(0.1, 0.3) * rr._unit(rng.standard_normal(3))
        tran = tran + 0.3 * rr._unit(rng.standard_normal(3))
        Y = s.truth_X @ rr.rotmat(rot, np.float64).T - tran
        yk = rr._unit(rr._unit(Y) + 1e-3 * rng.standard_normal((n, 3))) * length
        frames.append((yk, rot.copy(), tran.copy()))
    for yk, _, _ in frames:
        yk.setflags(write=False)
    return tuple(frames)


@lru_cache(maxsize=None)
def posterior_pool(bs, robust, at_the_truth):
    """float64 numpy's worst errors per kind over the write-backs of both sizes and both forms: at_the_truth, frozen and
    evaluated at the pose the edge rows were placed at (le.scene(n)); else the scenes of the three evaluation poses."""
    qs = []
    for n, _ in le.SIZES:
        for s in ([le.scene(n)] if at_the_truth else [le.scene(n, p) for p in rb.POSE_NAMES]):
            ref_pose = dict(rot_ref=s.rot, tran_ref=s.tran) if at_the_truth else {}
            qs += [posterior(s, bs, idx, rb.DELTA if robust else None, **ref_pose) for _, idx in le.forms(s)]
    return pool(qs)


@lru_cache(maxsize=None)
def sequence_fuse(n):
    """The float64 recursion (the product's formulation feeding itself) over sequence(n): the qualified step of every frame."""
    s = le.scene(n)
    X, C, out = np.array(s.X), np.array(s.cov), []
    for yk, rot, tran in sequence(n):
        q = fuse_at(X, C, yk, rot, tran, SEQUENCE_BEARING_SIGMA, None, s, np.arange(n))
        X, C = q.got.X, q.got.cov
        out.append(q)
    return tuple(out)


@lru_cache(maxsize=None)
def sequence_fuse_pool():
    """float64 numpy's worst errors per kind over every frame of the fuse recursion at both sizes."""
    return pool([q for n, _ in le.SIZES for q in sequence_fuse(n)])


def sequence_start(n, k, rot):
    """The start of frame k's robust registration: 2e-3 rad off the frame's pose along a seeded direction."""
    return rot + 2e-3 * rr._unit(np.random.default_rng(62000 + 10 * n + k).standard_normal(3))


@lru_cache(maxsize=None)
def sequence_register_pool():
    """float64 numpy's worst errors per kind over every frame of the robust registration recursion at both sizes: each frame
    solved by the long-double reference from sequence_start, the write-back qualified at its minimiser, float64 numpy's posterior
    the next frame's state."""
    qs = []
    for n, _ in le.SIZES:
        s = le.scene(n)
        X, C = np.array(s.X), np.array(s.cov)
        for k, (yk, rot, tran) in enumerate(sequence(n)):
            y = sequence_fuse(n)[k].y
            start = sequence_start(n, k, rot)
            with np.errstate(all="ignore"):
                noise, _ = lr.freeze(X, C, y, start, tran, SEQUENCE_BEARING_SIGMA, basis=lr.PROJECTED)
                rot_r, tran_r, _, _ = rb.solve(X, C, y, noise, start, tran, rb.DELTA, basis=lr.PROJECTED)
            q = posterior(s, SEQUENCE_BEARING_SIGMA, None, rb.DELTA, rot=rot_r, tran=tran_r, rot_ref=start, tran_ref=tran, state=(X, C, y))
            X, C = np.asarray(q.got.X, dtype=np.float64), np.asarray(q.got.cov, dtype=np.float64)
            qs.append(q)
    return pool(qs)
