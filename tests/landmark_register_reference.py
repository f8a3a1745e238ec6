"""Shared by the joint-registration tests (tests/ only): numpy restatements of Landmarks.eval_register / register, the cases
the CPU qualification and the GPU tests walk, and the g++-built harness around csrc/sba_landmarks_register.hpp.

Unknowns: the pose (w, t) and every observed landmark X_j with the prior N(Xb_j, Sigma_j); the bearing noise across the ray,
s_j^2 = bearing_sigma^2 d*_j^2 (y . y), is frozen at a reference pose and Xb_j.  Per observation at a pose:

    c = -R Xb + t,   d* = -(y . c) / (y . y),   r = c + d* y,   S = R Sigma R^T + s_j^2 I
    M = S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y),   chi2 = r^T M r,   Xh = Xb + Sigma R^T M r,   Sigma_cond = Sigma - Sigma R^T M R Sigma
    F = [A(Xh) | I],   H = sum F^T M F,   g = sum F^T M r,   cost = 1/2 sum chi2
    Sigma_c = H^-1,   G = Sigma R^T M F,   X+ = Xh,   Sigma+ = Sigma_cond + G Sigma_c G^T,   Cov(X, pose) = G Sigma_c

The REFERENCE (freeze, evaluate, solve, posterior) is this basis-free form in numpy long double per observation: M as
tests/resection_weighted_reference.py forms it (the 3 x 3 inverse by the adjugate), the Jacobian from tests/resection_reference.py,
a Levenberg-Marquardt loop of its own run to a step below 1e-13.  The BASIS FORM (dtype float64, basis=True) is the product's
formulation -- b1 = e_k x y, b2 = y x b1, the Cholesky factor of B^T S B, W = G^-1 B^T, u = W r, T = Sigma R^T W^T, J_w = W F -- in
numpy's own order of operations: its error against the reference is what float64 can do, and 8 times that is what the device is
held to."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import landmark_fusion_reference as lf
import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr

LD = np.longdouble
SKIPPED, BEHIND, GATED, FUSED = lf.SKIPPED, lf.BEHIND, lf.GATED, lf.FUSED
LIVE = FUSED                         # the freeze's class of an observation that takes part
GATE = lf.GATE
BEARING_SIGMAS = (0.0, 1e-3)
SIZES = (1, 2, 3, 63, 64, 65, 511, 512, 513)
LONG = (1537, 3073)                  # SBA_RESECT_GRID=1: one block takes several steps with a partial last wave
SOLVE_SIZES = (63, 65, 513)
SOLVE_LONG = (1537,)
MARGIN = 1e-9
FREEZE_OFFSET = 1e-2                 # rad: the evaluation pose against the freeze pose
START_ROT, START_TRAN = 2e-3, 1e-2   # the solve's start against the truth


# ---- per observation at a pose ---------------------------------------------------------------------------------------------------
@dataclass
class Point:
    R: np.ndarray
    Sg: np.ndarray         # (n, 3, 3)
    r: np.ndarray          # (n, 3)
    dstar: np.ndarray
    bad: np.ndarray        # the factor fails: S is not positive definite across the bearing, or d* is not finite
    M: np.ndarray          # (n, 3, 3), zero where bad (basis form: W^T W)
    W: np.ndarray | None   # (n, 2, 3), the basis form only


PROJECTED = "projected"             # point(..., basis=PROJECTED): the reference formulation that forms no S^-1


def _pd_across(S, y, dtype):
    _, _, c11, c12, c22 = wr.across(S, y, dtype)
    return (c11 > 0) & (c11 * c22 - c12 * c12 > 0)


projected_weight = wr.projected_weight


def point(X, cov6, y, noise2, rot, tran, dtype=LD, basis=False):
    """X, cov6, y: rows of observations with finite entries; noise2 (n,) >= 0."""
    X, y, cov6 = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(cov6, dtype=dtype).reshape(-1, 6)
    R = rr.rotmat(rot, dtype)
    with np.errstate(all="ignore"):
        _, dstar, r, _, _ = rr.per_match(X, y, rot, tran, dtype)
        Sg = wr.full(cov6, dtype)
        S = R[None] @ Sg @ R.T[None] + np.asarray(noise2, dtype=dtype)[:, None, None] * np.eye(3, dtype=dtype)[None]
        if basis is True:
            b1, b2 = wr.basis(y)
            c11 = np.einsum("ia,iab,ib->i", b1, S, b1)
            c12 = np.einsum("ia,iab,ib->i", b1, S, b2)
            c22 = np.einsum("ia,iab,ib->i", b2, S, b2)
            g11 = np.sqrt(c11)
            g21 = c12 / g11
            d = c22 - g21 * g21
            g22 = np.sqrt(d)
            q = np.stack([1 / g11, -g21 / (g11 * g22), 1 / g22], axis=1)
            ok = (c11 > 0) & (d > 0) & np.isfinite(q).all(axis=1) & (q[:, 0] > 0) & (q[:, 2] > 0) & np.isfinite(dstar)
            q = np.where(ok[:, None], q, dtype(0))
            W = np.stack([q[:, 0:1] * b1, q[:, 1:2] * b1 + q[:, 2:3] * b2], axis=1)
            return Point(R, Sg, r, dstar, ~ok, np.einsum("ika,ikb->iab", W, W), W)
        bad = ~np.isfinite(dstar.astype(np.float64)) | ~np.isfinite(S.astype(np.float64)).all(axis=(1, 2))
        ysafe = np.where(bad[:, None], np.array([1, 0, 0], dtype=dtype)[None], y)
        Ssafe = np.where(bad[:, None, None], np.eye(3, dtype=dtype)[None], S)
        bad |= ~_pd_across(Ssafe, ysafe, dtype)
        Ssafe = np.where(bad[:, None, None], np.eye(3, dtype=dtype)[None], S)
        ysafe = np.where(bad[:, None], np.array([1, 0, 0], dtype=dtype)[None], y)
        if basis == PROJECTED:
            M = projected_weight(Ssafe, ysafe, dtype)
        else:
            Si, _ = wr._adjugate_inverse(Ssafe)
            v = np.einsum("iab,ib->ia", Si, ysafe)
            M = Si - v[:, :, None] * v[:, None, :] / np.sum(v * ysafe, axis=1)[:, None, None]
        M = np.where(bad[:, None, None], dtype(0), M)
        r = np.where(bad[:, None], dtype(0), r)
    return Point(R, Sg, r, dstar, bad, M, None)


def _finite_rows(X, cov6, y):
    f = lambda a: np.isfinite(np.asarray(a, dtype=np.float64)).all(axis=1)
    return f(X) & f(np.asarray(cov6).reshape(-1, 6)) & f(y)


# ---- the freeze ------------------------------------------------------------------------------------------------------------------
def freeze(X, cov6, y, rot_ref, tran_ref, bearing_sigma, dtype=LD, basis=False):
    """-> noise (n,) in `dtype`: s_j^2 of an observation that takes part, -s_j^2 (sign bit set) of one behind, NaN of one
    skipped; cls (n,) int: SKIPPED, BEHIND or LIVE."""
    n = len(X)
    noise, cls = np.full(n, np.nan, dtype=dtype), np.full(n, SKIPPED, dtype=int)
    if n == 0:
        return noise, cls
    fin = _finite_rows(X, cov6, y)
    Xs, Cs, ys = (np.asarray(a, dtype=np.float64)[fin] for a in (X, np.asarray(cov6).reshape(-1, 6), y))
    with np.errstate(all="ignore"):
        _, dstar, _, _, _ = rr.per_match(Xs, ys, rot_ref, tran_ref, dtype)
        s2 = dtype(bearing_sigma) ** 2 * dstar * dstar * np.sum(np.asarray(ys, dtype=dtype) ** 2, axis=1)
        okn = np.isfinite(s2.astype(np.float64)) & np.isfinite(dstar.astype(np.float64))
        pt = point(Xs, Cs, ys, np.where(okn, s2, dtype(0)), rot_ref, tran_ref, dtype, basis)
        ok = okn & ~pt.bad
        behind = ok & (dstar <= 0)
    sub_noise = np.where(ok, np.where(behind, -s2, s2), dtype(np.nan))
    sub_cls = np.where(ok, np.where(behind, BEHIND, LIVE), SKIPPED)
    noise[fin], cls[fin] = sub_noise, sub_cls
    return noise, cls


def live_of(noise):
    with np.errstate(invalid="ignore"):
        return ~np.isnan(noise.astype(np.float64)) & ~np.signbit(noise.astype(np.float64))


# ---- one evaluation --------------------------------------------------------------------------------------------------------------
@dataclass
class Equations:
    H: np.ndarray
    g: np.ndarray
    cost: float
    n_used: int
    n_behind: int


def _jacobian(pt, Xh, rot, dtype):
    A = -rr.rotated_jacobians(rot, Xh, dtype)
    return np.concatenate([A, np.broadcast_to(np.eye(3, dtype=dtype), (len(Xh), 3, 3))], axis=2)


def evaluate(X, cov6, y, noise, rot, tran, dtype=LD, basis=False, raw=False):
    """The reduce pass's sums at (rot, tran) over the observations that take part; raw: H, g in `dtype` instead of float64."""
    live = live_of(noise)
    if not live.any():
        return Equations(np.zeros((6, 6)), np.zeros(6), 0.0, 0, 0)
    Xs, Cs, ys = (np.asarray(a, dtype=np.float64)[live] for a in (X, np.asarray(cov6).reshape(-1, 6), y))
    pt = point(Xs, Cs, ys, np.asarray(noise, dtype=dtype)[live], rot, tran, dtype, basis)
    with np.errstate(all="ignore"):
        GM = pt.Sg @ pt.R.T[None] @ pt.M
        Xh = np.asarray(Xs, dtype=dtype) + np.einsum("iab,ib->ia", GM, pt.r)
        F = _jacobian(pt, Xh, rot, dtype)
        if basis is True:
            Jw = pt.W @ F
            u = np.einsum("ika,ia->ik", pt.W, pt.r)
            H, g, chi2 = np.einsum("ika,ikb->ab", Jw, Jw), np.einsum("ika,ik->a", Jw, u), np.sum(u * u, axis=1)
        else:
            MF = pt.M @ F
            H, g, chi2 = np.einsum("ika,ikb->ab", F, MF), np.einsum("ika,ik->a", MF, pt.r), np.einsum("ia,iab,ib->i", pt.r, pt.M, pt.r)
    used = ~pt.bad
    out = (H, g) if raw else (H.astype(np.float64), g.astype(np.float64))
    cost = 0.5 * chi2.sum()
    return Equations(out[0], out[1], cost if raw else float(cost), int(used.sum()), int((used & (pt.dstar <= 0)).sum()))


def eq_errors(got, ref):
    """(H relative to its largest entry, g relative to its largest entry, cost relative): the normalisation of
    tests/helpers.py's assert_normal_eq_close, which tests/test_gpu_resection_weighted.py compares the weighted row by."""
    sH = max(np.abs(ref.H).max(), 1e-300)
    sg = max(np.abs(ref.g).max(), 1e-300)
    return (float(np.abs(np.asarray(got.H, dtype=LD) - ref.H).max() / sH), float(np.abs(np.asarray(got.g, dtype=LD) - ref.g).max() / sg),
            float(abs(LD(got.cost) - LD(ref.cost)) / max(abs(ref.cost), 1e-300)))


# ---- the solve: a Levenberg-Marquardt loop of its own --------------------------------------------------------------------------
def solve(X, cov6, y, noise, rot, tran, dtype=LD, max_iterations=200, step_tol=1e-13, basis=False):
    """-> rot, tran (float64), the Equations there, iterations.  Damping lam diag(H): accepted steps divide lam by 3, rejected
    ones multiply it by 4; stops when an accepted step is below step_tol in every parameter."""
    p = np.concatenate([np.asarray(rot, dtype=np.float64), np.asarray(tran, dtype=np.float64)]).astype(dtype)
    e = evaluate(X, cov6, y, noise, p[:3], p[3:], dtype, basis, raw=True)
    lam, it = dtype(1e-4), 0
    for it in range(1, max_iterations + 1):
        H, g = np.asarray(e.H, dtype=dtype), np.asarray(e.g, dtype=dtype)
        d = -(wr.inverse_ld(H + lam * np.diag(np.diag(H))) @ g)
        q = p + d
        e2 = evaluate(X, cov6, y, noise, q[:3], q[3:], dtype, basis, raw=True)
        if e2.cost <= e.cost:
            p, e, lam = q, e2, lam / 3
            if np.abs(d).max() < step_tol:
                break
        else:
            lam = lam * 4
            if lam > 1e12:
                break
    # Where the cost's own rounding (the adjugate inverse cancels to about 1e4 eps) hides the decrease of the last steps, the loop
    # above stalls a few 1e-10 short: finish with undamped steps, accepted while they shrink the gradient (which is exact).
    for _ in range(10):
        H, g = np.asarray(e.H, dtype=dtype), np.asarray(e.g, dtype=dtype)
        d = -(wr.inverse_ld(H) @ g)
        if np.abs(d).max() < step_tol:
            break
        q = p + d
        e2 = evaluate(X, cov6, y, noise, q[:3], q[3:], dtype, basis, raw=True)
        if not np.abs(e2.g).max() < np.abs(e.g).max():
            break
        p, e = q, e2
    p64 = p.astype(np.float64)
    return p64[:3], p64[3:], evaluate(X, cov6, y, noise, p64[:3], p64[3:], dtype, basis), it


# ---- the posterior at a pose -----------------------------------------------------------------------------------------------------
@dataclass
class Registered:
    X: np.ndarray          # (m, 3) posterior where cls == FUSED, the prior elsewhere
    cov: np.ndarray        # (m, 6)
    chi2: np.ndarray       # (m,) NaN where skipped
    cls: np.ndarray        # (m,) int
    dstar: np.ndarray      # (m,) at the pose (NaN where the freeze skipped)
    pose_cov: np.ndarray   # (6, 6) Sigma_c
    cross: np.ndarray      # (m, 3, 6) G Sigma_c (zeros where not fused)
    eq: Equations

    def counts(self):
        """(n_obs, n_skipped, n_behind, n_gated, n_fused)"""
        return (len(self.cls),) + tuple(int((self.cls == k).sum()) for k in (SKIPPED, BEHIND, GATED, FUSED))


def posterior(X, cov6, y, noise, rot, tran, gate=np.inf, dtype=LD, basis=False):
    """The write-back at (rot, tran): Sigma_c from the sums there, then per observation the class, chi2, X+ and Sigma+."""
    m = len(X)
    X0, C0 = np.asarray(X, dtype=dtype), np.asarray(cov6, dtype=dtype).reshape(-1, 6)
    eq = evaluate(X, cov6, y, noise, rot, tran, dtype, basis, raw=True)
    Sc = wr.inverse_ld(eq.H).astype(dtype)
    Sc = (Sc + Sc.T) / 2
    marked = np.isnan(np.asarray(noise, dtype=np.float64))
    cls = np.full(m, SKIPPED, dtype=int)
    Xo, Co, chi2 = X0.copy(), C0.copy(), np.full(m, np.nan, dtype=dtype)
    dstar_all, cross = np.full(m, np.nan, dtype=dtype), np.zeros((m, 3, 6), dtype=dtype)
    rows = np.flatnonzero(~marked)
    if len(rows):
        Xs, Cs, ys = (np.asarray(a, dtype=np.float64)[rows] for a in (X, np.asarray(cov6).reshape(-1, 6), y))
        nz = np.asarray(noise, dtype=dtype)[rows]
        pt = point(Xs, Cs, ys, np.abs(nz), rot, tran, dtype, basis)
        with np.errstate(all="ignore"):
            GM = pt.Sg @ pt.R.T[None] @ pt.M
            Xh = np.asarray(Xs, dtype=dtype) + np.einsum("iab,ib->ia", GM, pt.r)
            F = _jacobian(pt, Xh, rot, dtype)
            if basis is True:
                T = pt.Sg @ pt.R.T[None] @ np.swapaxes(pt.W, 1, 2)
                cond = pt.Sg - T @ np.swapaxes(T, 1, 2)
                G = T @ (pt.W @ F)
                u = np.einsum("ika,ia->ik", pt.W, pt.r)
                s = np.sum(u * u, axis=1)
            else:
                cond = pt.Sg - GM @ np.swapaxes(pt.Sg @ pt.R.T[None], 1, 2)
                G = GM @ F
                s = np.einsum("ia,iab,ib->i", pt.r, pt.M, pt.r)
            Cp = wr.rows_of(cond + G @ Sc[None] @ np.swapaxes(G, 1, 2))
            bad = pt.bad | ~np.isfinite(Xh.astype(np.float64)).all(axis=1) | ~np.isfinite(Cp.astype(np.float64)).all(axis=1)
            behind = np.signbit(nz.astype(np.float64)) | (pt.dstar <= 0)
            c = np.where(bad, SKIPPED, np.where(behind, BEHIND, np.where(s > dtype(gate), GATED, FUSED))).astype(int)
        f = c == FUSED
        cls[rows] = c
        Xo[rows] = np.where(f[:, None], Xh, Xo[rows])
        Co[rows] = np.where(f[:, None], Cp, Co[rows])
        chi2[rows] = np.where(c == SKIPPED, dtype(np.nan), s)
        dstar_all[rows] = pt.dstar
        cross[rows] = np.where(f[:, None, None], G @ Sc[None], dtype(0))
    out_eq = Equations(eq.H.astype(np.float64), eq.g.astype(np.float64), eq.cost, eq.n_used, eq.n_behind)
    return Registered(Xo, Co, chi2, cls, dstar_all, Sc, cross, out_eq)


def post_errors(got_X, got_cov, got_chi2, got_pose_cov, ref, prior_X, prior_cov):
    """(X+, Sigma+, chi2) in the normalisations of landmark_fusion_reference.errors, and Sigma_c relative to sqrt(c_ii c_jj)."""
    ex, ec, es = lf.errors(got_X, got_cov, got_chi2, ref, prior_X, prior_cov)
    sd = np.sqrt(np.diag(ref.pose_cov))
    ep = float((np.abs(np.asarray(got_pose_cov, dtype=LD) - ref.pose_cov) / (sd[:, None] * sd[None, :])).max())
    return ex, ec, es, ep


# ---- the cases the CPU qualification and the GPU tests share ------------------------------------------------------------------
@dataclass(frozen=True)
class Scene:
    name: str
    X: np.ndarray          # (n, 3) prior landmarks, as given to set()
    cov: np.ndarray        # (n, 6) as given to set() with cov_scale 1
    y: np.ndarray          # (n, 3) bearings, lengths in [0.5, 2]
    rot: np.ndarray        # the evaluation pose
    tran: np.ndarray
    rot_ref: np.ndarray    # the freeze pose, FREEZE_OFFSET away
    tran_ref: np.ndarray
    truth_X: np.ndarray
    grid_one: bool = False


@lru_cache(maxsize=None)
def scene(n, pose_name):
    """The scene recipe of landmark_fusion_reference.scene: n landmarks drawn from their covariances around a truth whose rotation
    is 0.2 degrees off POSES[pose_name], bearing noise 1e-3, bearings scaled to lengths in [0.5, 2].  Evaluated AT POSES[pose_name],
    frozen 1e-2 rad (and 1e-2 units) away along seeded directions."""
    w = pose_edges.POSES[pose_name]
    seed = 900 + n
    s = rr.make_scene(n, seed, noise=1e-3, rot=w + np.deg2rad(0.2) * wr.EDGE_AXIS)
    cov, root = wr.landmark_cov(s.X, seed)
    rng = np.random.default_rng(seed + 5151)
    X = s.X + np.einsum("iab,ib->ia", root, rng.standard_normal((n, 3)))
    y = s.y * rng.uniform(0.5, 2.0, size=(n, 1))
    dr, dt = rr._unit(rng.standard_normal(3)), rr._unit(rng.standard_normal(3))
    for a in (X, y, cov):
        a.setflags(write=False)
    return Scene(f"n={n} {pose_name}", X, cov, y, w.copy(), s.tran.copy(), w + FREEZE_OFFSET * dr, s.tran + FREEZE_OFFSET * dt, s.X, n in LONG)


def scenes(sizes=SIZES + LONG):
    return [scene(n, name) for n in sizes for name in pose_edges.NAMES]


def subset(n):
    """About half the landmarks, strictly increasing: the indexed form's idx."""
    rng = np.random.default_rng(4343 + n)
    return np.flatnonzero(rng.random(n) < 0.5).astype(np.int64)


def forms(s):
    """(name, idx or None) of the dense and the indexed run of a scene."""
    return (("dense", None), ("indexed", subset(len(s.X))))


def _rows(s, idx):
    return (s.X, s.cov, s.y) if idx is None else (s.X[idx], s.cov[idx], s.y[idx])


@lru_cache(maxsize=None)
def eval_reference(n, pose_name, bs, indexed):
    """Long double: (noise, freeze classes, Equations) of a scene's dense or indexed evaluation."""
    s = scene(n, pose_name)
    X, cov, y = _rows(s, subset(n) if indexed else None)
    noise, cls = freeze(X, cov, y, s.rot_ref, s.tran_ref, bs)
    return noise, cls, evaluate(X, cov, y, noise, s.rot, s.tran)


def qualify_eval(s, bs, indexed):
    """float64 numpy in the product's formulation classifies as long double does and keeps the margins -> its (H, g, cost) errors."""
    n = len(s.X)
    X, cov, y = _rows(s, subset(n) if indexed else None)
    noise, cls, ref = eval_reference(n, s.name.split()[1], bs, indexed)
    nb, cb = freeze(X, cov, y, s.rot_ref, s.tran_ref, bs, np.float64, basis=True)
    assert np.array_equal(cls, cb), s.name
    got = evaluate(X, cov, y, nb, s.rot, s.tran, np.float64, basis=True)
    assert (got.n_used, got.n_behind) == (ref.n_used, ref.n_behind), s.name
    if len(X):
        _, d_ref, _, _, _ = rr.per_match(X, y, s.rot_ref, s.tran_ref, LD)
        _, d_at, _, _, _ = rr.per_match(X, y, s.rot, s.tran, LD)
        assert (np.abs(d_ref) > MARGIN).all() and (np.abs(d_at) > MARGIN).all(), s.name
    if ref.n_used == 0:
        return 0.0, 0.0, 0.0
    return eq_errors(got, ref)


@lru_cache(maxsize=None)
def measured_eval_errors():
    """float64 numpy's worst (H, g, cost) errors against long double over EVERY evaluation the GPU test runs."""
    worst = np.zeros(3)
    for s in scenes():
        for bs in BEARING_SIGMAS:
            for indexed in (False, True):
                worst = np.maximum(worst, qualify_eval(s, bs, indexed))
    return tuple(float(v) for v in worst)


# ---- the solve scenes ------------------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class SolveScene:
    name: str
    X: np.ndarray
    cov: np.ndarray
    y: np.ndarray
    rot0: np.ndarray       # the start
    tran0: np.ndarray
    truth: rr.Scene
    bearing_sigma: float
    grid_one: bool = False


@lru_cache(maxsize=None)
def solve_scene(n, seed=None, bearing_noise=1e-3):
    """Section 3.20's recipe (resection_weighted_reference.noisy_scene): priors drawn from their covariances, bearing noise 1e-3,
    the start 2e-3 rad and 1e-2 units off the truth along seeded directions."""
    seed = 7000 + n if seed is None else seed
    ns = wr.noisy_scene(n, seed, bearing_noise)
    r0, t0 = rr.start_near(ns.scene, seed, START_ROT, START_TRAN)
    return SolveScene(f"n={n} seed={seed}", ns.X, ns.cov, ns.y, r0, t0, ns.scene, bearing_noise, n in SOLVE_LONG)


@lru_cache(maxsize=None)
def solve_reference(n):
    """Long double: the noise frozen at the start, the minimiser, the Equations there."""
    s = solve_scene(n)
    noise, cls = freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
    rot, tran, eq, it = solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0)
    return noise, cls, rot, tran, eq, it


def qualify_posterior(X, cov, y, rot_ref, tran_ref, rot, tran, bs, gate=GATE, form=False):
    """The posterior at (rot, tran), noise frozen at (rot_ref, tran_ref): float64 in the product's formulation classifies as long
    double does, no chi2 within MARGIN of the gate, no d* within MARGIN of 0 -> (ref, float64's (X+, Sigma+, chi2, Sigma_c) errors).
    form: PROJECTED for the reference that holds for a singular S."""
    noise, cls = freeze(X, cov, y, rot_ref, tran_ref, bs, basis=form)
    ref = posterior(X, cov, y, noise, rot, tran, gate, basis=form)
    nb, cb = freeze(X, cov, y, rot_ref, tran_ref, bs, np.float64, basis=True)
    b = posterior(X, cov, y, nb, rot, tran, gate, np.float64, basis=True)
    assert np.array_equal(cls, cb) and np.array_equal(ref.cls, b.cls)
    live = ref.cls != SKIPPED
    assert (np.abs(ref.chi2[live] - GATE) > MARGIN * GATE).all()
    assert (np.abs(ref.dstar[live]) > MARGIN).all()
    return ref, post_errors(b.X, b.cov, b.chi2, b.pose_cov, ref, X, cov)


# ---- the product's host side through the g++-built harness (tests/harness/landmark_register_harness.cpp) ------------------------
_h = None


def harness():
    """csrc/sba_landmarks_register.hpp compiled for the CPU."""
    global _h
    if _h is None:
        import ctypes as C
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "liblandmark_register_harness.so"
        src = root / "tests" / "harness" / "landmark_register_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f
                for f in ("sba_landmarks_register.hpp", "sba_landmarks.hpp", "sba_resection_weighted.hpp", "sba_resection.hpp", "sba_rotation.hpp",
                          "sba_epipolar.hpp")]
        hdrs.append(root / "include" / "sba_hip.h")
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        dp, ip = C.POINTER(C.c_double), C.POINTER(C.c_int)
        _h.landmark_register_harness_freeze.argtypes = [C.c_longlong, dp, dp, dp, dp, dp, C.c_double, dp, ip]
        _h.landmark_register_harness_eval.argtypes = [C.c_longlong, dp, dp, dp, dp, dp, dp, dp]
        _h.landmark_register_harness_apply.argtypes = [C.c_longlong, dp, dp, dp, dp, dp, dp, dp, C.c_double, dp, dp, dp, ip]
        _h.landmark_register_harness_check_loss.argtypes = [C.c_double]
    return _h


def _a(v):
    return np.ascontiguousarray(v, dtype=np.float64)


def harness_freeze(X, cov6, y, rot_ref, tran_ref, bearing_sigma):
    """landmark_register_fill + landmark_register_noise per row -> noise (float64), classes."""
    import ctypes as C
    X, cov6, y, rot_ref, tran_ref = _a(X), _a(cov6), _a(y), _a(rot_ref), _a(tran_ref)
    n = len(X)
    noise, cls = np.zeros(n), np.full(n, -1, dtype=np.int32)
    harness().landmark_register_harness_freeze(n, rr._dp(X), rr._dp(cov6), rr._dp(y), rr._dp(rot_ref), rr._dp(tran_ref), float(bearing_sigma),
                                               rr._dp(noise), cls.ctypes.data_as(C.POINTER(C.c_int)))
    return noise, cls.astype(int)


def harness_eval(X, cov6, y, noise, rot, tran):
    """landmark_register_accumulate over the rows into one set of sums, expanded by resect_expand_row -> Equations."""
    X, cov6, y, noise, rot, tran = _a(X), _a(cov6), _a(y), _a(noise), _a(rot), _a(tran)
    out = np.zeros(45)
    harness().landmark_register_harness_eval(len(X), rr._dp(X), rr._dp(cov6), rr._dp(y), rr._dp(noise), rr._dp(rot), rr._dp(tran), rr._dp(out))
    return Equations(out[:36].reshape(6, 6).copy(), out[36:42].copy(), float(out[42]), int(out[43]), int(out[44]))


def harness_apply(X, cov6, y, noise, rot, tran, pose_cov, gate=np.inf):
    """landmark_register_one per row with Sigma_c = pose_cov -> (X+, Sigma+ (the prior where not fused), chi2, classes)."""
    import ctypes as C
    X, cov6, y, noise, rot, tran, pc = _a(X), _a(cov6), _a(y), _a(noise), _a(rot), _a(tran), _a(pose_cov)
    n = len(X)
    Xo, Co, chi2, cls = np.full((n, 3), np.nan), np.full((n, 6), np.nan), np.full(n, np.nan), np.full(n, -1, dtype=np.int32)
    harness().landmark_register_harness_apply(n, rr._dp(X), rr._dp(cov6), rr._dp(y), rr._dp(noise), rr._dp(rot), rr._dp(tran), rr._dp(pc),
                                              float(gate), rr._dp(Xo), rr._dp(Co), rr._dp(chi2), cls.ctypes.data_as(C.POINTER(C.c_int)))
    return Xo, Co, chi2, cls.astype(int)
