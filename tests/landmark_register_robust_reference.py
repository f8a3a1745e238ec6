"""Shared by the robust joint-registration tests (tests/ only): numpy restatements of Landmarks.eval_register_robust /
register_robust on top of tests/landmark_register_reference.py (imported, not edited), the cases the CPU qualification and the
GPU tests walk, and the g++-built harness around csrc/sba_landmarks_register_robust.hpp.

The objective: the Huber loss on every landmark's block of the joint registration's F, F_rho = sum_j rho(min_X f_j(X, pose)) =
sum_j rho(chi2_j) with chi2_j = r^T M r of landmark_register_reference; rho(s) = s for s <= delta^2, else 2 delta sqrt(s) -
delta^2; w = rho'(s).  Per evaluation H = sum w F^T M F, g = sum w F^T M r (the exact gradient of 1/2 F_rho), cost = 1/2 sum rho,
n_outlier = the used observations with chi2 > delta^2.  At the solution Sigma_c = H^-1 and the posterior of
landmark_register_reference with that Sigma_c; the gate must not exceed delta^2, so every fused observation had weight 1.

The REFERENCE is the basis-free form in numpy long double with a Levenberg-Marquardt loop of its own run to a step below 1e-13;
the BASIS FORM (float64, basis=True) is the product's formulation in numpy's own order: its error against the reference is what
float64 can do, and 8 times that is what the host code and the device are held to."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import landmark_register_reference as lr
import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr

LD = lr.LD
SKIPPED, BEHIND, GATED, FUSED = lr.SKIPPED, lr.BEHIND, lr.GATED, lr.FUSED
DELTA = 2.0                          # Huber delta of every case, in units of the whitened residual
GATE = DELTA * DELTA                 # the largest gate the entry points accept
BIG_DELTA = 1e6                      # above every sqrt(chi2) of every case: nothing is an outlier
DISPLACE = 0.2                       # rad: a wrong match
MARGIN = 1e-9
BEARING_SIGMAS = lr.BEARING_SIGMAS
SIZES, LONG = lr.SIZES, lr.LONG
POSE_NAMES = ("zero", "closed", "near_pi")   # of tests/pose_edges.py: identity (the small-angle branch), one generic, one near pi
assert all(k in pose_edges.POSES for k in POSE_NAMES)
SOLVE_SIZES, SOLVE_LONG = (65, 513), (1537,)
DEMO_N = 513


def displace(y, rows, seed, angle=DISPLACE):
    """y with the rows `rows` turned by `angle` about seeded axes across them; lengths kept."""
    y = np.array(y, dtype=np.float64)
    rows = np.asarray(rows, dtype=int)
    if len(rows) == 0:
        return y
    rng = np.random.default_rng(seed)
    v = y[rows]
    k = np.cross(v, rng.standard_normal(v.shape))
    k /= np.linalg.norm(k, axis=1, keepdims=True)
    y[rows] = v * np.cos(angle) + np.cross(k, v) * np.sin(angle)
    return y


def planted(n, every):
    """Every `every`-th row: the wrong matches of a scene of n observations."""
    return np.arange(every // 2, n, every, dtype=int)


# ---- the loss ----------------------------------------------------------------------------------------------------------------
def huber(s, delta, dtype=LD):
    """-> w, rho, out of chi2 values s."""
    s = np.asarray(s, dtype=dtype)
    d = dtype(delta)
    out = s > d * d
    root = np.sqrt(np.where(out, s, dtype(1)))
    return np.where(out, d / root, dtype(1)), np.where(out, 2 * d * root - d * d, s), out


# ---- one evaluation ------------------------------------------------------------------------------------------------------------
@dataclass
class Equations(lr.Equations):
    n_outlier: int = 0


def _parts(Xs, Cs, ys, noise2, rot, tran, dtype, basis):
    """Per observation that takes part: the point, Sigma R^T M, Xh, F = [A(Xh) | I] and chi2."""
    pt = lr.point(Xs, Cs, ys, noise2, rot, tran, dtype, basis)
    with np.errstate(all="ignore"):
        GM = pt.Sg @ pt.R.T[None] @ pt.M
        Xh = np.asarray(Xs, dtype=dtype) + np.einsum("iab,ib->ia", GM, pt.r)
        F = lr._jacobian(pt, Xh, rot, dtype)
        if basis is True:
            u = np.einsum("ika,ia->ik", pt.W, pt.r)
            s = np.sum(u * u, axis=1)
        else:
            s = np.einsum("ia,iab,ib->i", pt.r, pt.M, pt.r)
    return pt, GM, Xh, F, s


def chi2_at(X, cov6, y, noise, rot, tran, dtype=LD, basis=False):
    """chi2 of every observation that takes part (NaN elsewhere), and the mask of those the sums use."""
    live = lr.live_of(noise)
    s_all, used = np.full(len(X), np.nan, dtype=dtype), np.zeros(len(X), dtype=bool)
    if live.any():
        Xs, Cs, ys = (np.asarray(a, dtype=np.float64)[live] for a in (X, np.asarray(cov6).reshape(-1, 6), y))
        pt, _, _, _, s = _parts(Xs, Cs, ys, np.asarray(noise, dtype=dtype)[live], rot, tran, dtype, basis)
        s_all[live], used[live] = s, ~pt.bad
    return s_all, used


def evaluate(X, cov6, y, noise, rot, tran, delta, dtype=LD, basis=False, raw=False):
    """The robust reduce pass's sums at (rot, tran) over the observations that take part."""
    live = lr.live_of(noise)
    if not live.any():
        return Equations(np.zeros((6, 6)), np.zeros(6), 0.0, 0, 0, 0)
    Xs, Cs, ys = (np.asarray(a, dtype=np.float64)[live] for a in (X, np.asarray(cov6).reshape(-1, 6), y))
    pt, _, _, F, s = _parts(Xs, Cs, ys, np.asarray(noise, dtype=dtype)[live], rot, tran, dtype, basis)
    used = ~pt.bad
    w, rho, out = huber(s, delta, dtype)
    w, rho, out = np.where(used, w, dtype(0)), np.where(used, rho, dtype(0)), out & used
    with np.errstate(all="ignore"):
        if basis is True:
            Jw = pt.W @ F
            u = np.einsum("ika,ia->ik", pt.W, pt.r)
            H, g = np.einsum("i,ika,ikb->ab", w, Jw, Jw), np.einsum("i,ika,ik->a", w, Jw, u)
        else:
            MF = pt.M @ F
            H, g = np.einsum("i,ika,ikb->ab", w, F, MF), np.einsum("i,ika,ik->a", w, MF, pt.r)
    res = (H, g) if raw else (H.astype(np.float64), g.astype(np.float64))
    cost = 0.5 * rho.sum()
    return Equations(res[0], res[1], cost if raw else float(cost), int(used.sum()), int((used & (pt.dstar <= 0)).sum()), int(out.sum()))


def half_objective(X, cov6, y, noise, p, delta):
    """1/2 F_rho at p = [rot | tran] in long double: what g is the gradient of."""
    return evaluate(X, cov6, y, noise, p[:3], p[3:], delta, raw=True).cost


def chi2_margin(s, used, bound):
    """The smallest relative distance of a used chi2 from `bound`."""
    v = np.asarray(s, dtype=LD)[used]
    return float(np.abs(v / LD(bound) - 1).min()) if len(v) else np.inf


# ---- the solve: landmark_register_reference's loop over the robust sums -----------------------------------------------------
def solve(X, cov6, y, noise, rot, tran, delta, dtype=LD, max_iterations=200, step_tol=1e-13, basis=False):
    """-> rot, tran (float64), the Equations there, iterations: damping lam diag(H), accepted steps divide lam by 3, rejected ones
    multiply it by 4, until an accepted step is below step_tol; then undamped steps while they shrink the (exact) gradient."""
    ev = lambda q: evaluate(X, cov6, y, noise, q[:3], q[3:], delta, dtype, basis, raw=True)
    p = np.concatenate([np.asarray(rot, dtype=np.float64), np.asarray(tran, dtype=np.float64)]).astype(dtype)
    e = ev(p)
    lam, it = dtype(1e-4), 0
    for it in range(1, max_iterations + 1):
        d = -(wr.inverse_ld(e.H + lam * np.diag(np.diag(e.H))) @ e.g)
        e2 = ev(p + d)
        if e2.cost <= e.cost:
            p, e, lam = p + d, e2, lam / 3
            if np.abs(d).max() < step_tol:
                break
        else:
            lam = lam * 4
            if lam > 1e12:
                break
    for _ in range(20):
        d = -(wr.inverse_ld(e.H) @ e.g)
        if np.abs(d).max() < step_tol:
            break
        e2 = ev(p + d)
        if not np.abs(e2.g).max() < np.abs(e.g).max():
            break
        p, e = p + d, e2
    p64 = p.astype(np.float64)
    return p64[:3], p64[3:], evaluate(X, cov6, y, noise, p64[:3], p64[3:], delta, dtype, basis), it


# ---- the posterior at a pose -----------------------------------------------------------------------------------------------------
def posterior(X, cov6, y, noise, rot, tran, delta, gate=GATE, dtype=LD, basis=False):
    """The write-back at (rot, tran): Sigma_c = H_rho^-1 from the robust sums there, then landmark_register_reference's posterior
    per observation with that Sigma_c."""
    assert gate <= delta * delta
    m = len(X)
    X0, C0 = np.asarray(X, dtype=dtype), np.asarray(cov6, dtype=dtype).reshape(-1, 6)
    eq = evaluate(X, cov6, y, noise, rot, tran, delta, dtype, basis, raw=True)
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
        pt, GM, Xh, F, s = _parts(Xs, Cs, ys, np.abs(nz), rot, tran, dtype, basis)
        with np.errstate(all="ignore"):
            if basis is True:
                T = pt.Sg @ pt.R.T[None] @ np.swapaxes(pt.W, 1, 2)
                cond = pt.Sg - T @ np.swapaxes(T, 1, 2)
                G = T @ (pt.W @ F)
            else:
                cond = pt.Sg - GM @ np.swapaxes(pt.Sg @ pt.R.T[None], 1, 2)
                G = GM @ F
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
    out_eq = Equations(eq.H.astype(np.float64), eq.g.astype(np.float64), eq.cost, eq.n_used, eq.n_behind, eq.n_outlier)
    return lr.Registered(Xo, Co, chi2, cls, dstar_all, Sc, cross, out_eq)


# ---- the evaluation cases: landmark_register_reference's scenes with about one bearing in eight displaced --------------------
@lru_cache(maxsize=None)
def scene(n, pose_name):
    s = lr.scene(n, pose_name)
    y = displace(s.y, planted(n, 8), 8800 + n)
    y.setflags(write=False)
    return lr.Scene(s.name, s.X, s.cov, y, s.rot, s.tran, s.rot_ref, s.tran_ref, s.truth_X, s.grid_one)


def scenes(sizes=SIZES + LONG):
    return [scene(n, name) for n in sizes for name in POSE_NAMES]


@lru_cache(maxsize=None)
def eval_reference(n, pose_name, bs, indexed, delta=DELTA):
    """Long double: (noise, freeze classes, Equations, chi2, used) of a scene's dense or indexed evaluation."""
    s = scene(n, pose_name)
    X, cov, y = lr._rows(s, lr.subset(n) if indexed else None)
    noise, cls = lr.freeze(X, cov, y, s.rot_ref, s.tran_ref, bs)
    chi2, used = chi2_at(X, cov, y, noise, s.rot, s.tran)
    return noise, cls, evaluate(X, cov, y, noise, s.rot, s.tran, delta), chi2, used


def qualify_eval(s, bs, indexed, delta=DELTA):
    """float64 numpy in the product's formulation counts as long double does and no chi2 lies within MARGIN of delta^2 -> its (H,
    g, cost) errors against long double."""
    n = len(s.X)
    pose_name = s.name.split()[1]
    X, cov, y = lr._rows(s, lr.subset(n) if indexed else None)
    noise, cls, ref, chi2, used = eval_reference(n, pose_name, bs, indexed, delta)
    assert chi2_margin(chi2, used, delta * delta) > MARGIN, s.name
    nb, cb = lr.freeze(X, cov, y, s.rot_ref, s.tran_ref, bs, np.float64, basis=True)
    assert np.array_equal(cls, cb), s.name
    got = evaluate(X, cov, y, nb, s.rot, s.tran, delta, np.float64, basis=True)
    assert (got.n_used, got.n_behind, got.n_outlier) == (ref.n_used, ref.n_behind, ref.n_outlier), s.name
    if ref.n_used == 0:
        return 0.0, 0.0, 0.0
    return lr.eq_errors(got, ref)


@lru_cache(maxsize=None)
def measured_eval_errors(sizes=SIZES + LONG):
    """float64 numpy's worst (H, g, cost) errors against long double over every evaluation of these sizes, DELTA and BIG_DELTA."""
    worst = np.zeros(3)
    for s in scenes(sizes):
        for bs in BEARING_SIGMAS:
            for indexed in (False, True):
                worst = np.maximum(worst, qualify_eval(s, bs, indexed))
        worst = np.maximum(worst, qualify_eval(s, BEARING_SIGMAS[1], False, BIG_DELTA))
    return tuple(float(v) for v in worst)


# ---- the solve scenes: section 3.20's recipe with one bearing in ten a wrong match -----------------------------------------
@lru_cache(maxsize=None)
def solve_scene(n, seed=None, bearing_noise=1e-3, every=10):
    seed = 17000 + n if seed is None else seed
    ns = wr.noisy_scene(n, seed, bearing_noise)
    r0, t0 = rr.start_near(ns.scene, seed, lr.START_ROT, lr.START_TRAN)
    y = displace(ns.y, planted(n, every), seed + 4242)
    y.setflags(write=False)
    return lr.SolveScene(f"n={n} seed={seed}", ns.X, ns.cov, y, r0, t0, ns.scene, bearing_noise, n in SOLVE_LONG)


@lru_cache(maxsize=None)
def solve_reference(n, seed=None):
    """Long double: the noise frozen at the start, the robust minimiser, the Equations there."""
    s = solve_scene(n, seed)
    noise, cls = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
    rot, tran, eq, it = solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0, DELTA)
    return noise, cls, rot, tran, eq, it


@lru_cache(maxsize=None)
def plain_reference(n, seed=None):
    """Long double: landmark_register_reference's minimiser (no loss) of the same scene, wrong matches included."""
    s = solve_scene(n, seed)
    noise, cls = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
    rot, tran, eq, it = lr.solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0)
    return noise, cls, rot, tran, eq, it


def pose_distance2(rot, tran, s, H):
    """(p - truth)^T H (p - truth) of a solve scene."""
    d = np.concatenate([np.asarray(rot, dtype=LD) - s.truth.rot, np.asarray(tran, dtype=LD) - s.truth.tran])
    return float(d @ np.asarray(H, dtype=LD) @ d)


def qualify_posterior(X, cov, y, rot_ref, tran_ref, rot, tran, bs, delta=DELTA, gate=GATE, form=False):
    """The posterior at (rot, tran): float64 in the product's formulation classifies as long double does, no chi2 within MARGIN
    of the gate or of delta^2, no d* within MARGIN of 0 -> (ref, float64's (X+, Sigma+, chi2, Sigma_c) errors)."""
    noise, cls = lr.freeze(X, cov, y, rot_ref, tran_ref, bs, basis=form)
    ref = posterior(X, cov, y, noise, rot, tran, delta, gate, basis=form)
    nb, cb = lr.freeze(X, cov, y, rot_ref, tran_ref, bs, np.float64, basis=True)
    b = posterior(X, cov, y, nb, rot, tran, delta, gate, np.float64, basis=True)
    assert np.array_equal(cls, cb) and np.array_equal(ref.cls, b.cls)
    live = ref.cls != SKIPPED
    assert (np.abs(ref.chi2[live] - gate) > MARGIN * gate).all()
    assert (np.abs(ref.chi2[live] - delta * delta) > MARGIN * delta * delta).all()
    assert (np.abs(ref.dstar[live]) > MARGIN).all()
    return ref, lr.post_errors(b.X, b.cov, b.chi2, b.pose_cov, ref, X, cov)


# ---- the product's host side through the g++-built harness (tests/harness/landmark_register_robust_harness.cpp) ------------------
_h = None


def harness():
    """csrc/sba_landmarks_register_robust.hpp compiled for the CPU."""
    global _h
    if _h is None:
        import ctypes as C
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "liblandmark_register_robust_harness.so"
        src = root / "tests" / "harness" / "landmark_register_robust_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f
                for f in ("sba_landmarks_register_robust.hpp", "sba_landmarks_register.hpp", "sba_landmarks.hpp", "sba_resection_weighted.hpp",
                          "sba_resection.hpp", "sba_rotation.hpp", "sba_epipolar.hpp")]
        hdrs.append(root / "include" / "sba_hip.h")
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        dp = C.POINTER(C.c_double)
        _h.landmark_register_robust_harness_eval.argtypes = [C.c_longlong, dp, dp, dp, dp, dp, dp, C.c_double, dp]
        _h.landmark_register_robust_harness_check.argtypes = [C.c_double, C.c_double]
    return _h


def harness_eval(X, cov6, y, noise, rot, tran, delta):
    """landmark_register_accumulate_robust over the rows into one set of sums, expanded by resect_expand_row -> Equations."""
    X, cov6, y, noise, rot, tran = (lr._a(v) for v in (X, cov6, y, noise, rot, tran))
    out = np.zeros(46)
    harness().landmark_register_robust_harness_eval(len(X), rr._dp(X), rr._dp(cov6), rr._dp(y), rr._dp(noise), rr._dp(rot), rr._dp(tran),
                                                    float(delta), rr._dp(out))
    return Equations(out[:36].reshape(6, 6).copy(), out[36:42].copy(), float(out[42]), int(out[43]), int(out[44]), int(out[45]))


def harness_check(huber_delta, chi2_gate):
    """1 when landmark_register_check_robust accepts."""
    return int(harness().landmark_register_robust_harness_check(float(huber_delta), float(chi2_gate)))
