"""Shared by the Hampel joint-registration tests (tests/ only): numpy restatements of Landmarks.eval_register_hampel /
register_hampel on top of tests/landmark_register_robust_reference.py (imported, not edited), the cases the CPU qualification and
the GPU tests walk, and the g++-built harness around csrc/sba_landmarks_register_hampel.hpp.

The objective is the robust reference's F_rho = sum_j rho(chi2_j) with Hampel's three-part loss in place of Huber's.  With s =
chi2, r = sqrt(s), 0 < a < b < c:
    s <= a^2          w = 1                           rho = s
    a^2 < s <= b^2    w = a / r                       rho = 2 a r - a^2
    b^2 < s <= c^2    w = a (c - r) / ((c - b) r)     rho = 2 a b - a^2 + a (c - b) - a (c - r)^2 / (c - b)
    s > c^2           w = 0                           rho = a (b + c) - a^2
H = sum w F^T M F, g = sum w F^T M r (the exact gradient of 1/2 F_rho), cost = 1/2 sum rho, n_outlier = the used observations with
s > a^2, n_rejected = those with s > c^2.  b = c = inf is Huber: the first two rows are the robust reference's very expressions,
so that case reproduces it to the bit.

The REFERENCE is long double; the BASIS FORM (float64, basis=True) is the product's formulation in numpy's own order, and 8 times
its error against the reference is what the host code and the device are held to.  The solve is STAGED as the product's is: the
robust reference's Huber solve from the start pose, then the Hampel solve from its minimiser on the same frozen noise."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import landmark_register_reference as lr
import landmark_register_robust_reference as rb
import resection_reference as rr
import resection_weighted_reference as wr

LD = rb.LD
SKIPPED, BEHIND, GATED, FUSED = rb.SKIPPED, rb.BEHIND, rb.GATED, rb.FUSED
A, B, C = 2.0, 4.0, 8.0              # the thresholds of every case, in units of the whitened residual
GATE = A * A
INF = float("inf")
DISPLACE, DISPLACE_MID = rb.DISPLACE, 0.02   # rad: a wrong match, and a poor one that lands between the thresholds
MARGIN = rb.MARGIN
BEARING_SIGMAS = rb.BEARING_SIGMAS
SIZES, LONG = rb.SIZES, rb.LONG
POSE_NAMES = rb.POSE_NAMES
SOLVE_SIZES, SOLVE_LONG = rb.SOLVE_SIZES, rb.SOLVE_LONG
DEMO_N = rb.DEMO_N
displace, planted = rb.displace, rb.planted


# ---- the loss ----------------------------------------------------------------------------------------------------------------
def hampel(s, a, b, c, dtype=LD):
    """-> w, rho, out (s > a^2), mid (s > b^2), rej (s > c^2) of chi2 values s.  Rows are chosen by np.where: with b = c = inf the
    third and the fourth row hold inf and NaN and are never chosen."""
    s = np.asarray(s, dtype=dtype)
    d, b, c = dtype(a), dtype(b), dtype(c)
    out, mid, rej = s > d * d, s > b * b, s > c * c
    root = np.sqrt(np.where(out, s, dtype(1)))
    w2, rho2 = d / root, 2 * d * root - d * d                # the robust reference's expressions
    with np.errstate(all="ignore"):
        t = c - root
        w3 = d * t / ((c - b) * root)
        rho3 = 2 * d * b - d * d + d * (c - b) - d * t * t / (c - b)
        rho4 = d * (b + c) - d * d
    w = np.where(rej, dtype(0), np.where(mid, w3, np.where(out, w2, dtype(1))))
    rho = np.where(rej, rho4, np.where(mid, rho3, np.where(out, rho2, s)))
    return w, rho, out, mid, rej


# ---- one evaluation ------------------------------------------------------------------------------------------------------------
@dataclass
class Equations(rb.Equations):
    n_rejected: int = 0


def evaluate(X, cov6, y, noise, rot, tran, a=A, b=B, c=C, dtype=LD, basis=False, raw=False):
    """The Hampel reduce pass's sums at (rot, tran) over the observations that take part: rb.evaluate with the other loss."""
    live = lr.live_of(noise)
    if not live.any():
        return Equations(np.zeros((6, 6)), np.zeros(6), 0.0, 0, 0, 0, 0)
    Xs, Cs, ys = (np.asarray(v, dtype=np.float64)[live] for v in (X, np.asarray(cov6).reshape(-1, 6), y))
    pt, _, _, F, s = rb._parts(Xs, Cs, ys, np.asarray(noise, dtype=dtype)[live], rot, tran, dtype, basis)
    used = ~pt.bad
    w, rho, out, _, rej = hampel(s, a, b, c, dtype)
    w, rho, out, rej = np.where(used, w, dtype(0)), np.where(used, rho, dtype(0)), out & used, rej & used
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
    return Equations(res[0], res[1], cost if raw else float(cost), int(used.sum()), int((used & (pt.dstar <= 0)).sum()), int(out.sum()),
                     int(rej.sum()))


def half_objective(X, cov6, y, noise, p, a=A, b=B, c=C):
    """1/2 F_rho at p = [rot | tran] in long double: what g is the gradient of."""
    return evaluate(X, cov6, y, noise, p[:3], p[3:], a, b, c, raw=True).cost


def branch_counts(s, used, a=A, b=B, c=C):
    """How many used chi2 fall into each of the loss's four rows."""
    v = np.asarray(s, dtype=LD)[used]
    _, _, out, mid, rej = hampel(v, a, b, c)
    return int((~out).sum()), int((out & ~mid).sum()), int((mid & ~rej).sum()), int(rej.sum())


def margins(s, used, a=A, b=B, c=C):
    """The smallest relative distance of a used chi2 from a^2, b^2 and c^2 (the finite ones)."""
    return min(rb.chi2_margin(s, used, t * t) for t in (a, b, c) if np.isfinite(t))


# ---- the solve: Huber first (the robust reference's own solve), then the same loop over the Hampel sums ---------------------------
def solve_direct(X, cov6, y, noise, rot, tran, a=A, b=B, c=C, dtype=LD, max_iterations=200, step_tol=1e-13, basis=False):
    """-> rot, tran (float64), the Equations there, iterations: rb.solve's loop (damping lam diag(H), accepted steps divide lam by 3,
    rejected ones multiply it by 4, until an accepted step is below step_tol; then undamped steps while they shrink the exact
    gradient) over the Hampel sums from (rot, tran)."""
    ev = lambda q: evaluate(X, cov6, y, noise, q[:3], q[3:], a, b, c, dtype, basis, raw=True)
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
    return p64[:3], p64[3:], evaluate(X, cov6, y, noise, p64[:3], p64[3:], a, b, c, dtype, basis), it


def solve(X, cov6, y, noise, rot, tran, a=A, b=B, c=C, dtype=LD, basis=False):
    """The staged solve -> rot, tran, Equations, Hampel iterations, (rot_huber, tran_huber, Huber iterations)."""
    rot_h, tran_h, _, it_h = rb.solve(X, cov6, y, noise, rot, tran, a, dtype, basis=basis)
    rot_s, tran_s, eq, it = solve_direct(X, cov6, y, noise, rot_h, tran_h, a, b, c, dtype, basis=basis)
    return rot_s, tran_s, eq, it, (rot_h, tran_h, it_h)


# ---- the posterior at a pose -----------------------------------------------------------------------------------------------------
def posterior(X, cov6, y, noise, rot, tran, a=A, b=B, c=C, gate=GATE, dtype=LD, basis=False):
    """The write-back at (rot, tran): rb.posterior with Sigma_c = H_rho^-1 from the HAMPEL sums there."""
    assert gate <= a * a
    m = len(X)
    X0, C0 = np.asarray(X, dtype=dtype), np.asarray(cov6, dtype=dtype).reshape(-1, 6)
    eq = evaluate(X, cov6, y, noise, rot, tran, a, b, c, dtype, basis, raw=True)
    Sc = wr.inverse_ld(eq.H).astype(dtype)
    Sc = (Sc + Sc.T) / 2
    marked = np.isnan(np.asarray(noise, dtype=np.float64))
    cls = np.full(m, SKIPPED, dtype=int)
    Xo, Co, chi2 = X0.copy(), C0.copy(), np.full(m, np.nan, dtype=dtype)
    dstar_all, cross = np.full(m, np.nan, dtype=dtype), np.zeros((m, 3, 6), dtype=dtype)
    rows = np.flatnonzero(~marked)
    if len(rows):
        Xs, Cs, ys = (np.asarray(v, dtype=np.float64)[rows] for v in (X, np.asarray(cov6).reshape(-1, 6), y))
        nz = np.asarray(noise, dtype=dtype)[rows]
        pt, GM, Xh, F, s = rb._parts(Xs, Cs, ys, np.abs(nz), rot, tran, dtype, basis)
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
            k = np.where(bad, SKIPPED, np.where(behind, BEHIND, np.where(s > dtype(gate), GATED, FUSED))).astype(int)
        f = k == FUSED
        cls[rows] = k
        Xo[rows] = np.where(f[:, None], Xh, Xo[rows])
        Co[rows] = np.where(f[:, None], Cp, Co[rows])
        chi2[rows] = np.where(k == SKIPPED, dtype(np.nan), s)
        dstar_all[rows] = pt.dstar
        cross[rows] = np.where(f[:, None, None], G @ Sc[None], dtype(0))
    out_eq = Equations(eq.H.astype(np.float64), eq.g.astype(np.float64), eq.cost, eq.n_used, eq.n_behind, eq.n_outlier, eq.n_rejected)
    return lr.Registered(Xo, Co, chi2, cls, dstar_all, Sc, cross, out_eq)


# ---- the evaluation cases: the robust reference's scenes with a second set of rows turned a little ------------------------------
def planted_mid(n):
    """The rows turned by DISPLACE_MID: two behind every wrong match."""
    rows = planted(n, 8) + 2
    return rows[rows < n]


@lru_cache(maxsize=None)
def scene(n, pose_name):
    """lr.scene(n, pose) with planted(n, 8) turned by 0.2 rad (seed 8800 + n: rb.scene's own rows) and planted(n, 8) + 2 by 0.02
    rad (seed 9900 + n)."""
    s = lr.scene(n, pose_name)
    y = displace(s.y, planted(n, 8), 8800 + n)
    y = displace(y, planted_mid(n), 9900 + n, DISPLACE_MID)
    y.setflags(write=False)
    return lr.Scene(s.name, s.X, s.cov, y, s.rot, s.tran, s.rot_ref, s.tran_ref, s.truth_X, s.grid_one)


def scenes(sizes=SIZES + LONG):
    return [scene(n, name) for n in sizes for name in POSE_NAMES]


@lru_cache(maxsize=None)
def eval_reference(n, pose_name, bs, indexed, abc=(A, B, C)):
    """Long double: (noise, freeze classes, Equations, chi2, used) of a scene's dense or indexed evaluation."""
    s = scene(n, pose_name)
    X, cov, y = lr._rows(s, lr.subset(n) if indexed else None)
    noise, cls = lr.freeze(X, cov, y, s.rot_ref, s.tran_ref, bs)
    chi2, used = rb.chi2_at(X, cov, y, noise, s.rot, s.tran)
    return noise, cls, evaluate(X, cov, y, noise, s.rot, s.tran, *abc), chi2, used


def qualify_eval(s, bs, indexed, abc=(A, B, C)):
    """float64 numpy in the product's formulation counts as long double does, no chi2 lies within MARGIN of a threshold, and at n >=
    63 every row of the loss holds a used observation -> its (H, g, cost) errors against long double."""
    n = len(s.X)
    pose_name = s.name.split()[1]
    X, cov, y = lr._rows(s, lr.subset(n) if indexed else None)
    noise, cls, ref, chi2, used = eval_reference(n, pose_name, bs, indexed, abc)
    assert margins(chi2, used, *abc) > MARGIN, s.name
    if n >= 63 and np.isfinite(abc[2]):
        assert min(branch_counts(chi2, used, *abc)) >= 1, (s.name, bs, indexed, branch_counts(chi2, used, *abc))
    nb, cb = lr.freeze(X, cov, y, s.rot_ref, s.tran_ref, bs, np.float64, basis=True)
    assert np.array_equal(cls, cb), s.name
    got = evaluate(X, cov, y, nb, s.rot, s.tran, *abc, dtype=np.float64, basis=True)
    assert (got.n_used, got.n_behind, got.n_outlier, got.n_rejected) == (ref.n_used, ref.n_behind, ref.n_outlier, ref.n_rejected), s.name
    if ref.n_used == 0:
        return 0.0, 0.0, 0.0
    return lr.eq_errors(got, ref)


@lru_cache(maxsize=None)
def measured_eval_errors(sizes=SIZES + LONG):
    """float64 numpy's worst (H, g, cost) errors against long double over every evaluation of these sizes, under (A, B, C) and under
    the Huber limit (A, inf, inf)."""
    worst = np.zeros(3)
    for s in scenes(sizes):
        for bs in BEARING_SIGMAS:
            for indexed in (False, True):
                worst = np.maximum(worst, qualify_eval(s, bs, indexed))
        worst = np.maximum(worst, qualify_eval(s, BEARING_SIGMAS[1], False, (A, INF, INF)))
    return tuple(float(v) for v in worst)


# ---- the solve scenes are the robust reference's: section 3.20's recipe with one bearing in ten a wrong match --------------------
solve_scene = rb.solve_scene
pose_distance2 = rb.pose_distance2


@lru_cache(maxsize=None)
def solve_reference(n, seed=None):
    """Long double: the noise frozen at the start, the staged minimiser, the Equations there, the Hampel iterations, the Huber
    stage."""
    s = solve_scene(n, seed)
    noise, cls = lr.freeze(s.X, s.cov, s.y, s.rot0, s.tran0, s.bearing_sigma)
    rot, tran, eq, it, huber = solve(s.X, s.cov, s.y, noise, s.rot0, s.tran0)
    return noise, cls, rot, tran, eq, it, huber


def qualify_posterior(X, cov, y, rot_ref, tran_ref, rot, tran, bs, abc=(A, B, C), gate=GATE):
    """The posterior at (rot, tran): float64 in the product's formulation classifies as long double does, no chi2 within MARGIN
    of the gate or of a threshold, no d* within MARGIN of 0 -> (ref, float64's (X+, Sigma+, chi2, Sigma_c) errors)."""
    noise, cls = lr.freeze(X, cov, y, rot_ref, tran_ref, bs)
    ref = posterior(X, cov, y, noise, rot, tran, *abc, gate=gate)
    nb, cb = lr.freeze(X, cov, y, rot_ref, tran_ref, bs, np.float64, basis=True)
    b = posterior(X, cov, y, nb, rot, tran, *abc, gate=gate, dtype=np.float64, basis=True)
    assert np.array_equal(cls, cb) and np.array_equal(ref.cls, b.cls)
    live = ref.cls != SKIPPED
    for bound in (gate,) + tuple(t * t for t in abc if np.isfinite(t)):
        assert (np.abs(ref.chi2[live] - bound) > MARGIN * bound).all()
    assert (np.abs(ref.dstar[live]) > MARGIN).all()
    assert (b.eq.n_used, b.eq.n_outlier, b.eq.n_rejected) == (ref.eq.n_used, ref.eq.n_outlier, ref.eq.n_rejected)
    return ref, lr.post_errors(b.X, b.cov, b.chi2, b.pose_cov, ref, X, cov)


# ---- the product's host side through the g++-built harness (tests/harness/landmark_register_hampel_harness.cpp) ------------------
_h = None


def harness():
    """csrc/sba_landmarks_register_hampel.hpp compiled for the CPU."""
    global _h
    if _h is None:
        import ctypes as CT
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "liblandmark_register_hampel_harness.so"
        src = root / "tests" / "harness" / "landmark_register_hampel_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f
                for f in ("sba_landmarks_register_hampel.hpp", "sba_landmarks_register_robust.hpp", "sba_landmarks_register.hpp", "sba_landmarks.hpp",
                          "sba_resection_weighted.hpp", "sba_resection.hpp", "sba_rotation.hpp", "sba_epipolar.hpp")]
        hdrs.append(root / "include" / "sba_hip.h")
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = CT.CDLL(str(so))
        dp = CT.POINTER(CT.c_double)
        _h.landmark_register_hampel_harness_eval.argtypes = [CT.c_longlong, dp, dp, dp, dp, dp, dp, CT.c_double, CT.c_double, CT.c_double, dp]
        _h.landmark_register_hampel_harness_check.argtypes = [CT.c_double, CT.c_double, CT.c_double, CT.c_double]
    return _h


def harness_eval(X, cov6, y, noise, rot, tran, a=A, b=B, c=C):
    """landmark_register_accumulate_hampel over the rows into one set of sums, expanded by resect_expand_row -> Equations."""
    X, cov6, y, noise, rot, tran = (lr._a(v) for v in (X, cov6, y, noise, rot, tran))
    out = np.zeros(47)
    harness().landmark_register_hampel_harness_eval(len(X), rr._dp(X), rr._dp(cov6), rr._dp(y), rr._dp(noise), rr._dp(rot), rr._dp(tran),
                                                    float(a), float(b), float(c), rr._dp(out))
    return Equations(out[:36].reshape(6, 6).copy(), out[36:42].copy(), float(out[42]), int(out[43]), int(out[44]), int(out[45]), int(out[46]))


def harness_check(a, b, c, chi2_gate):
    """1 when landmark_register_check_hampel accepts."""
    return int(harness().landmark_register_hampel_harness_check(float(a), float(b), float(c), float(chi2_gate)))
