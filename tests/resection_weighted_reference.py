"""Shared by the weighted-resection tests (tests/ only): numpy restatements of the resection weighted by landmark covariances,
seeded covariances for the scenes of tests/resection_reference.py, and the list of cases both the CPU qualification and the
GPU tests walk.

    S_i = cov_scale R(w_ref) Sigma_i R(w_ref)^T + bearing_sigma^2 d_i*(ref)^2 (y . y) I          frozen at a reference pose
    M_i = S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y),   s_i = r_i^T M_i r_i,   cost = 1/2 sum rho(s_i)
    H = sum w_i [A | I]^T M_i [A | I],   g = sum w_i [A | I]^T M_i r_i

The REFERENCE (info_matrices, sums) is the closed form above in numpy long double per match, its 3 x 3 inverse by the adjugate:
no basis of the plane across the bearing appears in it.  The BASIS FORM (basis_factor, basis_sums) is float64 numpy in the
product's formulation -- b1 = e_k x y, b2 = y x b1, the Cholesky factor of B^T S B, z = G^-1 B^T r -- in numpy's own summation
order: the proof that the GPU tests' tolerance can be met in float64 at all."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import pose_edges
import resection_reference as rr

LD = np.longdouble
COV_SCALE = 1.3
DELTA = 2.0                       # Huber delta of the cases with planted outliers, sigma units
BEARING_SIGMAS = (0.0, 1e-3)
SIZES_F64 = (0, 1, 2, 3, 63, 64, 65, 511, 512, 513)
SIZES_F32 = SIZES_F64 + (1023, 1024, 1025)
LONG = (1537, 3073)               # SBA_RESECT_GRID=1: three grid-stride steps and a ragged tail (f64: 1537 / 512, f32: 3073 / 1024)
MARGIN = 1e-9                     # no s_i within MARGIN * delta^2 of delta^2: outlier counts may be demanded equal
EDGE_AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
# the solve tests: (n, seed) of noisy_scene, started 0.01 off the truth, delta = DELTA, bearing noise and bearing_sigma 1e-3
SOLVE_SCENES = ((65, 4100), (513, 4101))
SOLVE_BEARING_SIGMA = 1e-3


# ---- seeded covariances -----------------------------------------------------------------------------------------------------
def landmark_sigmas(X, seed, max_aniso=100.0):
    """Per landmark (sigma_t, sigma_r): sigma_t = 0.002 |X| U(0.5, 2) across the viewing ray x^ = X / |X|, sigma_r / sigma_t
    log-uniform in [3, max_aniso] along it."""
    rng = np.random.default_rng(seed + 9001)
    n = len(X)
    st = 0.002 * np.linalg.norm(X, axis=1) * rng.uniform(0.5, 2.0, size=n)
    sr = st * np.exp(rng.uniform(np.log(3.0), np.log(max_aniso), size=n))
    return st, sr


def landmark_cov(X, seed, max_aniso=100.0):
    """(n, 6) rows (xx, yy, zz, xy, xz, yz) of Sigma_i = sigma_r^2 x^ x^^T + sigma_t^2 (I - x^ x^^T), and their square roots
    (n, 3, 3) for drawing noise."""
    X = np.asarray(X, dtype=np.float64)
    n = len(X)
    if n == 0:
        return np.zeros((0, 6)), np.zeros((0, 3, 3))
    st, sr = landmark_sigmas(X, seed, max_aniso)
    u = X / np.linalg.norm(X, axis=1, keepdims=True)
    uu = u[:, :, None] * u[:, None, :]
    eye = np.eye(3)[None]
    S = sr[:, None, None] ** 2 * uu + st[:, None, None] ** 2 * (eye - uu)
    root = sr[:, None, None] * uu + st[:, None, None] * (eye - uu)
    rows = np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]], axis=1)
    return np.ascontiguousarray(rows), root


def full(rows, dtype=LD):
    """(n, 6) rows -> (n, 3, 3) symmetric matrices."""
    r = np.asarray(rows, dtype=dtype).reshape(-1, 6)
    S = np.zeros((len(r), 3, 3), dtype=dtype)
    S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = r[:, 0], r[:, 1], r[:, 2]
    S[:, 0, 1] = S[:, 1, 0] = r[:, 3]
    S[:, 0, 2] = S[:, 2, 0] = r[:, 4]
    S[:, 1, 2] = S[:, 2, 1] = r[:, 5]
    return S


def rows_of(M):
    return np.stack([M[:, 0, 0], M[:, 1, 1], M[:, 2, 2], M[:, 0, 1], M[:, 0, 2], M[:, 1, 2]], axis=1)


# ---- the reference: closed form, long double ---------------------------------------------------------------------------------
def _adjugate_inverse(S):
    """(n, 3, 3) symmetric -> inverse by the adjugate, and the determinant."""
    a, b, c = S[:, 0, 0], S[:, 0, 1], S[:, 0, 2]
    d, e, f = S[:, 1, 1], S[:, 1, 2], S[:, 2, 2]
    A = np.empty_like(S)
    A[:, 0, 0] = d * f - e * e
    A[:, 0, 1] = A[:, 1, 0] = c * e - b * f
    A[:, 0, 2] = A[:, 2, 0] = b * e - c * d
    A[:, 1, 1] = a * f - c * c
    A[:, 1, 2] = A[:, 2, 1] = b * c - a * e
    A[:, 2, 2] = a * d - b * b
    det = a * A[:, 0, 0] + b * A[:, 0, 1] + c * A[:, 0, 2]
    return A / det[:, None, None], det


def across(S, y, dtype=LD):
    """A unit pair q1, q2 across y and the entries of Q^T S Q.  q1 = e_k x y with k the first smallest |y_k|: the k of the product's
    resect_weight_basis, restated here and normalised."""
    k = np.argmin(np.abs(y), axis=1)
    q1 = np.cross(np.eye(3, dtype=dtype)[k], y)
    q1 = q1 / np.sqrt(np.sum(q1 * q1, axis=1))[:, None]
    q2 = np.cross(y, q1)
    q2 = q2 / np.sqrt(np.sum(q2 * q2, axis=1))[:, None]
    c11 = np.einsum("ia,iab,ib->i", q1, S, q1)
    c12 = np.einsum("ia,iab,ib->i", q1, S, q2)
    c22 = np.einsum("ia,iab,ib->i", q2, S, q2)
    return q1, q2, c11, c12, c22


def projected_weight(S, y, dtype=LD):
    """M = Q (Q^T S Q)^-1 Q^T of rows whose S is positive definite across y, through the Cholesky factor of the 2 x 2 block: no
    S^-1, so S itself may be singular (a prior of rank <= 2 with no bearing noise).  Equal to S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y)
    wherever that exists."""
    q1, q2, c11, c12, c22 = across(S, y, dtype)
    g11 = np.sqrt(c11)
    g21 = c12 / g11
    g22 = np.sqrt(c22 - g21 * g21)
    w1 = q1 / g11[:, None]
    w2 = (q2 - (g21 / g11)[:, None] * q1) / g22[:, None]
    return w1[:, :, None] * w1[:, None, :] + w2[:, :, None] * w2[:, None, :]


def frozen_cov(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, dtype=LD):
    """S_i (n, 3, 3) at the reference pose, and d_i* there."""
    X, y = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype)
    R = rr.rotmat(rot_w, dtype)
    c, dstar, _, _, _ = rr.per_match(X, y, rot_w, tran_w, dtype)
    yy = np.sum(y * y, axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        S = dtype(cov_scale) * (R[None] @ full(cov6, dtype) @ R.T[None])
        S = S + (dtype(bearing_sigma) ** 2 * dstar * dstar * yy)[:, None, None] * np.eye(3, dtype=dtype)[None]
    return S, dstar


def info_matrices(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, dtype=LD):
    """-> M (n, 3, 3) by the closed form, zero (n,) bool: the matches of zero weight (non-finite Sigma row, non-finite d* at the
    reference, S not positive definite across the bearing -- decided on an orthonormal basis of the plane)."""
    n = len(X)
    if n == 0:
        return np.zeros((0, 3, 3), dtype=dtype), np.zeros(0, dtype=bool)
    y = np.asarray(y, dtype=dtype)
    S, dstar = frozen_cov(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, dtype)
    zero = ~np.isfinite(np.asarray(cov6, dtype=np.float64).reshape(-1, 6)).all(axis=1) | ~np.isfinite(dstar.astype(np.float64))
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        # positive definite across the bearing: both leading minors of Q^T S Q, Q orthonormal with columns in y-perp
        k = np.argmin(np.abs(y), axis=1)
        e = np.eye(3, dtype=dtype)[k]
        q1 = np.cross(e, y)
        q1 = q1 / np.sqrt(np.sum(q1 * q1, axis=1))[:, None]
        q2 = np.cross(y, q1)
        q2 = q2 / np.sqrt(np.sum(q2 * q2, axis=1))[:, None]
        c11 = np.einsum("ia,iab,ib->i", q1, S, q1)
        c12 = np.einsum("ia,iab,ib->i", q1, S, q2)
        c22 = np.einsum("ia,iab,ib->i", q2, S, q2)
        zero |= ~((c11 > 0) & (c11 * c22 - c12 * c12 > 0))
        Ssafe = np.where(zero[:, None, None], np.eye(3, dtype=dtype)[None], S)
        Si, _ = _adjugate_inverse(Ssafe)
        v = np.einsum("iab,ib->ia", Si, y)
        M = Si - v[:, :, None] * v[:, None, :] / np.sum(v * y, axis=1)[:, None, None]
    M = np.where(zero[:, None, None], dtype(0), M)
    return M, zero


@dataclass
class WeightedSums(rr.Sums):
    n_zero_weight: int = 0
    s: np.ndarray = None         # (n,) the per-match chi^2 (0 for a match of zero weight)


def sums(X, y, M, zero, rot, tran, delta, dtype=LD):
    """The weighted reduce pass's sums with M as given, per match in `dtype`."""
    n = len(X)
    if n == 0:
        return WeightedSums(np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, 0.0, 0.0, 0, np.zeros(0))
    Xs = np.where(zero[:, None], 0.0, np.asarray(X, dtype=np.float64))         # a match of zero weight adds nothing, whatever it holds
    ys = np.where(zero[:, None], np.array([1.0, 0.0, 0.0])[None], np.asarray(y, dtype=np.float64))
    M = np.asarray(M, dtype=dtype)
    c, dstar, r, _, A = rr.per_match(Xs, ys, rot, tran, dtype)
    F = np.concatenate([A, np.broadcast_to(np.eye(3, dtype=dtype), (n, 3, 3))], axis=2)
    s = np.einsum("ia,iab,ib->i", r, M, r)
    out = (s > dtype(delta) * dtype(delta)) if delta > 0 else np.zeros(n, dtype=bool)
    root = np.sqrt(np.where(out, s, dtype(1)))
    live = ~zero
    w = np.where(out, dtype(delta) / root, dtype(1)) * live
    rho = np.where(out, 2 * dtype(delta) * root - dtype(delta) ** 2, s) * live
    MF = M @ F
    H = np.einsum("i,ika,ikb->ab", w, F, MF)
    g = np.einsum("i,ika,ik->a", w, MF, r)
    return WeightedSums(H.astype(np.float64), g.astype(np.float64), float(0.5 * rho.sum()), float(w.sum()), float((out & live).sum()),
                        float(((dstar <= 0) & live).sum()), int(zero.sum()), (s * live).astype(np.float64))


# ---- the basis form: float64, the product's formulation -----------------------------------------------------------------------
def basis(y):
    """b1 = e_k x y, b2 = y x b1, k = the index of the smallest |y_k| (the lowest on ties)."""
    y = np.asarray(y)
    k = np.argmin(np.abs(y), axis=1)            # argmin returns the first minimum
    e = np.eye(3, dtype=y.dtype)[k]
    b1 = np.cross(e, y)
    return b1, np.cross(y, b1)


def basis_factor(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, dtype=np.float64):
    """-> W (n, 2, 3) = G^-1 B^T (zeros for a match of zero weight), q (n, 3) the stored factor, zero (n,) bool."""
    n = len(X)
    if n == 0:
        return np.zeros((0, 2, 3), dtype=dtype), np.zeros((0, 3), dtype=dtype), np.zeros(0, dtype=bool)
    y = np.asarray(y, dtype=dtype)
    S, dstar = frozen_cov(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, dtype)
    b1, b2 = basis(y)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        c11 = np.einsum("ia,iab,ib->i", b1, S, b1)
        c12 = np.einsum("ia,iab,ib->i", b1, S, b2)
        c22 = np.einsum("ia,iab,ib->i", b2, S, b2)
        g11 = np.sqrt(c11)
        g21 = c12 / g11
        d = c22 - g21 * g21
        g22 = np.sqrt(d)
        q = np.stack([1 / g11, -g21 / (g11 * g22), 1 / g22], axis=1)
        ok = (c11 > 0) & (d > 0) & np.isfinite(q).all(axis=1) & (q[:, 0] > 0) & (q[:, 2] > 0)
    ok &= np.isfinite(np.asarray(cov6, dtype=np.float64).reshape(-1, 6)).all(axis=1) & np.isfinite(dstar.astype(np.float64))
    q = np.where(ok[:, None], q, dtype(0))
    W = np.stack([q[:, 0:1] * b1, q[:, 1:2] * b1 + q[:, 2:3] * b2], axis=1)
    return W, q, ~ok


def basis_rows(W):
    """(n, 6): M = W^T W as rows."""
    return rows_of(np.einsum("ika,ikb->iab", W, W))


def basis_sums(X, y, W, zero, rot, tran, delta, dtype=np.float64):
    """The sums through z = W r and J_z = [W A | W]."""
    n = len(X)
    if n == 0:
        return WeightedSums(np.zeros((6, 6)), np.zeros(6), 0.0, 0.0, 0.0, 0.0, 0, np.zeros(0))
    Xs = np.where(zero[:, None], 0.0, np.asarray(X, dtype=np.float64))
    ys = np.where(zero[:, None], np.array([1.0, 0.0, 0.0])[None], np.asarray(y, dtype=np.float64))
    c, dstar, r, _, A = rr.per_match(Xs, ys, rot, tran, dtype)
    z = np.einsum("ika,ia->ik", W, r)
    Jz = np.concatenate([W @ A, W], axis=2)
    s = np.sum(z * z, axis=1)
    out = (s > dtype(delta) * dtype(delta)) if delta > 0 else np.zeros(n, dtype=bool)
    root = np.sqrt(np.where(out, s, dtype(1)))
    live = ~zero
    w = np.where(out, dtype(delta) / root, dtype(1)) * live
    rho = np.where(out, 2 * dtype(delta) * root - dtype(delta) ** 2, s) * live
    H = np.einsum("i,ika,ikb->ab", w, Jz, Jz)
    g = np.einsum("i,ika,ik->a", w, Jz, z)
    return WeightedSums(H.astype(np.float64), g.astype(np.float64), float(0.5 * rho.sum()), float(w.sum()), float((out & live).sum()),
                        float(((dstar <= 0) & live).sum()), int(zero.sum()), (s * live).astype(np.float64))


def weighted_evaluator(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, delta, dtype=np.float64):
    """The evaluator callback of rr.harness_solve with the weights frozen at (rot_w, tran_w), in the basis form."""
    W, _, zero = basis_factor(X, y, cov6, rot_w, tran_w, cov_scale, bearing_sigma, dtype)
    return lambda r, t: rr.pack_from_sums(basis_sums(X, y, W, zero, r, t, delta, dtype))


def solve_rounds(X, y, cov6, rot, tran, cov_scale, bearing_sigma, delta, rounds, **opt):
    """What sba_problem_solve_resection_weighted does, through the g++-built LM: per round freeze at the current pose, solve.
    -> rot, tran, the last round's summary, rc."""
    r, t, sm, rc = np.array(rot, dtype=np.float64), np.array(tran, dtype=np.float64), None, 0
    for _ in range(rounds):
        r, t, sm, rc = rr.harness_solve(r, t, weighted_evaluator(X, y, cov6, r, t, cov_scale, bearing_sigma, delta), **opt)
        if rc != 0:
            break
    return r, t, sm, rc


# ---- the cases the CPU qualification and the GPU tests share ------------------------------------------------------------------
@dataclass(frozen=True)
class Case:
    name: str
    scene: rr.Scene
    cov: np.ndarray            # (n, 6)
    rot_w: np.ndarray          # reference pose
    tran_w: np.ndarray
    rot: np.ndarray            # evaluation pose, != the reference pose
    tran: np.ndarray
    delta: float
    bearing_sigma: float
    grid_one: bool = False     # run with SBA_RESECT_GRID=1


def eval_scene(n, with_outliers):
    return rr.make_scene(n, 700 + n, noise=1e-3, outliers=rr.planted(n) if with_outliers else ())


def _case(name, s, seed, delta, bs, grid_one=False, rot_w=None, rot=None):
    """Reference pose 0.004 from the truth, evaluation pose 0.002 from it on another seeded direction: with sigma_t = 0.002 |X| the
    chi^2 values straddle delta^2 = 4, so both Huber branches are populated beside the planted outliers."""
    rw, tw = rr.start_near(s, seed + 1000, 0.004, 0.004)
    re, te = rr.start_near(s, seed, 0.002, 0.002)
    cov, _ = landmark_cov(s.X, seed)
    return Case(name, s, cov, rw if rot_w is None else rot_w, tw, re if rot is None else rot, te, delta, bs, grid_one)


@lru_cache(maxsize=None)
def eval_cases(f32):
    out = []
    for n in (SIZES_F32 if f32 else SIZES_F64):
        for delta, with_outliers in ((0.0, False), (DELTA, True)):
            for bs in BEARING_SIGMAS:
                out.append(_case(f"n={n} delta={delta} bs={bs}", eval_scene(n, with_outliers), n, delta, bs))
    for n in LONG:
        out.append(_case(f"one block n={n}", eval_scene(n, True), n, DELTA, 1e-3, grid_one=True))
    return tuple(out)


@lru_cache(maxsize=None)
def edge_cases():
    """The nine rotations of tests/pose_edges.py as the reference pose and as the evaluation pose; the truth is 0.2 degrees off."""
    out = []
    for name in pose_edges.NAMES:
        w = pose_edges.POSES[name]
        s = rr.make_scene(129, 62, noise=1e-3, outliers=rr.planted(129), rot=w + np.deg2rad(0.2) * EDGE_AXIS)
        out.append(_case(f"{name} as reference", s, 129, DELTA, 1e-3, rot_w=w))
        out.append(_case(f"{name} as evaluation", s, 129, DELTA, 0.0, rot=w))
    return tuple(out)


def case_planes(c, f32):
    return rr.planes(c.scene, f32)


def case_reference(c, f32, cov_scale=COV_SCALE):
    """The long-double sums of a case on what the planes hold, with M and the zero mask."""
    X, y = case_planes(c, f32)
    M, zero = info_matrices(X, y, c.cov, c.rot_w, c.tran_w, cov_scale, c.bearing_sigma)
    return sums(X, y, M, zero, c.rot, c.tran, c.delta), M, zero


def row_error(got_rows, M):
    """Worst per-match error of (n, 6) rows against the reference M, relative to the largest entry of the match's row."""
    ref = rows_of(M)
    if len(ref) == 0:
        return 0.0
    scale = np.abs(ref).max(axis=1)
    scale = np.where(scale > 0, scale, 1)
    return float((np.abs(np.asarray(got_rows, dtype=LD) - ref).max(axis=1) / scale).max())


# ---- the noisy scenes of the calibration and the solve tests ------------------------------------------------------------------
@dataclass(frozen=True)
class NoisyScene:
    scene: rr.Scene            # the truth
    X: np.ndarray              # landmarks with noise drawn from their covariances
    y: np.ndarray              # bearings with noise
    cov: np.ndarray


@lru_cache(maxsize=None)
def noisy_scene(n, seed, bearing_noise=1e-3):
    s = rr.make_scene(n, seed, noise=bearing_noise)
    cov, root = landmark_cov(s.X, seed)
    rng = np.random.default_rng(seed + 31337)
    X = s.X + np.einsum("iab,ib->ia", root, rng.standard_normal((n, 3)))
    for a in (X, cov):
        a.setflags(write=False)
    return NoisyScene(s, X, s.y, cov)


def inverse_ld(H):
    """The inverse of a small symmetric positive definite matrix in long double (Gauss-Jordan, no pivoting needed)."""
    n = len(H)
    A = np.concatenate([np.asarray(H, dtype=LD), np.eye(n, dtype=LD)], axis=1)
    for k in range(n):
        A[k] = A[k] / A[k, k]
        for i in range(n):
            if i != k:
                A[i] = A[i] - A[i, k] * A[k]
    return A[:, n:]


def gauss_newton(evaluate, rot, tran, steps=12):
    """Plain Gauss-Newton on an evaluator (rot, tran) -> Sums; the calibration needs no trust region this close to the optimum."""
    r, t = np.array(rot, dtype=np.float64), np.array(tran, dtype=np.float64)
    for _ in range(steps):
        e = evaluate(r, t)
        d = -np.linalg.solve(e.H, e.g)
        r, t = r + d[:3], t + d[3:]
        if np.abs(d).max() < 1e-13:
            break
    return r, t, evaluate(r, t)


# ---- the product's host side through the g++-built harness (tests/harness/resection_weighted_harness.cpp) ---------------------
_h = None


def harness():
    """csrc/sba_resection_weighted.hpp compiled for the CPU."""
    global _h
    if _h is None:
        import ctypes as C
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "libresection_weighted_harness.so"
        src = root / "tests" / "harness" / "resection_weighted_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f
                for f in ("sba_resection_weighted.hpp", "sba_resection.hpp", "sba_epipolar.hpp")] + [root / "include" / "sba_hip.h"]
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        _h.resection_weighted_harness_check.argtypes = [C.c_int, C.c_double]
        _h.resection_weighted_harness_rows.argtypes = [C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_longlong, C.POINTER(C.c_double)]
        _h.resection_weighted_harness_finish.argtypes = [C.POINTER(C.c_double), C.c_longlong, C.c_longlong, C.POINTER(C.c_double)]
    return _h


def harness_factor(S6, y):
    """The product's factor of one projected covariance -> (has weight, q (3,))."""
    S6, y, q = np.ascontiguousarray(S6, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64), np.full(3, np.nan)
    ok = harness().resection_weighted_harness_factor(rr._dp(S6), rr._dp(y), rr._dp(q))
    return bool(ok), q


def harness_rows(q, y):
    """The product's expansion of stored factors (n, 3) and bearings (n, 3) to rows of M (n, 6)."""
    q, y = np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    out = np.full((len(q), 6), np.nan)
    harness().resection_weighted_harness_rows(rr._dp(q), rr._dp(y), len(q), rr._dp(out))
    return out
