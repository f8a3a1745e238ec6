"""Shared by the landmark-map tests (tests/ only): numpy restatements of the fusion of one frame's bearings into landmarks, the
cases the CPU qualification and the GPU tests walk, and the g++-built harness around csrc/sba_landmarks.hpp.

Per observation of a landmark X with covariance Sigma by a bearing y from the pose (w, t) with covariance Sigma_pose:

    c = -R X + t,   d* = -(y . c) / (y . y),   r = c + d* y
    S = R Sigma R^T + bearing_sigma^2 d*^2 (y . y) I + [A | I] Sigma_pose [A | I]^T
    M = S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y)
    Sigma+ = Sigma - Sigma R^T M R Sigma,   X+ = X + Sigma R^T M r,   chi2 = r^T M r

The REFERENCE (fuse) is this basis-free form in numpy long double per observation: M as tests/resection_weighted_reference.py
forms it (the 3 x 3 inverse by the adjugate), the Jacobian [A | I] from tests/resection_reference.py.  The BASIS FORM (fuse_basis)
is float64 numpy in the product's formulation -- b1 = e_k x y, b2 = y x b1, the Cholesky factor of B^T S B, W = G^-1 B^T, u = W r,
T = Sigma R^T W^T, X+ = X + T u, Sigma+ = Sigma - T T^T -- in numpy's own order of operations: its error against the reference is
what float64 can do, and 8 times that is what the device is held to."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import pose_edges
import resection_reference as rr
import resection_weighted_reference as wr

LD = np.longdouble
SKIPPED, BEHIND, GATED, FUSED = 0, 1, 2, 3
COV_SCALE = 1.3
GATE = 9.21                          # chi^2 with 2 degrees of freedom at 0.99
BEARING_SIGMAS = (0.0, 1e-3)
SIZES = (0, 1, 2, 3, 63, 64, 65, 511, 512, 513)
LONG = (1537, 3073)                  # SBA_RESECT_GRID=1: one block takes several steps with a partial last wave
MARGIN = 1e-9
POSE_COV = np.diag(np.array([2e-4, 2e-4, 2e-4, 1e-3, 1e-3, 1e-3]) ** 2)
# a full pose covariance with every block populated: the diagonal one mixed by a fixed rotation of the 6 parameters
_Q, _ = np.linalg.qr(np.random.default_rng(20).standard_normal((6, 6)))
POSE_COV_FULL = _Q @ POSE_COV @ _Q.T
POSE_COV_FULL = np.ascontiguousarray(0.5 * (POSE_COV_FULL + POSE_COV_FULL.T))


@dataclass
class Fused:
    X: np.ndarray          # (m, 3) posterior where cls == FUSED, the prior elsewhere
    cov: np.ndarray        # (m, 6)
    chi2: np.ndarray       # (m,) NaN where skipped
    cls: np.ndarray        # (m,) int
    dstar: np.ndarray      # (m,)

    def counts(self):
        """(n_obs, n_skipped, n_behind, n_gated, n_fused)"""
        return (len(self.cls),) + tuple(int((self.cls == k).sum()) for k in (SKIPPED, BEHIND, GATED, FUSED))


def _empty(dtype):
    return Fused(np.zeros((0, 3), dtype), np.zeros((0, 6), dtype), np.zeros(0, dtype), np.zeros(0, int), np.zeros(0, dtype))


def _prior_cov_S(X, cov6, y, rot, tran, bearing_sigma, pose_cov, dtype):
    """Sigma (n, 3, 3), S (n, 3, 3), R, r, dstar, the mask of non-finite priors."""
    R = rr.rotmat(rot, dtype)
    c, dstar, r, _, A = rr.per_match(X, y, rot, tran, dtype)
    yy = np.sum(y * y, axis=1)
    Sg = wr.full(cov6, dtype)
    S = R[None] @ Sg @ R.T[None] + (dtype(bearing_sigma) ** 2 * dstar * dstar * yy)[:, None, None] * np.eye(3, dtype=dtype)[None]
    if pose_cov is not None:
        F = np.concatenate([A, np.broadcast_to(np.eye(3, dtype=dtype), (len(X), 3, 3))], axis=2)
        S = S + F @ np.asarray(pose_cov, dtype=dtype)[None] @ np.swapaxes(F, 1, 2)
    return Sg, S, R, r, dstar


def _classify(bad, dstar, chi2, gate, Xp, Cp):
    with np.errstate(invalid="ignore"):
        bad = bad | ~np.isfinite(Xp.astype(np.float64)).all(axis=1) | ~np.isfinite(Cp.astype(np.float64)).all(axis=1)
        cls = np.where(bad, SKIPPED, np.where(dstar <= 0, BEHIND, np.where(chi2 > gate, GATED, FUSED)))
    return cls.astype(int)


def fuse(X, cov6, y, rot, tran, bearing_sigma=0.0, gate=np.inf, pose_cov=None, dtype=LD, projected=False):
    """The reference: one bearing per landmark (rows correspond), basis-free, per observation in `dtype`.  projected: M as
    Q (Q^T S Q)^-1 Q^T, which forms no S^-1 and so holds for a singular S (resection_weighted_reference.projected_weight)."""
    n = len(X)
    if n == 0:
        return _empty(dtype)
    X, y, cov6 = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(cov6, dtype=dtype).reshape(-1, 6)
    with np.errstate(all="ignore"):
        Sg, S, R, r, dstar = _prior_cov_S(X, cov6, y, rot, tran, bearing_sigma, pose_cov, dtype)
        bad = ~np.isfinite(X.astype(np.float64)).all(axis=1) | ~np.isfinite(cov6.astype(np.float64)).all(axis=1)
        bad |= ~np.isfinite(dstar.astype(np.float64))
        # positive definite across the bearing: both leading minors of Q^T S Q, Q orthonormal with columns in y-perp
        k = np.argmin(np.abs(y), axis=1)
        q1 = np.cross(np.eye(3, dtype=dtype)[k], y)
        q1 = q1 / np.sqrt(np.sum(q1 * q1, axis=1))[:, None]
        q2 = np.cross(y, q1)
        q2 = q2 / np.sqrt(np.sum(q2 * q2, axis=1))[:, None]
        c11 = np.einsum("ia,iab,ib->i", q1, S, q1)
        c12 = np.einsum("ia,iab,ib->i", q1, S, q2)
        c22 = np.einsum("ia,iab,ib->i", q2, S, q2)
        bad |= ~((c11 > 0) & (c11 * c22 - c12 * c12 > 0))
        Ssafe = np.where(bad[:, None, None], np.eye(3, dtype=dtype)[None], S)
        ysafe = np.where(bad[:, None], np.array([1, 0, 0], dtype=dtype)[None], y)
        if projected:
            M = wr.projected_weight(Ssafe, ysafe, dtype)
        else:
            Si, _ = wr._adjugate_inverse(Ssafe)
            v = np.einsum("iab,ib->ia", Si, ysafe)
            M = Si - v[:, :, None] * v[:, None, :] / np.sum(v * ysafe, axis=1)[:, None, None]
        G = Sg @ R.T[None]                                   # Sigma R^T
        GM = G @ M
        Cp = wr.rows_of(Sg - GM @ np.swapaxes(G, 1, 2))
        Xp = X + np.einsum("iab,ib->ia", GM, r)
        chi2 = np.einsum("ia,iab,ib->i", r, M, r)
        cls = _classify(bad, dstar, chi2, dtype(gate), Xp, Cp)
    fused = cls == FUSED
    return Fused(np.where(fused[:, None], Xp, X), np.where(fused[:, None], Cp, cov6), np.where(cls == SKIPPED, dtype(np.nan), chi2), cls, dstar)


def fuse_basis(X, cov6, y, rot, tran, bearing_sigma=0.0, gate=np.inf, pose_cov=None, dtype=np.float64):
    """The product's formulation in numpy `dtype` (float64: what the device bound is measured from)."""
    n = len(X)
    if n == 0:
        return _empty(dtype)
    X, y, cov6 = np.asarray(X, dtype=dtype), np.asarray(y, dtype=dtype), np.asarray(cov6, dtype=dtype).reshape(-1, 6)
    with np.errstate(all="ignore"):
        Sg, S, R, r, dstar = _prior_cov_S(X, cov6, y, rot, tran, bearing_sigma, pose_cov, dtype)
        bad = ~np.isfinite(X).all(axis=1) | ~np.isfinite(cov6).all(axis=1) | ~np.isfinite(dstar)
        b1, b2 = wr.basis(y)
        c11 = np.einsum("ia,iab,ib->i", b1, S, b1)
        c12 = np.einsum("ia,iab,ib->i", b1, S, b2)
        c22 = np.einsum("ia,iab,ib->i", b2, S, b2)
        g11 = np.sqrt(c11)
        g21 = c12 / g11
        d = c22 - g21 * g21
        g22 = np.sqrt(d)
        q = np.stack([1 / g11, -g21 / (g11 * g22), 1 / g22], axis=1)
        bad |= ~((c11 > 0) & (d > 0) & np.isfinite(q).all(axis=1) & (q[:, 0] > 0) & (q[:, 2] > 0))
        W = np.stack([q[:, 0:1] * b1, q[:, 1:2] * b1 + q[:, 2:3] * b2], axis=1)            # (n, 2, 3)
        u = np.einsum("ika,ia->ik", W, r)
        T = Sg @ R.T[None] @ np.swapaxes(W, 1, 2)                                          # (n, 3, 2)
        Xp = X + np.einsum("iak,ik->ia", T, u)
        Cp = wr.rows_of(Sg - T @ np.swapaxes(T, 1, 2))
        chi2 = np.sum(u * u, axis=1)
        cls = _classify(bad, dstar, chi2, dtype(gate), Xp, Cp)
    fused = cls == FUSED
    return Fused(np.where(fused[:, None], Xp, X), np.where(fused[:, None], Cp, cov6), np.where(cls == SKIPPED, dtype(np.nan), chi2), cls, dstar)


# ---- error measures: the three the GPU test bounds -----------------------------------------------------------------------------
def errors(got_X, got_cov, got_chi2, ref, prior_X, prior_cov):
    """(X+ relative to |X|, Sigma+ relative to the largest entry of the PRIOR Sigma row, chi2 relative to max(chi2, 1)): the worst
    over the observations that are not skipped (X+ and Sigma+ over the fused ones)."""
    if len(ref.cls) == 0:
        return 0.0, 0.0, 0.0
    f, live = ref.cls == FUSED, ref.cls != SKIPPED
    ex = ec = es = 0.0
    if f.any():
        nX = np.sqrt(np.sum(np.asarray(prior_X, dtype=LD)[f] ** 2, axis=1))
        ex = float((np.abs(np.asarray(got_X, dtype=LD)[f] - ref.X[f]).max(axis=1) / nX).max())
        sc = np.maximum(np.abs(np.asarray(prior_cov, dtype=LD)[f]).max(axis=1), LD(1e-300))      # Sigma = 0 stays 0: any error there is huge
        ec = float((np.abs(np.asarray(got_cov, dtype=LD)[f] - ref.cov[f]).max(axis=1) / sc).max())
    if live.any():
        rs = ref.chi2[live]
        es = float((np.abs(np.asarray(got_chi2, dtype=LD)[live] - rs) / np.maximum(rs, 1)).max())
    return ex, ec, es


# ---- the cases the CPU qualification and the GPU tests share ------------------------------------------------------------------
@dataclass(frozen=True)
class Scene:
    name: str
    X: np.ndarray          # (n, 3) prior landmarks
    cov: np.ndarray        # (n, 6) as given to set(); the handle holds COV_SCALE * cov
    y: np.ndarray          # (n, 3) bearings
    rot: np.ndarray        # the pose the frame is fused at
    tran: np.ndarray
    grid_one: bool = False

    @property
    def prior_cov(self):
        return COV_SCALE * self.cov          # the float64 product, as the pack kernel forms it


@lru_cache(maxsize=None)
def scene(n, pose_name):
    """n landmarks drawn from their covariances around a truth whose rotation is 0.2 degrees off POSES[pose_name]; the frame is
    fused AT POSES[pose_name], so the rotations where the kernels' frame changes are the ones evaluated.  Bearing noise 1e-3;
    bearings are scaled to lengths in [0.5, 2]: any length > 0 is allowed."""
    w = pose_edges.POSES[pose_name]
    seed = 800 + n
    s = rr.make_scene(n, seed, noise=1e-3, rot=w + np.deg2rad(0.2) * wr.EDGE_AXIS)
    cov, root = wr.landmark_cov(s.X, seed)
    rng = np.random.default_rng(seed + 5150)
    X = s.X + np.einsum("iab,ib->ia", root, rng.standard_normal((n, 3))) if n else s.X.copy()
    y = s.y * rng.uniform(0.5, 2.0, size=(n, 1))
    cov = cov / COV_SCALE                                     # so that the handle's prior is the covariance the noise was drawn from
    for a in (X, y, cov):
        a.setflags(write=False)
    return Scene(f"n={n} {pose_name}", X, cov, y, w.copy(), s.tran.copy(), n in LONG)


def scenes(sizes=SIZES + LONG):
    return [scene(n, name) for n in sizes for name in pose_edges.NAMES]


def variants():
    """(bearing_sigma, pose_cov) of every scene."""
    return [(bs, pc) for bs in BEARING_SIGMAS for pc in (None, POSE_COV_FULL)]


def subset(n):
    """About half the landmarks, strictly increasing: the indexed form's idx."""
    rng = np.random.default_rng(4242 + n)
    return np.flatnonzero(rng.random(n) < 0.5).astype(np.int64)


@lru_cache(maxsize=None)
def reference(n, pose_name, bs, with_pose_cov):
    s = scene(n, pose_name)
    return fuse(s.X, s.prior_cov, s.y, s.rot, s.tran, bs, GATE, POSE_COV_FULL if with_pose_cov else None)


def qualify(s, bs, pc):
    """The margins the exact counts rest on, and float64 numpy's own errors on the case -> (ex, ec, es)."""
    ref = reference(len(s.X), s.name.split()[1], bs, pc is not None)
    b = fuse_basis(s.X, s.prior_cov, s.y, s.rot, s.tran, bs, GATE, pc)
    assert np.array_equal(ref.cls, b.cls), s.name
    if len(s.X):
        live = ref.cls != SKIPPED
        assert live.all(), s.name
        assert (np.abs(ref.chi2 - GATE) > MARGIN * GATE).all(), s.name
        assert (np.abs(ref.dstar) > MARGIN).all(), s.name
    return errors(b.X, b.cov, b.chi2, ref, s.X, s.prior_cov)


@lru_cache(maxsize=None)
def measured_errors():
    """float64 numpy's worst errors against long double over EVERY case the GPU test runs: what it multiplies by 8."""
    worst = np.zeros(3)
    for s in scenes():
        for bs, pc in variants():
            worst = np.maximum(worst, qualify(s, bs, pc))
    return tuple(float(v) for v in worst)


# ---- the product's host side through the g++-built harness (tests/harness/landmark_fusion_harness.cpp) --------------------------
_h = None


def harness():
    """csrc/sba_landmarks.hpp compiled for the CPU."""
    global _h
    if _h is None:
        import ctypes as C
        import subprocess
        from pathlib import Path
        root = Path(__file__).resolve().parent.parent
        so = root / "tests" / "harness" / "liblandmark_fusion_harness.so"
        src = root / "tests" / "harness" / "landmark_fusion_harness.cpp"
        hdrs = [root / "spherical_bundle_adjuster_amd" / "csrc" / f
                for f in ("sba_landmarks.hpp", "sba_resection_weighted.hpp", "sba_resection.hpp", "sba_rotation.hpp", "sba_epipolar.hpp")]
        hdrs.append(root / "include" / "sba_hip.h")
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        dp = C.POINTER(C.c_double)
        _h.landmark_fusion_harness_fuse.argtypes = [C.c_longlong, dp, dp, dp, dp, dp, dp, C.c_double, C.c_double, dp, dp, dp,
                                                    C.POINTER(C.c_int)]
        _h.landmark_fusion_harness_check.argtypes = [C.c_int, C.c_double]
        _h.landmark_fusion_harness_check_pose_cov.argtypes = [dp]
        _h.landmark_fusion_harness_check_index.argtypes = [C.POINTER(C.c_int64), C.c_size_t, C.c_size_t]
    return _h


def harness_fuse(X, cov6, y, rot, tran, bearing_sigma=0.0, gate=np.inf, pose_cov=None):
    """csrc/sba_landmarks.hpp's landmark_fuse_fill + landmark_fuse_one per row -> Fused (float64)."""
    import ctypes as C
    a = lambda v: np.ascontiguousarray(v, dtype=np.float64)
    X, cov6, y, rot, tran = a(X), a(cov6), a(y), a(rot), a(tran)
    n = len(X)
    Xo, Co, chi2, cls = np.full((n, 3), np.nan), np.full((n, 6), np.nan), np.full(n, np.nan), np.full(n, -1, dtype=np.int32)
    pcv = None if pose_cov is None else a(pose_cov)
    pc = None if pcv is None else rr._dp(pcv)
    harness().landmark_fusion_harness_fuse(n, rr._dp(X), rr._dp(cov6), rr._dp(y), rr._dp(rot), rr._dp(tran), pc, float(bearing_sigma),
                                           float(gate), rr._dp(Xo), rr._dp(Co), rr._dp(chi2), cls.ctypes.data_as(C.POINTER(C.c_int)))
    return Fused(Xo, Co, chi2, cls.astype(int), np.zeros(n))
