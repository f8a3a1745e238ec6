"""Shared by the covariance tests (tests/ only): the DENSE reference of the joint problem's covariance and the scene
conditions the tests' bounds rest on.

dense_covariance inverts the whole (2n + m) x (2n + m) normal matrix of the robustified Jacobian of
ref_joint_numpy.JointProblem.jacobian -- camera columns through projection(tran_param, tran) -- and reads the camera block
and the matches' 2x2 diagonal blocks off the inverse.  It forms no Schur complement, no per-match elimination and no
depth scaling: it shares no algebra with the product."""
import numpy as np

import ref_joint_numpy as rj


class DenseCov:
    """cov (6, 6), depth_cov (n, 3) [inf, inf, 0 for matches left out], kappa (unit-diagonal projected S), kappa_i (n,),
    sin2 (n,), cost, sum_w, n_used, m."""


def sin2_parallax(x1, x2, rot):
    """sin^2 of the angle between R x1 and x2 per match."""
    u = np.asarray(x1, dtype=np.float64) @ rj.rotation(rot).T
    x2 = np.asarray(x2, dtype=np.float64)
    c2 = np.sum(u * x2, axis=1) ** 2 / (np.sum(u * u, axis=1) * np.sum(x2 * x2, axis=1))
    return 1.0 - c2


def dense_covariance(x1, x2, rot, tran, d, tran_param, keep=None, delta=1.0):
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    n_all = len(x1)
    keep = np.ones(n_all, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    idx = np.flatnonzero(keep)
    P = rj.JointProblem(x1[idx], x2[idx], delta)
    n = P.n
    J, f = P.jacobian(rot, tran, d[idx])
    Pm = rj.projection(tran_param, tran)
    m = Pm.shape[1]
    Jl = np.concatenate([J[:, :2 * n], J[:, 2 * n:] @ Pm], axis=1)
    C = np.linalg.inv(Jl.T @ Jl)
    C = 0.5 * (C + C.T)
    r = DenseCov()
    r.m, r.n_used = m, n
    Ccc = C[2 * n:, 2 * n:]
    r.cov = Pm @ Ccc @ Pm.T
    r.depth_cov = np.zeros((n_all, 3))
    r.depth_cov[:, :2] = np.inf
    k = 2 * np.arange(n)
    r.depth_cov[idx, 0], r.depth_cov[idx, 1], r.depth_cov[idx, 2] = C[k, k], C[k + 1, k + 1], C[k, k + 1]
    # conditions: the unit-diagonal projected S = (C_cc)^-1, the unit-diagonal U_i = [[1, c], [c, 1]], c the rays' cosine
    S = np.linalg.inv(Ccc)
    s = 1.0 / np.sqrt(np.diag(S))
    r.kappa = float(np.linalg.cond(S * s[:, None] * s[None, :]))
    r.sin2 = sin2_parallax(x1, x2, rot)
    c = np.sqrt(np.clip(1.0 - r.sin2, 0.0, 1.0))
    with np.errstate(divide="ignore"):
        r.kappa_i = (1.0 + c) / (1.0 - c)
    e = P.residuals(rot, tran, d[idx])
    rho, w = rj.huber(delta, np.sum(e * e, axis=1))
    r.cost, r.sum_w = 0.5 * float(rho.sum()), float(w.sum())
    return r


def kappa_limit(n, tran_param):
    """The scene condition that keeps the bounds meaningful: kappa <= 10 on the sphere, <= 1e4 with free translation.
    Measured on the seeds 900 + n: <= 7.4 and <= 2.4e3 for n >= 63.  n = 5 on the sphere is the square system (15 residuals,
    10 depths + 5 camera parameters) and measures 147 at the initial pose, 62 at the true one: it is held to the 1e4 of the
    free gauge.  The bounds themselves scale with the measured kappa either way."""
    return 10.0 if tran_param == 1 and n > 5 else 1e4


def check_against(got_cov, got_dd, ref, tol, used=None, what=""):
    """The two bounds of the covariance tests; returns the largest err / bound of either.  used: matches to compare
    (default: every match the reference kept)."""
    scale = np.abs(ref.cov).max()
    err_c = np.abs(got_cov - ref.cov).max()
    bound_c = ref.kappa * tol * scale
    ratio_c = err_c / bound_c
    ratio_d = 0.0
    if got_dd is not None:
        rows = np.flatnonzero(np.isfinite(ref.depth_cov[:, 0])) if used is None else np.asarray(used)
        err = np.abs(got_dd[rows] - ref.depth_cov[rows]).max(axis=1)
        bound = (2.0 * ref.kappa_i[rows] + ref.kappa) * tol * np.abs(ref.depth_cov[rows]).max(axis=1)
        ratio_d = float((err / bound).max()) if len(rows) else 0.0
    print(f"{what}: kappa {ref.kappa:.3g}, camera err/bound {ratio_c:.3g}, depth err/bound {ratio_d:.3g}")
    assert ratio_c <= 1.0, (what, "camera", err_c, bound_c)
    assert ratio_d <= 1.0, (what, "depth", ratio_d)
    return ratio_c, ratio_d
