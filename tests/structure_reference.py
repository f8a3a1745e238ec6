"""Shared by the structure tests (tests/ only): the DENSE reference of the triangulated landmarks and their covariances.

dense_structure inverts the whole (2n + m) x (2n + m) normal matrix of ref_joint_numpy.JointProblem.jacobian as
cov_reference.dense_covariance does and forms G Sigma G^T per match with its own G = [E diag(-1, 1) / 2 | -F P / 2] from
JointProblem.blocks -- the Jacobian of X_i = ((d1_i u_i - t) + d2_i x2_i) / 2, pinned by finite differences in
tests/test_structure_host_cpu.py.  No Schur complement, no per-match elimination, no depth scaling."""
import numpy as np

import ref_joint_numpy as rj
from cov_reference import dense_covariance


def landmarks(x1, x2, rot, tran, d, dt=np.float64):
    """X (n, 3): the midpoint of the two ray ends in camera 2's frame."""
    d = np.asarray(d, dtype=dt).reshape(-1, 2)
    u = np.asarray(x1, dtype=dt) @ rj.rotation(rot, dt).T
    a = d[:, 0:1] * u - np.asarray(tran, dtype=dt)
    b = d[:, 1:2] * np.asarray(x2, dtype=dt)
    return (a + b) / 2


def landmark_jacobians(x1, x2, rot, tran, d, dt=np.float64):
    """G_d (n, 3, 2) = dX / d(d1, d2) and G_c (n, 3, 6) = dX / d(rot, tran), from the blocks of the joint problem."""
    _, _, E, F = rj.JointProblem(np.asarray(x1), np.asarray(x2), 1.0).blocks(rot, tran, np.asarray(d), dt)
    return E * np.array([-1, 1], dtype=dt) / 2, -F / 2


def pack6(S):
    """(n, 3, 3) -> (n, 6): xx, yy, zz, xy, xz, yz."""
    return np.stack([S[:, 0, 0], S[:, 1, 1], S[:, 2, 2], S[:, 0, 1], S[:, 0, 2], S[:, 1, 2]], axis=1)


class DenseStructure:
    """xyz (n, 3), cov (n, 6), score (n,) [inf, inf, inf, 0, 0, 0 and inf for matches left out], pose: the DenseCov of
    cov_reference.dense_covariance (kappa, kappa_i, sin2, cov, m, n_used, cost, sum_w)."""


def dense_structure(x1, x2, rot, tran, d, tran_param, keep=None, delta=1.0):
    x1, x2 = np.asarray(x1, dtype=np.float64), np.asarray(x2, dtype=np.float64)
    d = np.asarray(d, dtype=np.float64).reshape(-1, 2)
    n_all = len(x1)
    keep = np.ones(n_all, dtype=bool) if keep is None else np.asarray(keep, dtype=bool)
    idx = np.flatnonzero(keep)
    P = rj.JointProblem(x1[idx], x2[idx], delta)
    n = P.n
    J, _ = P.jacobian(rot, tran, d[idx])
    Pm = rj.projection(tran_param, tran)
    m = Pm.shape[1]
    Jl = np.concatenate([J[:, :2 * n], J[:, 2 * n:] @ Pm], axis=1)
    C = np.linalg.inv(Jl.T @ Jl)
    C = 0.5 * (C + C.T)
    Gd, Gc = landmark_jacobians(x1[idx], x2[idx], rot, tran, d[idx])
    G = np.concatenate([Gd, Gc @ Pm], axis=2)                       # (n, 3, 2 + m)
    cols = np.concatenate([2 * np.arange(n)[:, None] + np.arange(2)[None, :], np.tile(2 * n + np.arange(m), (n, 1))], axis=1)
    Sub = C[cols[:, :, None], cols[:, None, :]]                     # (n, 2 + m, 2 + m)
    SX = np.einsum("nia,nab,njb->nij", G, Sub, G)
    r = DenseStructure()
    r.xyz = landmarks(x1, x2, rot, tran, d)
    r.cov = np.zeros((n_all, 6))
    r.cov[:, :3] = np.inf
    r.cov[idx] = pack6(SX)
    r.score = np.full(n_all, np.inf)
    r.score[idx] = (SX[:, 0, 0] + SX[:, 1, 1] + SX[:, 2, 2]) / np.sum(r.xyz[idx] ** 2, axis=1)
    r.pose = dense_covariance(x1, x2, rot, tran, d, tran_param, keep=keep, delta=delta)
    return r


def check_structure(got_xyz, got_cov, got_score, ref, tol, used=None, what=""):
    """The bounds of the structure tests; returns the largest err / bound of (xyz, cov, score).
        |X_i - ref|_max        <= tol * |X_i|
        |Sigma_X,i - ref|_max  <= (2 kappa_i + kappa) * tol * |ref_i|_max      and the same for q_i
    used: matches to compare (default: every match the reference kept).  An output that is None is not compared."""
    rows = np.flatnonzero(np.isfinite(ref.score)) if used is None else np.asarray(used)
    ratios = [0.0, 0.0, 0.0]
    if got_xyz is not None:
        err = np.abs(got_xyz - ref.xyz).max(axis=1)
        ratios[0] = float((err / (tol * np.linalg.norm(ref.xyz, axis=1))).max())
    factor = (2.0 * ref.pose.kappa_i[rows] + ref.pose.kappa) * tol
    if got_cov is not None and len(rows):
        err = np.abs(got_cov[rows] - ref.cov[rows]).max(axis=1)
        ratios[1] = float((err / (factor * np.abs(ref.cov[rows]).max(axis=1))).max())
    if got_score is not None and len(rows):
        ratios[2] = float((np.abs(got_score[rows] - ref.score[rows]) / (factor * np.abs(ref.score[rows]))).max())
    print(f"{what}: kappa {ref.pose.kappa:.3g}, xyz err/bound {ratios[0]:.3g}, cov err/bound {ratios[1]:.3g}, score err/bound {ratios[2]:.3g}")
    assert ratios[0] <= 1.0, (what, "xyz", ratios[0])
    assert ratios[1] <= 1.0, (what, "cov", ratios[1])
    assert ratios[2] <= 1.0, (what, "score", ratios[2])
    return tuple(ratios)
