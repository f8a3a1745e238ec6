"""CPU: the HIP-free part of the joint covariance (csrc/sba_covariance.hpp) -- the host finish (project, Jacobi-scale,
Cholesky, invert, un-scale, lift) and the per-match 2x2 block arithmetic both kernels run -- compiled with g++
(tests/harness/cov_harness.cpp) and driven with S, U, W formed in numpy from ref_joint_numpy.JointProblem.blocks, against the
DENSE reference of tests/cov_reference.py (the inverse of the whole normal matrix: no Schur complement).

Bounds (first-order perturbation of an inverse, the project's REL_TOL_F64 on S, U, W):
    |Sigma_c - ref|_max    <= kappa * TOL * |ref|_max                 kappa: 2-norm condition of the unit-diagonal projected S
    |Sigma_dd,i - ref_i|_max <= (2 kappa_i + kappa) * TOL * |ref_i|_max   kappa_i: condition of the unit-diagonal U_i."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ref_joint_numpy as rj
from cov_reference import check_against, dense_covariance, kappa_limit
from helpers import REL_TOL_F64, ROOT
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import synthetic

_h = None
_dp = C.POINTER(C.c_double)


def harness():
    global _h
    if _h is None:
        so = ROOT / "tests" / "harness" / "libcov_harness.so"
        src = ROOT / "tests" / "harness" / "cov_harness.cpp"
        hdrs = [ROOT / "spherical_bundle_adjuster_amd" / "csrc" / f for f in ("sba_covariance.hpp", "sba_lm.hpp")]
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", str(ROOT / "tests" / "harness" / "fake_hip"),
                            "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        _h.cov_harness_blocks.restype = C.c_longlong
        _h.cov_harness_blocks.argtypes = [C.c_longlong, _dp, _dp, _dp, C.c_double, _dp, _dp, _dp]
        _h.cov_harness_finish.argtypes = [_dp, C.c_int, _dp, C.c_longlong, _dp, C.POINTER(C.c_int)]
    return _h


def _p(a):
    return a.ctypes.data_as(_dp)


def blocks(c, rot, tran):
    """What the reduce kernel forms per match, in numpy: U (n, 3), W (n, 12), s (n, 2), sum w F^T F (6, 6)."""
    e, w, E, F = rj.JointProblem(c.x1, c.x2, 1.0).blocks(rot, tran, c.d12)
    EtE = np.einsum("nri,nrj->nij", E, E) * w[:, None, None]
    s = 1.0 / (1.0 + np.sqrt(np.stack([EtE[:, 0, 0], EtE[:, 1, 1]], axis=1)))
    Us = EtE * s[:, :, None] * s[:, None, :]
    W = np.einsum("nri,nrj->nij", E, F) * w[:, None, None] * s[:, :, None]
    V = (np.einsum("nri,nrj->nij", F, F) * w[:, None, None]).sum(0)
    U = np.ascontiguousarray(np.stack([Us[:, 0, 0], Us[:, 0, 1], Us[:, 1, 1]], axis=1))
    return U, np.ascontiguousarray(W.reshape(len(w), 12)), np.ascontiguousarray(s), V


def product_host(c, rot, tran, tran_param, min_sin2=0.0):
    """-> (rc, cov, depth_cov, dim, n_degenerate) through the harness."""
    h = harness()
    n = len(c.x1)
    U, W, s, V = blocks(c, rot, tran)
    S21, dd = np.zeros(21), np.zeros((n, 3))
    ndeg = h.cov_harness_blocks(n, _p(U), _p(W), _p(s), min_sin2, None, None, _p(S21))
    S21 += V[np.triu_indices(6)]
    cov, dim = np.full(36, -7.0), C.c_int(-7)
    tran = np.ascontiguousarray(tran, dtype=np.float64)
    rc = h.cov_harness_finish(_p(S21), tran_param, _p(tran), n - ndeg, _p(cov), C.byref(dim))
    if rc != 0:
        assert (cov == -7.0).all() and dim.value == -7       # nothing written
        return rc, None, None, None, ndeg
    assert h.cov_harness_blocks(n, _p(U), _p(W), _p(s), min_sin2, _p(cov), _p(dd), None) == ndeg
    return rc, cov.reshape(6, 6), dd, dim.value, ndeg


@pytest.mark.parametrize("tran_param", [cabi.TRAN_SPHERE, cabi.TRAN_FREE], ids=["sphere", "free"])
@pytest.mark.parametrize("n", [5, 63, 64, 65])
def test_host_finish_and_blocks_against_dense(n, tran_param):
    c = synthetic.full_rt(n, seed=900 + n)
    for name, rot, tran in (("init", c.rot_init, c.tran_init), ("true", c.rot_true, c.tran_true)):
        rc, cov, dd, dim, ndeg = product_host(c, rot, tran, tran_param)
        if n == 5 and tran_param == cabi.TRAN_FREE:
            assert rc == cabi.SBA_ERR_NUMERIC      # 15 residuals, 16 parameters
            continue
        assert rc == 0 and ndeg == 0 and dim == (5 if tran_param == cabi.TRAN_SPHERE else 6)
        ref = dense_covariance(c.x1, c.x2, rot, tran, c.d12, tran_param)
        assert ref.kappa <= kappa_limit(n, tran_param), ref.kappa
        check_against(cov, dd, ref, REL_TOL_F64, what=f"n={n} {name} tran_param={tran_param}")
        assert np.array_equal(cov, cov.T)
        assert np.linalg.matrix_rank(cov, tol=1e-9 * np.abs(cov).max()) == dim
        if tran_param == cabi.TRAN_SPHERE:
            assert np.abs(cov[3:, 3:] @ tran).max() <= ref.kappa * REL_TOL_F64 * np.abs(cov).max()


@pytest.mark.parametrize("tran_param", [cabi.TRAN_SPHERE, cabi.TRAN_FREE], ids=["sphere", "free"])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_rank_deficient_scenes_are_numeric_errors(n, tran_param):
    c = synthetic.full_rt(n, seed=900 + n)
    rc, *_ = product_host(c, c.rot_init, c.tran_init, tran_param)
    assert rc == cabi.SBA_ERR_NUMERIC


def test_pivot_floor_and_non_finite_system():
    h = harness()
    tran = np.array([0.0, 0.0, 1.0])
    cov, dim = np.full(36, -7.0), C.c_int(-7)
    iu = np.triu_indices(6)
    good = np.eye(6)[iu].copy()
    assert h.cov_harness_finish(_p(good), cabi.TRAN_FREE, _p(tran), 100, _p(cov), C.byref(dim)) == 0
    assert dim.value == 6 and np.array_equal(cov.reshape(6, 6), np.eye(6))
    assert h.cov_harness_finish(_p(good), cabi.TRAN_FREE, _p(tran), 5, _p(cov), C.byref(dim)) == cabi.SBA_ERR_NUMERIC    # n_used < m
    assert h.cov_harness_finish(_p(good), cabi.TRAN_SPHERE, _p(tran), 5, _p(cov), C.byref(dim)) == 0 and dim.value == 5
    # sphere: the direction along tran carries no variance, the tangent plane does
    assert np.array_equal(cov.reshape(6, 6)[5], np.zeros(6)) and cov.reshape(6, 6)[3, 3] == 1.0
    before = cov.copy()
    for bad in (np.nan, np.inf):
        S = good.copy(); S[7] = bad
        assert h.cov_harness_finish(_p(S), cabi.TRAN_FREE, _p(tran), 100, _p(cov), C.byref(dim)) == cabi.SBA_ERR_NUMERIC
    # two equal columns: the second pivot of the unit-diagonal system is 0; nearly equal: below m * eps
    for off in (1.0, 1.0 - 1e-16, 1.0 - 2.0 * np.finfo(float).eps):
        M = np.eye(6); M[0, 1] = M[1, 0] = off
        assert h.cov_harness_finish(_p(M[iu].copy()), cabi.TRAN_FREE, _p(tran), 100, _p(cov), C.byref(dim)) == cabi.SBA_ERR_NUMERIC
    M = np.eye(6); M[0, 1] = M[1, 0] = 1.0 - 1e-12     # pivot 2e-12 > 6 eps: accepted
    assert h.cov_harness_finish(_p(M[iu].copy()), cabi.TRAN_FREE, _p(tran), 100, _p(cov), C.byref(dim)) == 0
    assert h.cov_harness_finish(_p((-np.eye(6))[iu].copy()), cabi.TRAN_FREE, _p(tran), 100, _p(before), C.byref(dim)) == cabi.SBA_ERR_NUMERIC


def test_degenerate_blocks():
    """Parallel rays: sin^2 = 0 <= any threshold; the rule uses the scaled block alone (weight and scaling cancel)."""
    h = harness()
    U = np.array([[2.0, 2.0, 2.0], [1.0, 0.5, 1.0], [1.0, np.nan, 1.0], [0.0, 0.0, 0.0], [1.0, 0.999, 1.0]])
    W = np.ones((5, 12)); s = np.ones((5, 2)); out = np.zeros((5, 3)); cov = np.eye(6).reshape(-1).copy()
    assert h.cov_harness_blocks(5, _p(U), _p(W), _p(s), 0.0, _p(cov), _p(out), None) == 3
    for i in (0, 2, 3):
        assert np.array_equal(out[i], [np.inf, np.inf, 0.0])
    assert np.isfinite(out[[1, 4]]).all()
    # sin^2 of row 4 is 1 - 0.999^2 = 1.999e-3
    assert h.cov_harness_blocks(5, _p(U), _p(W), _p(s), 2e-3, _p(cov), _p(out), None) == 4
    assert h.cov_harness_blocks(5, _p(U), _p(W), _p(s), 1.9e-3, _p(cov), _p(out), None) == 3
    # the block of row 1 by hand: U^-1 = [[4/3, -2/3], [-2/3, 4/3]], T rows = U^-1 W = (2/3) 1, T Sigma T^T = 6 * 4/9
    assert np.allclose(out[1], [4 / 3 + 8 / 3, 4 / 3 + 8 / 3, -2 / 3 + 8 / 3], rtol=1e-15)
