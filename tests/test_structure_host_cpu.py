"""CPU: the per-match arithmetic of the triangulated structure (csrc/sba_structure.hpp: structure_block) compiled with g++
(tests/harness/structure_harness.cpp) and driven with U, W, -u, A formed in numpy from ref_joint_numpy.JointProblem.blocks and
the Sigma_c of the host finish (tests/test_covariance_host_cpu.py), against the DENSE reference of tests/structure_reference.py
(G Sigma G^T on the inverse of the whole normal matrix) and, to pin G itself, central finite differences of X_i(d, rot, tran).

Bounds: |X_i - ref| <= REL_TOL_F64 |X_i|;  Sigma_X,i and q_i within (2 kappa_i + kappa) REL_TOL_F64 max|ref_i| -- the bound of
the 2 x 2 depth blocks (tests/cov_reference.py): Sigma_X is a fixed linear image of the blocks that bound covers."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import ref_joint_numpy as rj
from cov_reference import kappa_limit
from helpers import REL_TOL_F64, ROOT
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import synthetic
from structure_reference import check_structure, dense_structure, landmark_jacobians, landmarks
from test_covariance_host_cpu import blocks, product_host

_h = None
_dp = C.POINTER(C.c_double)
SIZES = [5, 63, 64, 65, 257]
GAUGES = [cabi.TRAN_SPHERE, cabi.TRAN_FREE]


def harness():
    global _h
    if _h is None:
        so = ROOT / "tests" / "harness" / "libstructure_harness.so"
        src = ROOT / "tests" / "harness" / "structure_harness.cpp"
        hdrs = [ROOT / "spherical_bundle_adjuster_amd" / "csrc" / f for f in ("sba_structure.hpp", "sba_covariance.hpp", "sba_lm.hpp")]
        if not so.exists() or so.stat().st_mtime < max(f.stat().st_mtime for f in [src] + hdrs):
            subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-I", str(ROOT / "tests" / "harness" / "fake_hip"),
                            "-o", str(so), str(src)], check=True)
        _h = C.CDLL(str(so))
        _h.structure_harness_blocks.restype = C.c_longlong
        _h.structure_harness_blocks.argtypes = [C.c_longlong] + [_dp] * 8 + [C.c_double] + [_dp] * 4
        _h.structure_harness_xyz.restype = None
        _h.structure_harness_xyz.argtypes = [C.c_longlong] + [_dp] * 5
    return _h


def _p(a):
    return a.ctypes.data_as(_dp)


def _points(c):
    return (("init", c.rot_init, c.tran_init), ("true", c.rot_true, c.tran_true))


def product_structure(c, rot, tran, cov36, min_sin2=0.0):
    """-> (xyz, cov, score, n_degenerate) through the harness, at the Sigma_c given."""
    n = len(c.x1)
    U, W, s, _ = blocks(c, rot, tran)
    _, _, E, F = rj.JointProblem(c.x1, c.x2, 1.0).blocks(rot, tran, c.d12)
    nu = np.ascontiguousarray(E[:, :, 0])
    A = np.ascontiguousarray(F[:, :, :3]).reshape(n, 9)
    x2, d, t = np.ascontiguousarray(c.x2, dtype=np.float64), np.ascontiguousarray(c.d12, dtype=np.float64), np.ascontiguousarray(tran, dtype=np.float64)
    xyz, cov, score = np.zeros((n, 3)), np.zeros((n, 6)), np.zeros(n)
    ndeg = harness().structure_harness_blocks(n, _p(U), _p(W), _p(s), _p(nu), _p(A), _p(x2), _p(d), _p(t), min_sin2,
                                              _p(np.ascontiguousarray(cov36).reshape(-1)), _p(xyz), _p(cov), _p(score))
    only = np.zeros((n, 3))
    harness().structure_harness_xyz(n, _p(nu), _p(x2), _p(d), _p(t), _p(only))
    assert only.tobytes() == xyz.tobytes()           # X does not depend on what else is asked for
    return xyz, cov, score, ndeg


@pytest.mark.parametrize("tran_param", GAUGES, ids=["sphere", "free"])
@pytest.mark.parametrize("n", SIZES)
def test_structure_block_against_dense(n, tran_param):
    c = synthetic.full_rt(n, seed=900 + n)
    for name, rot, tran in _points(c):
        rc, cov36, _, dim, ndeg = product_host(c, rot, tran, tran_param)
        if n == 5 and tran_param == cabi.TRAN_FREE:
            assert rc == cabi.SBA_ERR_NUMERIC      # 15 residuals, 16 parameters: no covariance, hence no structure
            continue
        assert rc == 0 and ndeg == 0
        ref = dense_structure(c.x1, c.x2, rot, tran, c.d12, tran_param)
        assert ref.pose.kappa <= kappa_limit(n, tran_param), ref.pose.kappa
        xyz, cov, score, ndeg = product_structure(c, rot, tran, cov36)
        assert ndeg == 0
        check_structure(xyz, cov, score, ref, REL_TOL_F64, what=f"n={n} {name} tran_param={tran_param}")
        # a covariance: positive semi-definite, and the score is its trace over |X|^2 to the bit
        S = np.zeros((n, 3, 3))
        for k, (r, q) in enumerate(((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))):
            S[:, r, q] = S[:, q, r] = cov[:, k]
        assert (np.linalg.eigvalsh(S).min(axis=1) >= -1e-12 * np.abs(cov).max(axis=1)).all()
        assert np.array_equal(score, (cov[:, 0] + cov[:, 1] + cov[:, 2]) / (xyz[:, 0] * xyz[:, 0] + xyz[:, 1] * xyz[:, 1] + xyz[:, 2] * xyz[:, 2]))


@pytest.mark.parametrize("n", SIZES)
def test_reference_jacobian_against_finite_differences(n):
    """G of the reference -- [E diag(-1, 1) / 2 | -F / 2] -- is the derivative of X_i(d, rot, tran): central differences in
    long double, step h = 1e-6: truncation h^2 |X'''| / 6 <= 2e-13 d plus rounding eps_ld |X| / h <= 1e-13 d with d the largest
    depth -- held to 1e-11 max(1, d)."""
    c = synthetic.full_rt(n, seed=900 + n)
    ld, h = np.longdouble, np.longdouble(1e-6)
    for name, rot, tran in _points(c):
        Gd, Gc = landmark_jacobians(c.x1, c.x2, rot, tran, c.d12)
        d = c.d12.astype(ld)
        scale = max(1.0, float(np.abs(c.d12).max()))
        for k in range(2):
            dp, dm = d.copy(), d.copy()
            dp[:, k] += h; dm[:, k] -= h
            fd = (landmarks(c.x1, c.x2, rot, tran, dp, ld) - landmarks(c.x1, c.x2, rot, tran, dm, ld)) / (2 * h)
            assert np.abs(fd - Gd[:, :, k]).max() <= 1e-11 * scale, (name, "depth", k)
        for k in range(6):
            rp, rm, tp, tm = (np.asarray(v, dtype=ld).copy() for v in (rot, rot, tran, tran))
            if k < 3:
                rp[k] += h; rm[k] -= h
            else:
                tp[k - 3] += h; tm[k - 3] -= h
            fd = (landmarks(c.x1, c.x2, rp, tp, d, ld) - landmarks(c.x1, c.x2, rm, tm, d, ld)) / (2 * h)
            assert np.abs(fd - Gc[:, :, k]).max() <= 1e-11 * scale, (name, "camera", k)
        # and the landmark closes the residual: b - a = e, X = b - e / 2
        e = rj.JointProblem(c.x1, c.x2).residuals(rot, tran, c.d12)
        X = landmarks(c.x1, c.x2, rot, tran, c.d12)
        assert np.abs(X - (c.d12[:, 1:2] * c.x2 - e / 2)).max() <= REL_TOL_F64 * np.abs(X).max()


def test_degenerate_rows():
    """A match cov_block leaves out keeps its X, has the row (inf, inf, inf, 0, 0, 0) and the score inf; the others are
    the problem without it (Sigma_c from that problem)."""
    n, planted = 65, np.array([1, 64])
    c = synthetic.full_rt(n, seed=900 + n)
    rot, tran = c.rot_init, c.tran_init
    x2 = c.x2.copy()
    x2[planted] = c.x1[planted] @ rj.rotation(rot).T
    cd = type(c)(c.x1, x2, c.d12, c.rot_true, c.tran_true, c.rot_init, c.tran_init)
    keep = np.ones(n, dtype=bool)
    keep[planted] = False
    less = type(c)(c.x1[keep], x2[keep], c.d12[keep], c.rot_true, c.tran_true, c.rot_init, c.tran_init)
    rc, cov36, _, dim, ndeg = product_host(less, rot, tran, cabi.TRAN_SPHERE, min_sin2=1e-9)
    assert rc == 0 and ndeg == 0
    xyz, cov, score, ndeg = product_structure(cd, rot, tran, cov36, min_sin2=1e-9)
    assert ndeg == 2
    assert np.array_equal(cov[planted], np.tile([np.inf, np.inf, np.inf, 0.0, 0.0, 0.0], (2, 1)))
    assert np.array_equal(score[planted], [np.inf, np.inf]) and np.isfinite(xyz).all()
    ref = dense_structure(cd.x1, cd.x2, rot, tran, cd.d12, cabi.TRAN_SPHERE, keep=keep)
    assert ref.pose.kappa <= kappa_limit(n, cabi.TRAN_SPHERE)
    check_structure(xyz, cov, score, ref, REL_TOL_F64, used=np.flatnonzero(keep), what="planted n=65")
    assert np.abs(xyz[planted] - ref.xyz[planted]).max() <= REL_TOL_F64 * np.abs(ref.xyz[planted]).max()
