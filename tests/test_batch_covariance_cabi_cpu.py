"""CPU: the batched covariance entry point (sba_batch_covariance_joint) is declared in include/sba_hip.h, exported by the
library and bound in _cabi.SIGNATURES; the ABI version stays 2 (an addition); a NULL handle, a NULL out and a negative or NaN
threshold come back as SBA_ERR_INVALID_ARG with a message before any device is touched and with nothing written; the Python
result type carries sigma2 per pair and slices a pair out."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sba_batch_covariance_joint"


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert re.search(r"^int %s\(sba_batch\* b, const double\* rot, const double\* tran, const sba_lm_options\* opt,$" % NAME, header, flags=re.M)
    assert re.search(r"^#define SBA_ABI_VERSION 2\b", header, flags=re.M)
    assert NAME in cabi.SIGNATURES and cabi.SIGNATURES[NAME][0] is C.c_int
    # handle, rot, tran, options, threshold, out, depth_cov, status
    assert cabi.SIGNATURES[NAME][1] == [C.c_void_p, cabi._dp, cabi._dp, C.POINTER(cabi.LmOptions), C.c_double, C.POINTER(cabi.JointCov),
                                        cabi._dp, C.POINTER(C.c_int)]
    assert getattr(lib, NAME) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    assert hasattr(api.Batch, "covariance_joint") and hasattr(api, "BatchJointCovariance")
    # the header says whose contract the per-pair failures follow
    doc = header[header.index("/* sba_batch_covariance_joint:"):header.index("int %s(" % NAME)]
    assert "the contract of sba_batch_solve_joint" in doc and "SBA_BATCH_DEVICE_COV" in doc


def _refused(lib, rc):
    assert rc < 0
    assert cabi.last_error(lib) != ""
    return rc


def test_nonsense_arguments_are_refused_without_a_device(lib):
    f = getattr(lib, NAME)
    z3 = (C.c_double * 3)(0, 0, 1)
    out = (cabi.JointCov * 1)()
    out[0].dim = -7
    dd = (C.c_double * 3)(-7.0, -7.0, -7.0)
    st = (C.c_int * 1)(-7)
    # a NULL handle throughout: nothing here may reach a device
    assert _refused(lib, f(None, z3, z3, None, 0.0, out, dd, st)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(C.c_void_p(0), z3, z3, None, 0.0, out, dd, st)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, z3, None, 0.0, None, None, None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, None, None, None, 0.0, out, dd, st)) == cabi.SBA_ERR_INVALID_ARG
    for bad in (-1e-300, -1.0, -math.inf, math.nan):
        assert _refused(lib, f(None, z3, z3, None, bad, out, dd, st)) == cabi.SBA_ERR_INVALID_ARG
    assert out[0].dim == -7 and list(dd) == [-7.0] * 3 and st[0] == -7         # nothing written


def test_threshold_and_out_are_checked_by_the_entry_point_itself():
    """The two refusals this entry point adds to those of sba_batch_solve_joint are in its source, ahead of the first HIP call
    (a live handle needs a device: tests/test_gpu_batch_covariance.py sends them through one)."""
    src = open(os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc", "sba_batch_covariance.cpp")).read()
    body = src[src.index("int %s(" % NAME):]
    first_hip = body.index("hipSetDevice")
    for needle in ("!(min_sin2_parallax >= 0.0)", "if (!out)", "joint_check(b, rot, tran)"):
        assert 0 <= body.index(needle) < first_hip, needle


def _result():
    B = 3
    cov = np.stack([np.eye(6) * (g + 1) for g in range(B)])
    dd = np.arange(18, dtype=np.float64).reshape(6, 3)
    return api.BatchJointCovariance(cov, dd, cost=np.array([3.0, 3.0, 0.0]), sum_w=np.array([10.0, 5.0, 0.0]),
                                    n_used=np.array([11, 5, 0]), n_degenerate=np.array([1, 0, 0]), dim=np.array([5, 5, 5], dtype=np.int32),
                                    dof=np.array([6, 0, -5], dtype=np.int32), status=np.array([0, 0, cabi.SBA_ERR_NUMERIC], dtype=np.int32),
                                    offsets=np.array([0, 4, 6, 6]))


def test_result_type_sigma2():
    r = _result()
    s2 = r.sigma2
    assert s2.shape == (3,) and s2[0] == 1.0 and math.isnan(s2[1]) and s2[2] == -0.0


def test_result_type_pair():
    r = _result()
    p0, p1, p2 = r.pair(0), r.pair(1), r.pair(2)
    assert isinstance(p0, api.JointCovariance)
    assert np.array_equal(p0.cov, np.eye(6)) and np.array_equal(p1.cov, 2 * np.eye(6))
    assert np.array_equal(p0.depth_cov, r.depth_cov[0:4]) and np.array_equal(p1.depth_cov, r.depth_cov[4:6]) and p2.depth_cov.shape == (0, 3)
    assert (p0.cost, p0.sum_w, p0.n_used, p0.n_degenerate, p0.dim, p0.dof) == (3.0, 10.0, 11, 1, 5, 6)
    assert p0.sigma2 == 1.0 and math.isnan(p1.sigma2)
    nd = api.BatchJointCovariance(r.cov, None, r.cost, r.sum_w, r.n_used, r.n_degenerate, r.dim, r.dof, r.status, r.offsets)
    assert nd.pair(1).depth_cov is None and nd.pair(1).n_used == 5
