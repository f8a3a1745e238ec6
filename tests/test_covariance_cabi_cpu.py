"""CPU: the covariance entry point (sba_problem_covariance_joint) is declared in include/sba_hip.h, exported by the library
and bound in _cabi.SIGNATURES; the ABI version stays 2 (an addition); NULL and nonsense arguments come back as a negative
status with a message before any device is touched; the Python result type carries sigma2."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "sba_problem_covariance_joint"


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert re.search(r"^int %s\(" % NAME, header, flags=re.M)
    assert re.search(r"^#define SBA_ABI_VERSION 2\b", header, flags=re.M)
    assert NAME in cabi.SIGNATURES and cabi.SIGNATURES[NAME][0] is C.c_int
    assert getattr(lib, NAME) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    # the struct the header declares and its ctypes mirror agree: 36 + 2 doubles, two 64-bit counts, two ints
    body = header[header.index("typedef struct sba_joint_cov {"):header.index("} sba_joint_cov;")]
    for field in ("double cov[36]", "double cost, sum_w", "long long n_used, n_degenerate", "int dim, dof"):
        assert field in body, field
    assert C.sizeof(cabi.JointCov) == 36 * 8 + 2 * 8 + 2 * 8 + 2 * 4
    assert [f[0] for f in cabi.JointCov._fields_] == ["cov", "cost", "sum_w", "n_used", "n_degenerate", "dim", "dof"]
    assert hasattr(api.Problem, "covariance_joint")


def _refused(lib, rc):
    assert rc < 0
    assert cabi.last_error(lib) != ""
    return rc


def test_nonsense_arguments_are_refused_without_a_device(lib):
    f = lib.sba_problem_covariance_joint
    z3 = (C.c_double * 3)(0, 0, 1)
    out = cabi.JointCov()
    out.dim = -7
    fake = C.c_void_p(0)        # NULL handle throughout: nothing here may reach a device
    assert _refused(lib, f(fake, z3, z3, None, 0.0, C.byref(out), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, None, z3, None, 0.0, C.byref(out), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, None, None, 0.0, C.byref(out), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, z3, None, 0.0, None, None)) == cabi.SBA_ERR_INVALID_ARG
    for bad in (-1e-300, -1.0, -math.inf, math.nan):
        assert _refused(lib, f(None, z3, z3, None, bad, C.byref(out), None)) == cabi.SBA_ERR_INVALID_ARG
    assert out.dim == -7         # nothing written


def test_result_type():
    r = api.JointCovariance(np.eye(6), None, cost=3.0, sum_w=10.0, n_used=11, n_degenerate=1, dim=5, dof=6)
    assert r.sigma2 == 1.0
    r0 = api.JointCovariance(np.eye(6), None, cost=3.0, sum_w=5.0, n_used=5, n_degenerate=0, dim=5, dof=0)
    assert math.isnan(r0.sigma2)
