"""CPU: the seven entry points of the covariance-weighted resection are declared in include/sba_hip.h, exported by the library and
bound in _cabi.SIGNATURES; the ABI version stays 2 (additions); a NULL handle or NULL arrays come back as SBA_ERR_INVALID_ARG with
a message before any device is touched and nothing is written; Problem carries the methods."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_problem_resection_set_landmark_cov", "sba_problem_resection_set_landmark_cov_device",
         "sba_problem_resection_freeze_weights", "sba_problem_resection_weights", "sba_problem_eval_resection_weighted",
         "sba_problem_solve_resection_weighted", "sba_problem_resection_covariance")


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [3, 3, 5, 2, 5, 9, 5]
    # the record matches the header's struct: 36 + 2 doubles, two 64-bit counts, a double, a 64-bit count, a double
    assert C.sizeof(cabi.ResectionCov) == 43 * 8
    body = header[header.index("typedef struct sba_resection_cov"):header.index("} sba_resection_cov;")]
    assert re.findall(r"\b(cov|cost|sum_w|n_used|n_zero_weight|n_outlier|dof|sigma2)\b(?=[\[;,])", body) == \
           [f[0] for f in cabi.ResectionCov._fields_]
    for method in ("set_landmark_covariances", "set_landmark_covariances_device", "freeze_resection_weights", "resection_weights",
                   "eval_resection_weighted", "solve_resection_weighted", "resection_covariance"):
        assert hasattr(api.Problem, method), method


def test_null_arguments_are_refused_without_a_device(lib):
    z3 = (C.c_double * 3)(0, 0, 1)
    cov = np.full(6, -7.0)
    dp = cov.ctypes.data_as(cabi._dp)
    eq = cabi.ResectionEq()
    eq.n_behind = -7.0
    res = cabi.ResectionCov()
    res.dof = -7
    s = cabi.LmSummary()
    s.termination = -7
    nb, nz = C.c_double(-7.0), C.c_longlong(-7)
    calls = (
        lambda: lib.sba_problem_resection_set_landmark_cov(None, dp, 1.0),
        lambda: lib.sba_problem_resection_set_landmark_cov_device(None, C.c_void_p(16), 1.0),
        lambda: lib.sba_problem_resection_freeze_weights(None, z3, z3, 0.0, C.byref(nz)),
        lambda: lib.sba_problem_resection_weights(None, dp),
        lambda: lib.sba_problem_eval_resection_weighted(None, z3, z3, None, C.byref(eq)),
        lambda: lib.sba_problem_solve_resection_weighted(None, z3, z3, None, 0.0, 1, C.byref(s), C.byref(nb), 1),
        lambda: lib.sba_problem_resection_covariance(None, z3, z3, None, C.byref(res)),
    )
    for k, call in enumerate(calls):
        assert call() == cabi.SBA_ERR_INVALID_ARG, NAMES[k]
        assert cabi.last_error(lib) != ""
    assert eq.n_behind == -7.0 and res.dof == -7 and s.termination == -7 and nb.value == -7.0 and nz.value == -7
    assert (cov == -7.0).all() and list(z3) == [0.0, 0.0, 1.0]                                   # nothing written


def test_result_type():
    c = api.ResectionCovariance(np.eye(6), cost=5.0, sum_w=10.0, n_used=10, n_zero_weight=1, n_outlier=0.0, dof=14, sigma2=5.0 / 7)
    assert c.cov.shape == (6, 6) and c.dof == 2 * c.n_used - 6
