"""CPU: the four resection entry points (sba_problem_eval_resection, ..._solve_resection, ..._resection_depths,
..._resection_guess) are declared in include/sba_hip.h, exported by the library and bound in _cabi.SIGNATURES; the ABI version
stays 2 (additions); NULL and nonsense arguments come back as a negative status with a message before any device is touched and
nothing is written; Problem carries the methods; without a device the handle itself fails loudly."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_problem_eval_resection", "sba_problem_solve_resection", "sba_problem_resection_depths", "sba_problem_resection_guess")


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert re.search(r"^#define SBA_ABI_VERSION 2\b", header, flags=re.M)
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [5, 7, 4, 5]
    # the records match the header's structs: a normal-equation record plus one double; 7 doubles, a 64-bit count, a double
    assert C.sizeof(cabi.ResectionEq) == C.sizeof(cabi.NormalEq) + 8
    assert C.sizeof(cabi.ResectionGuessInfo) == 9 * 8
    for field in ("lambda1", "lambda2", "lambda12", "sv", "scale", "n", "n_behind"):
        assert re.search(r"\b%s\b" % field, header[header.index("typedef struct sba_resection_guess_info"):]), field
    for method in ("eval_resection", "solve_resection", "resection_depths", "resection_guess", "upload_landmarks"):
        assert hasattr(api.Problem, method), method


def _refused(lib, rc):
    assert rc < 0
    assert cabi.last_error(lib) != ""
    return rc


def test_nonsense_arguments_are_refused_without_a_device(lib):
    """Every argument check comes before the first device call: there is no device here, and nothing is written."""
    z3, bad3 = (C.c_double * 3)(0, 0, 1), (C.c_double * 3)(0, math.nan, 1)
    eq = cabi.ResectionEq()
    eq.n_behind = -7.0
    info = cabi.ResectionGuessInfo()
    info.n = -7
    s = cabi.LmSummary()
    s.termination = -7
    nb = C.c_double(-7.0)
    out = np.full(4, -7.0)
    f = lib.sba_problem_eval_resection
    for args in ((None, z3, z3, None, C.byref(eq)), (None, None, z3, None, C.byref(eq)), (None, z3, None, None, C.byref(eq)),
                 (None, z3, z3, None, None), (None, bad3, z3, None, C.byref(eq))):
        assert _refused(lib, f(*args)) == cabi.SBA_ERR_INVALID_ARG
    f = lib.sba_problem_solve_resection
    for args in ((None, z3, z3, None, C.byref(s), C.byref(nb), 1), (None, None, z3, None, C.byref(s), C.byref(nb), 0),
                 (None, z3, None, None, None, None, 0)):
        assert _refused(lib, f(*args)) == cabi.SBA_ERR_INVALID_ARG
    f = lib.sba_problem_resection_depths
    for args in ((None, z3, z3, out.ctypes.data_as(cabi._dp)), (None, None, z3, None), (None, z3, None, None)):
        assert _refused(lib, f(*args)) == cabi.SBA_ERR_INVALID_ARG
    f = lib.sba_problem_resection_guess
    r3, t3 = (C.c_double * 3)(-7, -7, -7), (C.c_double * 3)(-7, -7, -7)
    for args in ((None, r3, t3, C.byref(info), None), (None, None, t3, C.byref(info), None), (None, r3, None, C.byref(info), None),
                 (None, r3, t3, None, out.ctypes.data_as(cabi._dp))):
        assert _refused(lib, f(*args)) == cabi.SBA_ERR_INVALID_ARG
    assert eq.n_behind == -7.0 and info.n == -7 and s.termination == -7 and nb.value == -7.0 and (out == -7.0).all()
    assert list(r3) == [-7.0] * 3 and list(t3) == [-7.0] * 3 and list(z3) == [0.0, 0.0, 1.0]           # nothing written


def _has_gpu():
    try:
        return api.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a box without a GPU")
def test_fails_loudly_without_device():
    """There is no CPU path to a resection: the handle the methods need cannot be made."""
    with pytest.raises(api.SbaError) as ei:
        with api.Problem(0) as p:
            p.solve_resection(np.zeros(3), np.zeros(3))
    assert ei.value.code == cabi.SBA_ERR_NO_DEVICE


def test_result_types():
    e = api.ResectionEquations(np.eye(6), np.zeros(6), cost=3.0, sum_w=10.0, n_outlier=1.0, n_behind=2.0)
    assert e.n_behind == 2.0 and e.H.shape == (6, 6)
    g = api.ResectionGuess(np.zeros(3), np.zeros(3), 0.0, 1.0, 2.0, np.ones(3), 1.0, 7, 0.0, None)
    assert g.n == 7 and g.lambda2 == 1.0 and g.moments is None
