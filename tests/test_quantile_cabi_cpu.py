"""CPU: the order-statistic entry points (sba_problem_residual_order_stats / _keep_below and their batch forms) are declared in
include/sba_hip.h, exported by the library and bound in _cabi.SIGNATURES; nonsense arguments come back as a negative status
with a message before any device is touched; and the quantile -> rank rule is floor(p * (n - 1))."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_problem_residual_order_stats", "sba_problem_keep_below", "sba_batch_residual_order_stats", "sba_batch_keep_below")


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int, name
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2        # additions only
    # each declaration cites the host route it replaces
    for name in NAMES:
        doc = header[:header.index("int %s(" % name)].rsplit("/*", 1)[1]
        assert "Replaces" in doc and "residuals" in doc, name


def _refused(lib, rc):
    assert rc < 0
    assert cabi.last_error(lib) != ""
    return rc


def test_nonsense_arguments_are_refused_without_a_device(lib):
    z3 = (C.c_double * 3)(0, 0, 0)
    rank = (C.c_size_t * 8)(*([0] * 8))
    vals = (C.c_double * 8)()
    kept, thr = C.c_size_t(0), C.c_double(0)
    sz = C.POINTER(C.c_size_t)
    f = lib.sba_problem_residual_order_stats
    assert _refused(lib, f(None, 0, z3, z3, 1.0, 1.0, rank, 1, vals)) == cabi.SBA_ERR_INVALID_ARG       # NULL handle
    assert _refused(lib, f(None, 0, z3, z3, 1.0, 1.0, None, 1, vals)) == cabi.SBA_ERR_INVALID_ARG       # NULL ranks
    assert _refused(lib, f(None, 0, z3, z3, 1.0, 1.0, rank, 1, None)) == cabi.SBA_ERR_INVALID_ARG       # NULL values
    for bad in (0, -1, 9):
        assert _refused(lib, f(None, 0, z3, z3, 1.0, 1.0, rank, bad, vals)) == cabi.SBA_ERR_INVALID_ARG
        assert "num_ranks" in cabi.last_error(lib)
    g = lib.sba_problem_keep_below
    assert _refused(lib, g(None, 0, z3, z3, 1.0, 1.0, 0, 2.0, C.byref(thr), C.byref(kept), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, g(None, 0, z3, z3, 1.0, 1.0, 0, 2.0, None, C.byref(kept), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, g(None, 0, z3, z3, 1.0, 1.0, 0, 2.0, C.byref(thr), None, None)) == cabi.SBA_ERR_INVALID_ARG
    for bad in (-1.0, math.inf, math.nan):
        assert _refused(lib, g(None, 0, z3, z3, 1.0, 1.0, 0, bad, C.byref(thr), C.byref(kept), None)) == cabi.SBA_ERR_INVALID_ARG
        assert "scale" in cabi.last_error(lib)
    fb = lib.sba_batch_residual_order_stats
    assert _refused(lib, fb(None, 0, z3, z3, None, None, rank, 1, vals)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, fb(None, 0, z3, z3, None, None, rank, 0, vals)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, fb(None, 0, z3, z3, None, None, None, 1, vals)) == cabi.SBA_ERR_INVALID_ARG
    gb = lib.sba_batch_keep_below
    one = (C.c_double * 1)(2.0)
    assert _refused(lib, gb(None, 0, z3, z3, None, None, rank, one, vals, C.cast(C.byref(kept), sz), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, gb(None, 0, z3, z3, None, None, None, one, vals, C.cast(C.byref(kept), sz), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, gb(None, 0, z3, z3, None, None, rank, None, vals, C.cast(C.byref(kept), sz), None)) == cabi.SBA_ERR_INVALID_ARG


def test_rank_rule():
    q = api.quantile_rank
    for n in (1, 2, 3, 10, 257, 10_000_001):
        assert q(0.0, n)[0] == 0 and q(1.0, n)[0] == n - 1
        for p in (0.25, 0.5, 0.9, 1.0 / 3.0):
            assert q(p, n)[0] == math.floor(p * (n - 1))
    assert np.array_equal(q([0.0, 0.25, 0.5, 0.9, 1.0], 1), np.zeros(5, dtype=np.uintp))      # n = 1: the only element
    assert np.array_equal(q([0.0, 0.5, 1.0], 2), [0, 0, 1])
    assert q(0.5, 5)[0] == 2 and q(0.5, 4)[0] == 1                                          # the lower neighbour, no interpolation
    assert q([0.1, 0.2], 11).dtype == np.uintp
    for bad in (-0.1, 1.0000001, math.nan):
        with pytest.raises(ValueError):
            q(bad, 10)
    with pytest.raises(ValueError):
        q(0.5, 0)
