"""CPU: the four structure entry points (sba_problem_structure_joint, ..._joint_device, ..._order_stats, ..._keep_below) are
declared in include/sba_hip.h, exported by the library and bound in _cabi.SIGNATURES; the ABI version stays 2 (additions);
NULL and nonsense arguments come back as a negative status with a message before any device is touched; Problem carries the
methods; without a device the handle itself fails loudly."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_problem_structure_joint", "sba_problem_structure_joint_device", "sba_problem_structure_order_stats",
         "sba_problem_structure_keep_below")


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
    # prototypes: the two forms differ only in what the three destinations are
    host, dev = cabi.SIGNATURES[NAMES[0]][1], cabi.SIGNATURES[NAMES[1]][1]
    assert len(host) == len(dev) == 9 and host[:6] == dev[:6]
    assert len(cabi.SIGNATURES[NAMES[2]][1]) == 8 and len(cabi.SIGNATURES[NAMES[3]][1]) == 10
    for method in ("structure_joint", "structure_joint_into", "structure_order_stats", "structure_keep_below"):
        assert hasattr(api.Problem, method), method


def _refused(lib, rc):
    assert rc < 0
    assert cabi.last_error(lib) != ""
    return rc


def test_nonsense_arguments_are_refused_without_a_device(lib):
    z3 = (C.c_double * 3)(0, 0, 1)
    out = cabi.JointCov()
    out.dim = -7
    xyz = np.full(6, -7.0)
    px = xyz.ctypes.data_as(cabi._dp)
    for f in (lib.sba_problem_structure_joint, lib.sba_problem_structure_joint_device):     # NULL handle throughout
        assert _refused(lib, f(None, z3, z3, None, 0.0, C.byref(out), None, None, None)) == cabi.SBA_ERR_INVALID_ARG
        assert _refused(lib, f(None, None, z3, None, 0.0, C.byref(out), None, None, None)) == cabi.SBA_ERR_INVALID_ARG
        assert _refused(lib, f(None, z3, z3, None, 0.0, None, None, None, None)) == cabi.SBA_ERR_INVALID_ARG
        for bad in (-1e-300, -1.0, -math.inf, math.nan):
            assert _refused(lib, f(None, z3, z3, None, bad, C.byref(out), None, None, None)) == cabi.SBA_ERR_INVALID_ARG
    # a destination that is not 16-byte aligned is refused before anything else is looked at
    odd = C.c_void_p(xyz.ctypes.data + 8 if xyz.ctypes.data % 16 == 0 else xyz.ctypes.data)
    assert odd.value % 16 == 8
    for k in range(3):
        dest = [None, None, None]
        dest[k] = odd
        assert _refused(lib, lib.sba_problem_structure_joint_device(None, z3, z3, None, 0.0, C.byref(out), *dest)) == cabi.SBA_ERR_INVALID_ARG
        assert "aligned" in cabi.last_error(lib)
    ranks, vals = (C.c_size_t * 1)(0), (C.c_double * 1)(-7.0)
    f = lib.sba_problem_structure_order_stats
    assert _refused(lib, f(None, z3, z3, None, 0.0, ranks, 1, vals)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, z3, None, 0.0, None, 1, vals)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, z3, None, 0.0, ranks, 1, None)) == cabi.SBA_ERR_INVALID_ARG
    for bad in (0, 9, -1):
        assert _refused(lib, f(None, z3, z3, None, 0.0, ranks, bad, vals)) == cabi.SBA_ERR_INVALID_ARG
    thr, kept = C.c_double(-7.0), C.c_size_t(7)
    f = lib.sba_problem_structure_keep_below
    assert _refused(lib, f(None, z3, z3, None, 0.0, 0, 1.0, thr, C.byref(kept), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, z3, None, 0.0, 0, 1.0, None, C.byref(kept), None)) == cabi.SBA_ERR_INVALID_ARG
    assert _refused(lib, f(None, z3, z3, None, 0.0, 0, 1.0, thr, None, None)) == cabi.SBA_ERR_INVALID_ARG
    for bad in (-1.0, math.inf, math.nan):
        assert _refused(lib, f(None, z3, z3, None, 0.0, 0, bad, thr, C.byref(kept), None)) == cabi.SBA_ERR_INVALID_ARG
    assert out.dim == -7 and (xyz == -7.0).all() and vals[0] == -7.0 and thr.value == -7.0 and kept.value == 7    # nothing written
    del px


def _has_gpu():
    try:
        return api.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a box without a GPU")
def test_fails_loudly_without_device():
    """There is no CPU path to a landmark: the handle the methods need cannot be made."""
    with pytest.raises(api.SbaError) as ei:
        with api.Problem(0) as p:
            p.structure_joint(np.zeros(3), np.array([0.0, 0.0, 1.0]))
    assert ei.value.code == cabi.SBA_ERR_NO_DEVICE


def test_result_type():
    pose = api.JointCovariance(np.eye(6), None, cost=3.0, sum_w=10.0, n_used=11, n_degenerate=1, dim=5, dof=6)
    r = api.JointStructure(np.zeros((2, 3)), None, None, pose)
    assert r.sigma2 == 1.0 and r.n_used == 11 and r.n_degenerate == 1 and r.dim == 5 and r.dof == 6 and r.cost == 3.0
    with pytest.raises(AttributeError):
        r.no_such_field
