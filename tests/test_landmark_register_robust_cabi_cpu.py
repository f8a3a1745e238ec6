"""CPU: the four entry points of the robust joint registration are declared in include/sba_hip.h, exported by the library and
bound in _cabi.SIGNATURES; the ABI version stays 2 (additions); the two new records are the existing ones plus n_outlier, in
size and in field order, in the header and in ctypes; a NULL handle is refused by all four as SBA_ERR_INVALID_ARG with a message
before any device is touched and nothing is written; the refusals are decided by host-side checks that come before the first
device call; api.Landmarks carries the two methods and nothing was added to api.Problem or api.Batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_landmarks_eval_register_robust", "sba_landmarks_register_robust", "sba_landmarks_eval_register_robust_device",
         "sba_landmarks_register_robust_device")


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def _struct_fields(header, name):
    body = header[header.index(f"typedef struct {name} {{"):header.index(f"}} {name};")]
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    out = []
    for decl in re.findall(r"^\s*(?:double|int|long long|sba_lm_options|sba_lm_summary)\s+([^;]+);", body, flags=re.M):
        out += [re.sub(r"\[\d+\]", "", f).strip() for f in decl.split(",")]
    return out


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    assert re.search(r"^#define SBA_ABI_VERSION 2$", header, flags=re.M)
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [10, 9, 10, 9]
    # the host forms take the non-robust forms' arguments but for the record; the device twins take the bearings (and chi2) as addresses
    for robust, plain, rec in ((NAMES[0], "sba_landmarks_eval_register", 9), (NAMES[1], "sba_landmarks_register", 7)):
        a, b = list(cabi.SIGNATURES[robust][1]), list(cabi.SIGNATURES[plain][1])
        assert a[:rec] + a[rec + 1:] == b[:rec] + b[rec + 1:] and a[rec] != b[rec], robust
    assert cabi.SIGNATURES[NAMES[2]][1][2] is C.c_void_p and cabi.SIGNATURES[NAMES[3]][1][2] is C.c_void_p
    assert cabi.SIGNATURES[NAMES[3]][1][8] is C.c_void_p
    assert cabi.SIGNATURES[NAMES[2]][1][1] == C.POINTER(C.c_int64) and cabi.SIGNATURES[NAMES[3]][1][1] == C.POINTER(C.c_int64)   # idx: host


def test_the_records_are_the_existing_ones_plus_n_outlier():
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert C.sizeof(cabi.LandmarkRegisterRobustResult) == C.sizeof(cabi.LandmarkRegisterResult) + 8
    assert C.sizeof(cabi.LandmarkRegisterRobustEval) == C.sizeof(cabi.LandmarkRegisterEval) + 8
    for rec, old, name, old_name in (
            (cabi.LandmarkRegisterRobustResult, cabi.LandmarkRegisterResult, "sba_landmark_register_robust_result", "sba_landmark_register_result"),
            (cabi.LandmarkRegisterRobustEval, cabi.LandmarkRegisterEval, "sba_landmark_register_robust_eval", "sba_landmark_register_eval")):
        fields = [f[0] for f in rec._fields_]
        assert _struct_fields(header, name) == fields, name
        assert fields == [f[0] for f in old._fields_] + ["n_outlier"]
        assert _struct_fields(header, name) == _struct_fields(header, old_name) + ["n_outlier"]
        assert [f[1] for f in rec._fields_[:-1]] == [f[1] for f in old._fields_] and rec._fields_[-1][1] is C.c_longlong
        for f in old._fields_:
            assert getattr(rec, f[0]).offset == getattr(old, f[0]).offset, f[0]
    assert "sba_landmark_register_robust_options" not in header          # opt is the existing record


def test_a_null_handle_is_refused_by_all_four_without_a_device(lib):
    z3 = (C.c_double * 3)(0, 0, 1)
    rows = np.full(18, -7.0)
    dp = rows.ctypes.data_as(cabi._dp)
    vp = C.c_void_p(rows.ctypes.data)                                    # never dereferenced: the handle is refused first
    opt = cabi.LandmarkRegisterOptions(0.0, 4.0, 1, api.default_lm_options(huber_delta=2.0))
    res = cabi.LandmarkRegisterRobustResult()
    res.n_obs = res.n_fused = res.n_outlier = -7
    ev = cabi.LandmarkRegisterRobustEval()
    ev.n_used = ev.n_outlier = -7
    calls = (
        lambda: lib.sba_landmarks_register_robust(None, None, dp, 2, z3, z3, C.byref(opt), C.byref(res), dp),
        lambda: lib.sba_landmarks_eval_register_robust(None, None, dp, 2, z3, z3, z3, z3, C.byref(opt), C.byref(ev)),
        lambda: lib.sba_landmarks_register_robust_device(None, None, vp, 2, z3, z3, C.byref(opt), C.byref(res), vp),
        lambda: lib.sba_landmarks_eval_register_robust_device(None, None, vp, 2, z3, z3, z3, z3, C.byref(opt), C.byref(ev)),
    )
    for k, call in enumerate(calls):
        assert call() == cabi.SBA_ERR_INVALID_ARG, k
        assert cabi.last_error(lib) != ""
    assert (rows == -7.0).all() and res.n_obs == -7 and res.n_fused == -7 and res.n_outlier == -7 and ev.n_used == -7 and ev.n_outlier == -7
    assert list(z3) == [0.0, 0.0, 1.0]                                                          # nothing written


def test_every_refusal_is_decided_on_the_host():
    """csrc/sba_landmarks.cpp: robust_check calls the host checks in register_check's order with the loss check replaced, holds no
    device call, and all four entry points reach it before the record is written and before robust_freeze, whose first device
    call is hipSetDevice."""
    src = open(os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc", "sba_landmarks.cpp")).read()
    check = src[src.index("int robust_check("):src.index("bool dense_vectors_fit(")]
    assert "hip" not in check.replace("SBA_ERR_HIP", "")
    order = [check.index(c) for c in ("null argument", "SBA_REFUSE_POISONED", "resect_weight_check_sigma", "landmark_check_gate",
                                      "landmark_check_index", "landmark_register_check_robust", "8-byte aligned", "finite3")]
    assert order == sorted(order)
    assert "SBA_ERR_UNSUPPORTED" not in check
    for common in ("int eval_register_robust_common(", "int register_robust_common("):
        body = src[src.index(common):]
        body = body[body.index("{"):]
        assert 0 <= body.index("robust_check(") < body.index("= sba_landmark_register_robust_") < body.index("robust_freeze("), common
    for entry, common in (("int sba_landmarks_eval_register_robust(", "eval_register_robust_common("),
                          ("int sba_landmarks_register_robust(", "register_robust_common("),
                          ("int sba_landmarks_eval_register_robust_device(", "eval_register_robust_common("),
                          ("int sba_landmarks_register_robust_device(", "register_robust_common(")):
        body = src[src.index(entry):]
        body = body[body.index("{"):body.index("}")]
        assert body.strip("{ \n").startswith("return " + common), entry
    freeze = src[src.index("int robust_freeze("):src.index("int robust_reduce_pass(")]
    assert freeze.index("hipSetDevice") < freeze.index("obs_scratch(") < freeze.index("hipMemcpyAsync")


def test_methods_and_result_types():
    for method in ("eval_register_robust", "register_robust"):
        assert hasattr(api.Landmarks, method), method
        assert not hasattr(api.Problem, method) and not hasattr(api.Batch, method)
    assert not any("robust" in n.lower() and "register" in n.lower() for n in dir(api.Problem) + dir(api.Batch))
    e = api.LandmarkRobustRegisterEquations(H=np.eye(6), g=np.zeros(6), cost=1.0, n_used=5, n_behind=0, n_outlier=2)
    assert isinstance(e, api.LandmarkRegisterEquations) and e.n_outlier == 2
    r = api.LandmarkRobustRegistration(rot=np.zeros(3), tran=np.zeros(3), cov=np.eye(6), summary=None, n_obs=10, n_skipped=1, n_behind=2,
                                       n_gated=3, n_fused=4, n_used=9, chi2=None, n_outlier=3)
    assert isinstance(r, api.LandmarkRegistration) and r.n_outlier == 3
    import inspect
    for method in ("eval_register_robust", "register_robust"):
        sig = inspect.signature(getattr(api.Landmarks, method))
        assert "huber_delta" in sig.parameters and sig.parameters["bearings_device"].default is None
    assert inspect.signature(api.Landmarks.register_robust).parameters["chi2_gate"].default is None     # None: huber_delta ** 2
