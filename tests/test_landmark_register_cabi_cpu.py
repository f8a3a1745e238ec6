"""CPU: the two entry points of the joint registration are declared in include/sba_hip.h, exported by the library and bound in
_cabi.SIGNATURES; the ABI version stays 2 (additions); the three records match the header's structs in size and field order; a
NULL handle or NULL arguments come back as SBA_ERR_INVALID_ARG with a message before any device is touched and nothing is
written; every refusal of the two entry points is decided by host-side checks that come before the first device call, which run
here without a device through the g++-built harnesses; api.Landmarks carries the two methods and nothing was added to api.Problem
or api.Batch."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import landmark_fusion_reference as lf
import landmark_register_reference as lr
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_landmarks_eval_register", "sba_landmarks_register")


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
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [10, 9]
    # the records match the header's structs
    assert C.sizeof(cabi.LandmarkRegisterOptions) == 24 + C.sizeof(cabi.LmOptions)
    assert C.sizeof(cabi.LandmarkRegisterResult) == 8 * (3 + 3 + 36) + C.sizeof(cabi.LmSummary) + 8 * 6
    assert C.sizeof(cabi.LandmarkRegisterEval) == 8 * (36 + 6 + 1 + 2)
    for rec, name in ((cabi.LandmarkRegisterOptions, "sba_landmark_register_options"), (cabi.LandmarkRegisterResult, "sba_landmark_register_result"),
                      (cabi.LandmarkRegisterEval, "sba_landmark_register_eval")):
        assert _struct_fields(header, name) == [f[0] for f in rec._fields_], name
    for method in ("eval_register", "register"):
        assert hasattr(api.Landmarks, method), method
        assert not hasattr(api.Problem, method) and not hasattr(api.Batch, method)
    assert not any("register" in n.lower() for n in dir(api.Problem) + dir(api.Batch))


def test_null_arguments_are_refused_without_a_device(lib):
    z3 = (C.c_double * 3)(0, 0, 1)
    rows = np.full(18, -7.0)
    dp = rows.ctypes.data_as(cabi._dp)
    opt = cabi.LandmarkRegisterOptions(0.0, float("inf"), 1, api.default_lm_options(huber_delta=0.0))
    res = cabi.LandmarkRegisterResult()
    res.n_obs = res.n_fused = -7
    ev = cabi.LandmarkRegisterEval()
    ev.n_used = -7
    calls = (
        lambda: lib.sba_landmarks_register(None, None, dp, 2, z3, z3, C.byref(opt), C.byref(res), dp),
        lambda: lib.sba_landmarks_eval_register(None, None, dp, 2, z3, z3, z3, z3, C.byref(opt), C.byref(ev)),
    )
    for k, call in enumerate(calls):
        assert call() == cabi.SBA_ERR_INVALID_ARG, k
        assert cabi.last_error(lib) != ""
    assert (rows == -7.0).all() and res.n_obs == -7 and res.n_fused == -7 and ev.n_used == -7
    assert list(z3) == [0.0, 0.0, 1.0]                                                          # nothing written


def test_every_refusal_is_decided_on_the_host():
    """The checks both entry points run before their first device call (csrc/sba_landmarks.cpp: register_check calls exactly these
    functions, and both entry points call it first), here without a device: each refusal the GPU test provokes through the handle
    is refused by them."""
    src = open(os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc", "sba_landmarks.cpp")).read()
    check = src[src.index("int register_check("):src.index("int register_freeze(")]
    assert "hip" not in check.replace("SBA_ERR_HIP", "")                                         # no device call in the checks
    order = [check.index(c) for c in ("null argument", "SBA_REFUSE_POISONED", "resect_weight_check_sigma", "landmark_check_gate",
                                      "landmark_check_index", "landmark_register_check_loss", "SBA_ERR_UNSUPPORTED", "finite3")]
    assert all(o >= 0 for o in order)
    for entry in ("int sba_landmarks_eval_register(", "int sba_landmarks_register("):
        body = src[src.index(entry):]
        body = body[body.index("{"):]
        assert 0 <= body.index("register_check(") < body.index("= sba_landmark_register_") < body.index("register_freeze("), entry
    freeze = src[src.index("int register_freeze("):src.index("int register_reduce_pass(")]
    assert freeze.index("hipSetDevice") < freeze.index("hipMalloc")                              # the first device call of both
    hf, hr = lf.harness(), lr.harness()
    assert hf.landmark_fusion_harness_check(1, -1e-3) == 0 and hf.landmark_fusion_harness_check(2, float("nan")) == 0
    assert hf.landmark_fusion_harness_check(2, 0.0) == 0 and hf.landmark_fusion_harness_check(2, float("inf")) == 1
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    for idx, n in (([0, 1, 1], 5), ([2, 1, 0], 5), ([0, 1, 5], 5), ([0, 1, 2], 2)):
        assert hf.landmark_fusion_harness_check_index(ip(idx), len(idx), n) == 0, idx
    assert hf.landmark_fusion_harness_check_index(None, 4, 5) == 0                               # dense with m != n
    chk = hr.landmark_register_harness_check_loss
    assert [chk(v) for v in (0.0, -0.0, 1.0, -1.0, 1e-300, float("inf"), float("nan"))] == [1, 1, 0, 0, 0, 0, 0]


def test_result_types():
    e = api.LandmarkRegisterEquations(H=np.eye(6), g=np.zeros(6), cost=1.0, n_used=5, n_behind=0)
    assert e.n_used == 5 and e.H.shape == (6, 6)
    r = api.LandmarkRegistration(rot=np.zeros(3), tran=np.zeros(3), cov=np.eye(6), summary=None, n_obs=10, n_skipped=1, n_behind=2,
                                 n_gated=3, n_fused=4, n_used=9, chi2=None)
    assert r.n_obs == r.n_skipped + r.n_behind + r.n_gated + r.n_fused and r.chi2 is None
