"""CPU: the nine entry points of the landmark map are declared in include/sba_hip.h, exported by the library and bound in
_cabi.SIGNATURES; the ABI version stays 2 (additions); the two records match the header's structs; without a device create fails
loudly; a NULL handle or NULL arguments come back as SBA_ERR_INVALID_ARG with a message before any device is touched and nothing
is written; every option and idx refusal of sba_landmarks_fuse is decided by the host-side checks of csrc/sba_landmarks.hpp, which
run here without a device through the g++-built harness; api.Landmarks carries the methods."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import landmark_fusion_reference as lf
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_landmarks_create", "sba_landmarks_destroy", "sba_landmarks_size", "sba_landmarks_set", "sba_landmarks_set_device",
         "sba_landmarks_get", "sba_landmarks_get_device", "sba_landmarks_counts", "sba_landmarks_fuse")


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def _has_gpu():
    try:
        return api.device_count() > 0
    except api.SbaError:
        return False


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [3, 1, 2, 5, 5, 3, 3, 2, 9]
    # the records match the header's structs
    assert C.sizeof(cabi.LandmarkFuseOptions) == 32 and C.sizeof(cabi.LandmarkFuseResult) == 40
    body = header[header.index("typedef struct sba_landmark_fuse_options"):header.index("} sba_landmark_fuse_options;")]
    assert re.findall(r"\b(bearing_sigma|chi2_gate|pose_cov|apply)\b(?=;)", body) == [f[0] for f in cabi.LandmarkFuseOptions._fields_]
    body = header[header.index("typedef struct sba_landmark_fuse_result"):header.index("} sba_landmark_fuse_result;")]
    assert re.findall(r"\b(n_obs|n_skipped|n_behind|n_gated|n_fused)\b(?=[;,])", body) == [f[0] for f in cabi.LandmarkFuseResult._fields_]
    for method in ("close", "set", "set_device", "size", "get", "get_device", "counts", "fuse", "__enter__", "__exit__"):
        assert hasattr(api.Landmarks, method), method
    # nothing was added to the two existing handle classes for this
    assert not any("landmarks" in n.lower() and n not in ("upload_landmarks",) for n in dir(api.Batch))
    assert not hasattr(api.Problem, "fuse") and not hasattr(api.Batch, "fuse")


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a box without a GPU")
def test_create_fails_loudly_without_a_device():
    with pytest.raises(api.SbaError) as ei:
        api.Landmarks(0)
    assert ei.value.code == cabi.SBA_ERR_NO_DEVICE and "no CPU path" in ei.value.message


def test_null_arguments_are_refused_without_a_device(lib):
    z3 = (C.c_double * 3)(0, 0, 1)
    rows = np.full(18, -7.0)
    dp = rows.ctypes.data_as(cabi._dp)
    n = C.c_size_t(77)
    cnt = np.full(4, 77, dtype=np.uint32)
    opt = cabi.LandmarkFuseOptions(0.0, float("inf"), None, 1)
    res = cabi.LandmarkFuseResult(-7, -7, -7, -7, -7)
    calls = (
        lambda: lib.sba_landmarks_create(None, 0, None),
        lambda: lib.sba_landmarks_size(None, C.byref(n)),
        lambda: lib.sba_landmarks_set(None, dp, dp, 2, 1.0),
        lambda: lib.sba_landmarks_set_device(None, C.c_void_p(16), C.c_void_p(32), 2, 1.0),
        lambda: lib.sba_landmarks_get(None, dp, dp),
        lambda: lib.sba_landmarks_get_device(None, C.c_void_p(16), C.c_void_p(32)),
        lambda: lib.sba_landmarks_counts(None, cnt.ctypes.data_as(C.POINTER(C.c_uint32))),
        lambda: lib.sba_landmarks_fuse(None, None, dp, 2, z3, z3, C.byref(opt), C.byref(res), dp),
    )
    for k, call in enumerate(calls):
        assert call() == cabi.SBA_ERR_INVALID_ARG, k
        assert cabi.last_error(lib) != ""
    assert lib.sba_landmarks_destroy(None) == cabi.SBA_OK                                        # a no-op, as for the other handles
    assert n.value == 77 and (cnt == 77).all() and (rows == -7.0).all() and res.n_obs == -7 and res.n_fused == -7
    assert list(z3) == [0.0, 0.0, 1.0]                                                          # nothing written


def test_every_fuse_refusal_is_decided_on_the_host():
    """The checks sba_landmarks_fuse runs before its first device call (csrc/sba_landmarks.cpp calls exactly these functions), here
    without a device: each refusal the GPU test provokes through the handle is refused by them."""
    h = lf.harness()
    src = open(os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc", "sba_landmarks.cpp")).read()
    fuse = src[src.index("int sba_landmarks_fuse("):]
    first_device_call = fuse.index("hipSetDevice")
    for check in ("resect_weight_check_sigma", "landmark_check_gate", "landmark_check_pose_cov", "landmark_check_index", "SBA_REFUSE_POISONED"):
        assert 0 <= fuse.index(check) < first_device_call, check
    assert "resect_weight_check_scale" in src[:src.index("int sba_landmarks_create(")]
    assert h.landmark_fusion_harness_check(1, -1e-3) == 0 and h.landmark_fusion_harness_check(2, float("nan")) == 0
    assert h.landmark_fusion_harness_check(2, 0.0) == 0 and h.landmark_fusion_harness_check(2, float("inf")) == 1
    bad = lf.POSE_COV_FULL.copy()
    bad[0, 1] = np.nextafter(bad[0, 1], 1.0)
    assert h.landmark_fusion_harness_check_pose_cov(bad.ctypes.data_as(cabi._dp)) == 0
    ip = lambda a: np.ascontiguousarray(a, dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    for idx, n in (([0, 1, 1], 5), ([2, 1, 0], 5), ([0, 1, 5], 5), ([0, 1, 2], 2)):
        assert h.landmark_fusion_harness_check_index(ip(idx), len(idx), n) == 0, idx


def test_result_type():
    f = api.LandmarkFusion(n_obs=10, n_skipped=1, n_behind=2, n_gated=3, n_fused=4, chi2=None)
    assert f.n_obs == f.n_skipped + f.n_behind + f.n_gated + f.n_fused and f.chi2 is None
