"""CPU: the descriptor-match entry points answer null or nonsense arguments with a negative code and a message before any
device call, and the header, the library's exports and the binding table carry them (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest

from helpers import declared_functions
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

NEW = ["sba_match_descriptors", "sba_match_descriptors_device", "sba_batch_match_descriptors", "sba_problem_upload_matches",
       "sba_batch_upload_matches"]


def test_declared_exported_and_bound():
    lib = cabi.load_library()
    declared = declared_functions()
    for name in NEW:
        assert name in declared and name in cabi.SIGNATURES and hasattr(lib, name), name
    assert lib.sba_abi_version() == 2


def _p(v=16):
    return C.c_void_p(v)


def test_invalid_arguments_fail_before_any_device_call():
    lib = cabi.load_library()
    n = C.c_size_t()
    f = C.c_float
    off_bad = (C.c_size_t * 3)(0, 5, 2)
    off_ok = (C.c_size_t * 3)(0, 2, 5)
    d_nan = (C.c_double * 1)(float("nan"))
    calls = {
        "match(null query)": lambda: lib.sba_match_descriptors(0, None, 5, _p(), 5, 64, 256, f(0.3), None, None, C.byref(n), None, None, None),
        "match(null train)": lambda: lib.sba_match_descriptors(0, _p(), 5, None, 5, 64, 256, f(0.3), None, None, C.byref(n), None, None, None),
        "match(null n_matched)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 64, 256, f(0.3), None, None, None, None, None, None),
        "match(dim 0)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 0, 256, f(0.3), None, None, C.byref(n), None, None, None),
        "match(dim 257)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 257, 2048, f(0.3), None, None, C.byref(n), None, None, None),
        "match(short stride)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 64, 252, f(0.3), None, None, C.byref(n), None, None, None),
        "match(odd stride)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 64, 258, f(0.3), None, None, C.byref(n), None, None, None),
        "match(ratio 0)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 64, 256, f(0.0), None, None, C.byref(n), None, None, None),
        "match(ratio nan)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 64, 256, f(float("nan")), None, None, C.byref(n), None, None, None),
        "match(ratio inf)": lambda: lib.sba_match_descriptors(0, _p(), 5, _p(), 5, 64, 256, f(float("inf")), None, None, C.byref(n), None, None, None),
        "match_device(null query)": lambda: lib.sba_match_descriptors_device(0, None, None, 5, _p(), 5, 64, 256, f(0.3), None, None, C.byref(n), None, None, None),
        "match_device(dim)": lambda: lib.sba_match_descriptors_device(0, None, _p(), 5, _p(), 5, -3, 256, f(0.3), None, None, C.byref(n), None, None, None),
        "match_device(null n_matched)": lambda: lib.sba_match_descriptors_device(0, None, _p(), 5, _p(), 5, 64, 256, f(0.3), None, None, None, None, None, None),
        "batch_match(num_pairs < 0)": lambda: lib.sba_batch_match_descriptors(0, _p(), off_ok, _p(), off_ok, -1, 64, 256, f(0.3), None, None, _p(), None, None, None),
        "batch_match(null offsets)": lambda: lib.sba_batch_match_descriptors(0, _p(), None, _p(), off_ok, 2, 64, 256, f(0.3), None, None, _p(), None, None, None),
        "batch_match(non-monotone)": lambda: lib.sba_batch_match_descriptors(0, _p(), off_bad, _p(), off_ok, 2, 64, 256, f(0.3), None, None, _p(), None, None, None),
        "batch_match(null query)": lambda: lib.sba_batch_match_descriptors(0, None, off_ok, _p(), off_ok, 2, 64, 256, f(0.3), None, None, _p(), None, None, None),
        "batch_match(stride)": lambda: lib.sba_batch_match_descriptors(0, _p(), off_ok, _p(), off_ok, 2, 64, 8, f(0.3), None, None, _p(), None, None, None),
        "batch_match(ratio)": lambda: lib.sba_batch_match_descriptors(0, _p(), off_ok, _p(), off_ok, 2, 64, 256, f(-1.0), None, None, _p(), None, None, None),
        "problem_upload_matches(null handle)": lambda: lib.sba_problem_upload_matches(None, _p(), 5, _p(), 5, 28, 128, 64, _p(), _p(), 64, 256, f(0.3), None, 0, C.byref(n), None, None),
        "batch_upload_matches(null handle)": lambda: lib.sba_batch_upload_matches(None, _p(), off_ok, _p(), off_ok, 2, 28, 128, 64, _p(), _p(), 64, 256, f(0.3), None, 0, _p(), None, None),
    }
    for name, call in calls.items():
        rc = call()
        assert rc == cabi.SBA_ERR_INVALID_ARG, (name, rc)
        msg = lib.sba_last_error()
        assert msg and len(msg) > 3, name


def _has_gpu():
    try:
        return api.device_count() > 0
    except api.SbaError:
        return False


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a box without a GPU")
def test_valid_arguments_fail_loudly_without_device():
    q = np.zeros((4, 64), np.float32)
    with pytest.raises(api.SbaError) as ei:
        api.match_descriptors(q, q)
    assert ei.value.code == cabi.SBA_ERR_NO_DEVICE and "no CPU path" in ei.value.message
    with pytest.raises(api.SbaError) as ei:
        api.batch_match_descriptors(q, [0, 2, 4], q, [0, 4, 4])
    assert ei.value.code == cabi.SBA_ERR_NO_DEVICE


def test_python_layer_rejects_bad_shapes():
    q = np.zeros((4, 64), np.float32)
    with pytest.raises(ValueError):
        api.match_descriptors(q, np.zeros((4, 32), np.float32))
    with pytest.raises(ValueError):
        api.match_descriptors(np.zeros(64, np.float32), q)
    with pytest.raises(ValueError):
        api.batch_match_descriptors(q, [0, 2, 9], q, [0, 1, 4])
    with pytest.raises(api.SbaError) as ei:
        api.match_descriptors(q, q, ratio=float("nan"))
    assert ei.value.code == cabi.SBA_ERR_INVALID_ARG


def test_padded_rows_pass_without_copy():
    from spherical_bundle_adjuster_amd.api import _descriptors
    wide = np.zeros((10, 71), np.float32)
    (a, b), dim, stride = _descriptors(wide[:, :64], wide[:5, :64])
    assert dim == 64 and stride == 71 * 4 and a.base is wide
