"""CPU: the six entry points that edit the landmark map are declared in include/sba_hip.h, exported by the library and bound in
_cabi.SIGNATURES; the ABI version stays 2 (additions); the two records match the header's structs; a NULL handle, a NULL required
pointer and a bad option come back as SBA_ERR_INVALID_ARG with a message before any device is touched and nothing is written; in the
source every check of every entry point stands before its first hipSetDevice; api.Landmarks carries the methods and the two other
handle classes gained nothing."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_landmarks_scores", "sba_landmarks_prune", "sba_landmarks_append", "sba_landmarks_append_device", "sba_landmarks_gather",
         "sba_landmarks_gather_device")
METHODS = ("scores", "prune", "append", "append_device", "gather", "gather_device")


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
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [2, 4, 5, 5, 6, 5]
    # the records match the header's structs
    assert C.sizeof(cabi.LandmarkPruneOptions) == 32 and C.sizeof(cabi.LandmarkPruneResult) == 48
    body = header[header.index("typedef struct sba_landmark_prune_options"):header.index("} sba_landmark_prune_options;")]
    assert re.findall(r"\b(max_score|min_count|mask|apply)\b(?=;)", body) == [f[0] for f in cabi.LandmarkPruneOptions._fields_]
    assert [f[1] for f in cabi.LandmarkPruneOptions._fields_] == [C.c_double, C.c_uint32, C.POINTER(C.c_uint8), C.c_int]
    body = header[header.index("typedef struct sba_landmark_prune_result"):header.index("} sba_landmark_prune_result;")]
    assert re.findall(r"\b(n_before|n_invalid|n_uncertain|n_unobserved|n_masked|n_kept)\b(?=[;,])", body) == \
        [f[0] for f in cabi.LandmarkPruneResult._fields_]


def test_the_methods_are_on_the_map_handle_alone():
    for method in METHODS:
        assert hasattr(api.Landmarks, method), method
        assert not hasattr(api.Problem, method) and not hasattr(api.Batch, method), method
    # the two other handle classes gained nothing: tests/handle_ops.py, unchanged, still accounts for every public name they have
    import handle_ops as ops
    for cls, table, excluded in ((api.Problem, ops.PROBLEM_OPS, ops.PROBLEM_EXCLUDED), (api.Batch, ops.BATCH_OPS, ops.BATCH_EXCLUDED)):
        assert set(ops.public_names(cls)) == {m for op in table for m in op.methods} | set(excluded), cls.__name__
    f = api.LandmarkPrune(n_before=10, n_invalid=1, n_uncertain=2, n_unobserved=3, n_masked=0, n_kept=4, kept=None)
    assert f.n_before == f.n_invalid + f.n_uncertain + f.n_unobserved + f.n_masked + f.n_kept and f.kept is None


def test_null_arguments_and_bad_options_are_refused_without_a_device(lib):
    rows = np.full(18, -7.0)
    dp = rows.ctypes.data_as(cabi._dp)
    cnt = np.full(4, 77, dtype=np.uint32)
    kept = np.full(4, -7, dtype=np.int64)
    idx = np.array([0, 1], dtype=np.int64)
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int64))
    opt = cabi.LandmarkPruneOptions(float("inf"), 0, None, 1)
    res = cabi.LandmarkPruneResult(-7, -7, -7, -7, -7, -7)
    fake = C.c_void_p(4096)                                              # never dereferenced: the NULL checks come first
    calls = (
        lambda: lib.sba_landmarks_scores(None, dp),
        lambda: lib.sba_landmarks_prune(None, C.byref(opt), C.byref(res), ip(kept)),
        lambda: lib.sba_landmarks_prune(fake, None, C.byref(res), ip(kept)),
        lambda: lib.sba_landmarks_prune(fake, C.byref(opt), None, ip(kept)),
        lambda: lib.sba_landmarks_append(None, dp, dp, 2, 1.0),
        lambda: lib.sba_landmarks_append_device(None, C.c_void_p(16), C.c_void_p(32), 2, 1.0),
        lambda: lib.sba_landmarks_gather(None, ip(idx), 2, dp, dp, cnt.ctypes.data_as(C.POINTER(C.c_uint32))),
        lambda: lib.sba_landmarks_gather_device(None, ip(idx), 2, C.c_void_p(16), C.c_void_p(32)),
    )
    for k, call in enumerate(calls):
        assert call() == cabi.SBA_ERR_INVALID_ARG, k
        assert cabi.last_error(lib) != ""
    assert (cnt == 77).all() and (rows == -7.0).all() and (kept == -7).all() and res.n_before == -7 and res.n_kept == -7   # nothing written


def _body(src, start):
    """The text of the function that begins at `start`, up to the next function at column 0."""
    at = src.index(start)
    end = re.search(r"^}\n", src[at:], flags=re.M)
    return src[at:at + end.end()]


def test_every_check_stands_before_the_first_device_call():
    """Source order: each entry point refuses -- the checks of csrc/sba_landmarks_edit.hpp and the shared ones, which run without a
    device through the harness in tests/test_landmark_edit_host_cpu.py -- before its first hipSetDevice."""
    src = open(os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc", "sba_landmarks.cpp")).read()
    edits = src[src.index("int sba_landmarks_fuse("):]
    wanted = {
        "int sba_landmarks_scores(": ("null landmark handle", "SBA_REFUSE_POISONED", "null output array"),
        "int sba_landmarks_prune(": ("null argument", "SBA_REFUSE_POISONED", "landmark_check_max_score"),
        "int append_common(": ("null landmark handle", "SBA_REFUSE_POISONED", "null landmark or covariance array", "16-byte aligned",
                               "resect_weight_check_scale", "landmark_check_sizes"),
        "int gather_common(": ("null landmark handle", "SBA_REFUSE_POISONED", "16-byte aligned", "landmark_check_sizes",
                               "landmark_check_gather_index"),
    }
    for start, checks in wanted.items():
        body = _body(edits, start)
        first_device_call = min(body.index(call) for call in ("hipSetDevice", "hipMalloc", "hipMemcpyAsync", "launch_") if call in body)
        assert first_device_call == body.index("hipSetDevice"), start
        for check in checks:
            assert 0 <= body.index(check) < first_device_call, (start, check)
        assert body.count("hipSetDevice") == 1 and "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body, start
        assert "stream_wait" in body, start                                  # every wait is the bounded one
    for name, common in (("sba_landmarks_append", "append_common"), ("sba_landmarks_append_device", "append_common"),
                         ("sba_landmarks_gather", "gather_common"), ("sba_landmarks_gather_device", "gather_common")):
        body = _body(edits, "int %s(" % name)
        assert "return %s(" % common in body and "hip" not in body.split("{", 1)[1], name
    assert "getenv" not in edits.replace(_body(edits, "int sba_landmarks_fuse("), "")      # no new environment switch
