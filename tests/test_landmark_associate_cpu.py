"""CPU: the landmark map's descriptors and the association of a frame without a device.  The vectorised
reference of tests/landmark_associate_reference.py equals a plain loop on every case and every case of its table is non-trivial with
the counts the table states; the ten entry points are declared in include/sba_hip.h, exported and bound in _cabi.SIGNATURES with
ABI version 2 and records that match the header's structs; every refusal comes back before any device is touched with a message and
nothing written; in the source every check stands before the first device call, every wait is the bounded one and no environment
switch was added; the methods are on api.Landmarks alone; and the host header's key, order and checks run through a g++-built
harness and, with exact-sized heap buffers, in a stand-alone program under ASan and UBSan."""
import ctypes as C
import re
import subprocess

import numpy as np
import pytest

import landmark_associate_reference as la
import match_cases as mc
from helpers import ROOT
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

NAMES = ("sba_landmarks_set_descriptors", "sba_landmarks_set_descriptors_device", "sba_landmarks_descriptor_dim",
         "sba_landmarks_get_descriptors", "sba_landmarks_append_described", "sba_landmarks_append_described_device",
         "sba_landmarks_associate", "sba_landmarks_associate_device")
METHODS = ("set_descriptors", "set_descriptors_device", "descriptor_dim", "get_descriptors", "append_described", "append_described_device",
           "associate", "associate_device")
CSRC = ROOT / "spherical_bundle_adjuster_amd" / "csrc"


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


# ---- the reference and its table ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(la.CASES)))
def test_the_vectorised_reference_equals_the_loop_and_the_table(k):
    c = la.CASES[k]
    frame, desc = la.arrays(k)
    assert frame.shape == (c.m, c.D) and desc.shape == (c.n, c.D)
    mc.assert_exact_domain(frame, desc)
    for ratio in la.RATIOS:
        for cut in (np.inf, 1.0):
            a, b = la.associate(frame, desc, ratio, cut), la.associate_loop(frame, desc, ratio, cut)
            assert all(np.array_equal(x, y) for x, y in zip(a, b)), (k, ratio, cut)
            assert a.idx.dtype == np.int64 and a.rows.dtype == np.int32 and a.distance.dtype == np.float32
            assert (np.diff(a.idx) > 0).all() and len(set(a.rows.tolist())) == a.n_associated and a.n_accepted == a.n_contested + a.n_associated
        a = la.expected(k, ratio)
        assert (a.n_accepted, a.n_associated, a.n_contested) == c.counts[ratio], (k, ratio)
        # non-trivial: landmarks are contested, equal distances among the claimants of one landmark occur, both planted distances occur
        assert a.n_contested > 0 and 0 < a.n_associated <= min(c.m, c.n)
        j, i, d = la.accepted(frame, desc, ratio)
        assert {1.0, float(np.sqrt(np.float32(2.0)))} <= set(np.unique(d).tolist())
        ties = sum(1 for lm in np.unique(i) if (d[i == lm] == d[i == lm].min()).sum() > 1)
        assert ties > 0, (k, ratio)
        cut = la.expected(k, ratio, 1.0)
        assert 0 < cut.n_accepted < a.n_accepted and (cut.distance == 1.0).all()


def test_the_reference_on_small_hand_cases():
    t = np.zeros((4, 3), dtype=np.float32)
    t[:, 0] = (0.0, 10.0, 20.0, 30.0)
    f = np.array([[1, 0, 0], [11, 0, 0], [0, 1, 0], [10, -1, 0], [21, 1, 0], [500, 0, 0]], dtype=np.float32)
    a = la.associate(f, t, 0.3)
    # rows 0 and 2 claim landmark 0 at distance 1: the lower row wins; rows 1 and 3 claim landmark 1; row 4 sits at sqrt 2; row 5 fails the ratio
    assert (a.n_frame, a.n_accepted, a.n_contested, a.n_associated) == (6, 5, 2, 3)
    assert a.idx.tolist() == [0, 1, 2] and a.rows.tolist() == [0, 1, 4] and a.distance.tolist() == [1.0, 1.0, float(np.sqrt(np.float32(2.0)))]
    cut = la.associate(f, t, 0.3, 1.0)
    assert (cut.n_accepted, cut.n_associated) == (4, 2) and cut.idx.tolist() == [0, 1]
    f[0, 1] = np.nan                                                   # the winner of landmark 0 drops out: row 2 takes it
    assert la.associate(f, t, 0.3).rows.tolist() == [2, 1, 4]
    assert la.associate(f, t[:1], 0.3).n_accepted == 0 and la.associate(f[:0], t, 0.3).n_frame == 0       # one train row: nothing matches
    assert int(la.keys(np.float32([1.0]), [7])[0]) == (0x3f800000 << 32) | 7


# ---- the C-ABI ---------------------------------------------------------------------------------------------------------------------
def test_declared_exported_and_bound(lib):
    header = (ROOT / "include" / "sba_hip.h").read_text()
    for name in NAMES:
        assert re.search(r"^int %s\(" % name, header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [5, 5, 2, 5, 8, 8, 12, 12]
    assert C.sizeof(cabi.LandmarkAssociateOptions) == 8 and C.sizeof(cabi.LandmarkAssociateResult) == 32
    body = header[header.index("typedef struct sba_landmark_associate_options"):header.index("} sba_landmark_associate_options;")]
    assert re.findall(r"\b(ratio|max_distance)\b(?=;)", body) == [f[0] for f in cabi.LandmarkAssociateOptions._fields_]
    assert [f[1] for f in cabi.LandmarkAssociateOptions._fields_] == [C.c_float, C.c_float]
    body = header[header.index("typedef struct sba_landmark_associate_result"):header.index("} sba_landmark_associate_result;")]
    assert re.findall(r"\b(n_frame|n_accepted|n_contested|n_associated)\b(?=[;,])", body) == [f[0] for f in cabi.LandmarkAssociateResult._fields_]


def test_the_methods_are_on_the_map_handle_alone():
    for method in METHODS:
        assert hasattr(api.Landmarks, method), method
        assert not hasattr(api.Problem, method) and not hasattr(api.Batch, method), method
    import handle_ops as ops
    for cls, table, excluded in ((api.Problem, ops.PROBLEM_OPS, ops.PROBLEM_EXCLUDED), (api.Batch, ops.BATCH_OPS, ops.BATCH_EXCLUDED)):
        assert set(ops.public_names(cls)) == {m for op in table for m in op.methods} | set(excluded), cls.__name__
    a = api.LandmarkAssociation(9, 5, 2, 3, np.arange(3), np.arange(3, dtype=np.int32), np.ones(3, dtype=np.float32), None)
    assert a.n_accepted == a.n_contested + a.n_associated and a.bearings is None


def test_refusals_come_back_without_a_device(lib):
    desc = np.full((4, 8), -7.0, dtype=np.float32)
    rows = np.full(18, -7.0)
    out_i, out_r, out_d, out_b = np.full(4, -7, dtype=np.int64), np.full(4, -7, dtype=np.int32), np.full(4, -7.0, dtype=np.float32), np.full(12, -7.0)
    dim = C.c_int(-7)
    opt = cabi.LandmarkAssociateOptions(0.3, float("inf"))
    res = cabi.LandmarkAssociateResult(-7, -7, -7, -7)
    vp, dp = C.c_void_p(desc.ctypes.data), rows.ctypes.data_as(cabi._dp)
    outs = (out_i.ctypes.data_as(C.POINTER(C.c_int64)), out_r.ctypes.data_as(C.POINTER(C.c_int32)), out_d.ctypes.data_as(C.POINTER(C.c_float)),
            out_b.ctypes.data_as(cabi._dp))
    dev_outs = outs[:3] + (C.c_void_p(64),)
    fake = C.c_void_p(4096)                                              # never dereferenced: the NULL checks come first
    idx = np.array([0, 1], dtype=np.int64).ctypes.data_as(C.POINTER(C.c_int64))
    calls = (
        lambda: lib.sba_landmarks_set_descriptors(None, vp, 4, 8, 32),
        lambda: lib.sba_landmarks_set_descriptors_device(None, C.c_void_p(64), 4, 8, 32),
        lambda: lib.sba_landmarks_descriptor_dim(None, C.byref(dim)),
        lambda: lib.sba_landmarks_descriptor_dim(fake, None),
        lambda: lib.sba_landmarks_get_descriptors(None, idx, 2, vp, 32),
        lambda: lib.sba_landmarks_append_described(None, dp, dp, vp, 2, 8, 32, 1.0),
        lambda: lib.sba_landmarks_append_described_device(None, C.c_void_p(16), C.c_void_p(32), C.c_void_p(64), 2, 8, 32, 1.0),
        lambda: lib.sba_landmarks_associate(None, vp, 4, 8, 32, dp, C.byref(opt), C.byref(res), *outs),
        lambda: lib.sba_landmarks_associate(fake, vp, 4, 8, 32, dp, None, C.byref(res), *outs),
        lambda: lib.sba_landmarks_associate(fake, vp, 4, 8, 32, dp, C.byref(opt), None, *outs),
        lambda: lib.sba_landmarks_associate(fake, None, 4, 8, 32, dp, C.byref(opt), C.byref(res), *outs),
        lambda: lib.sba_landmarks_associate_device(None, C.c_void_p(64), 4, 8, 32, C.c_void_p(128), C.byref(opt), C.byref(res), *dev_outs),
        lambda: lib.sba_landmarks_associate_device(fake, C.c_void_p(64), 4, 8, 32, C.c_void_p(128), None, C.byref(res), *dev_outs),
        lambda: lib.sba_landmarks_associate_device(fake, None, 4, 8, 32, C.c_void_p(128), C.byref(opt), C.byref(res), *dev_outs),
    )
    for k, call in enumerate(calls):
        assert call() == cabi.SBA_ERR_INVALID_ARG, k
        assert cabi.last_error(lib) != ""
    assert (out_i == -7).all() and (out_r == -7).all() and (out_d == -7.0).all() and (out_b == -7.0).all() and (desc == -7.0).all() and (rows == -7.0).all()
    assert dim.value == -7 and (res.n_frame, res.n_accepted, res.n_contested, res.n_associated) == (-7, -7, -7, -7)      # nothing written


def _body(src, start):
    """The text of the function that begins at `start`, up to the next function at column 0."""
    at = src.index(start)
    end = re.search(r"^}\n", src[at:], flags=re.M)
    return src[at:at + end.end()]


def test_every_check_stands_before_the_first_device_call():
    """Source order in csrc/sba_landmarks.cpp: each body refuses before its first hipSetDevice, holds one hipSetDevice, waits only
    through stream_wait, and the public wrappers hold nothing but their return."""
    src = (CSRC / "sba_landmarks.cpp").read_text()
    part = src[src.index("// ---- the descriptors:"):]
    wanted = {
        "int set_descriptors_common(": ("null landmark handle", "SBA_REFUSE_POISONED", "descriptor_check_rows", "one descriptor row per landmark",
                                        "null descriptor array", "4-byte aligned"),
        "int associate_common(": ("null argument", "SBA_REFUSE_POISONED", "associate_check_options", "keeps no descriptors",
                                  "keeps descriptors of dimension", "descriptor_check_rows", "associate_check_sizes", "16-byte aligned"),
        "int sba_landmarks_get_descriptors(": ("null landmark handle", "SBA_REFUSE_POISONED", "keeps no descriptors", "descriptor_check_rows",
                                               "landmark_check_gather_index", "null output array"),
    }
    device_calls = ("hipSetDevice", "hipMalloc", "hipMemcpyAsync", "hipMemcpy2DAsync", "hipMemsetAsync", "launch_", "grow_scratch", "alt_desc(",
                    "pack_desc_rows(", "associate_scratch(", "match_pair_on_stream")
    for start, checks in wanted.items():
        body = _body(part, start)
        first_device_call = min(body.index(call) for call in device_calls if call in body)
        assert first_device_call == body.index("hipSetDevice"), start
        for check in checks:
            assert 0 <= body.index(check) < first_device_call, (start, check)
        assert body.count("hipSetDevice") == 1 and "hipStreamSynchronize" not in body and "hipDeviceSynchronize" not in body, start
        assert "stream_wait" in body, start                                  # every wait is the bounded one
    # an association waits twice: the matcher's count (inside match_pair_on_stream) and the associated count
    body = _body(part, "int associate_common(")
    assert body.count("stream_wait(") == 1 and body.count("match_pair_on_stream(") == 1
    assert body.index("match_pair_on_stream(") < body.index("launch_landmarks_claim") < body.index("stream_wait(")
    for name, common in (("sba_landmarks_set_descriptors", "set_descriptors_common"), ("sba_landmarks_set_descriptors_device", "set_descriptors_common"),
                         ("sba_landmarks_append_described", "append_common"), ("sba_landmarks_append_described_device", "append_common"),
                         ("sba_landmarks_associate", "associate_common"), ("sba_landmarks_associate_device", "associate_common")):
        body = _body(part, "int %s(" % name)
        assert "return %s(" % common in body and "hip" not in body.split("{", 1)[1], name
    # the described append's checks stand with append_common's own, before its hipSetDevice
    body = _body(src, "int append_common(")
    for check in ("descriptor_check_rows", "null descriptor array", "4-byte aligned", "keeps descriptors of dimension"):
        assert 0 <= body.index(check) < body.index("hipSetDevice"), check
    # no environment switch: the one getenv of the file is grid_for's
    assert src.count("getenv") == 1 and "getenv" not in part
    for f in ("sba_landmarks_associate.hip", "sba_landmarks_associate.hpp"):
        text = (CSRC / f).read_text()
        assert "getenv" not in text and "hipStreamSynchronize" not in text and "hipDeviceSynchronize" not in text, f
    # integer atomics only, no floating-point reduction: the kernels' atomics are a 64-bit minimum and a count
    kernels = (CSRC / "sba_landmarks_associate.hip").read_text()
    assert set(re.findall(r"\batomic[A-Z]\w*", kernels)) == {"atomicMin", "atomicAdd"}
    assert re.search(r"atomicAdd\(&counters\[0\], accepted\)", kernels) and "unsigned long long accepted" in kernels
    assert "sba_landmarks_associate.hip" in (CSRC / "Makefile").read_text()


# ---- the host header through a harness ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    so = tmp_path_factory.mktemp("landmark_associate") / "liblandmark_associate_harness.so"
    src = ROOT / "tests" / "harness" / "landmark_associate_harness.cpp"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-ffp-contract=off", "-o", str(so), str(src)], check=True)
    h = C.CDLL(str(so))
    u64 = C.c_ulonglong
    h.landmark_associate_harness_key.argtypes, h.landmark_associate_harness_key.restype = [C.c_float, C.c_uint], u64
    h.landmark_associate_harness_key_row.argtypes, h.landmark_associate_harness_key_row.restype = [u64], C.c_uint
    h.landmark_associate_harness_key_distance.argtypes, h.landmark_associate_harness_key_distance.restype = [u64], C.c_float
    h.landmark_associate_harness_key_before.argtypes = [u64, u64]
    h.landmark_associate_harness_unclaimed.restype = u64
    h.landmark_associate_harness_claim.argtypes = [C.c_size_t, C.c_size_t, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_float), C.c_float,
                                                   C.POINTER(u64)]
    h.landmark_associate_harness_claim.restype = C.c_longlong
    h.landmark_associate_harness_check_options.argtypes = [C.c_float, C.c_float]
    h.landmark_associate_harness_check_rows.argtypes = [C.c_int, C.c_size_t]
    h.landmark_associate_harness_check_sizes.argtypes = [C.c_size_t, C.c_size_t]
    return h


def test_the_header_key_is_the_reference_key(harness):
    d = np.array([0.0, 1.0, np.sqrt(np.float32(2.0)), 3.5, 1e-40, 3e38, np.inf], dtype=np.float32)
    rows = np.array([0, 1, 255, 256, 65537, 2**31 - 1], dtype=np.uint32)
    for x in d:
        for r in rows:
            key = harness.landmark_associate_harness_key(float(x), int(r))
            assert key == int(la.keys(np.float32([x]), [r])[0])
            assert harness.landmark_associate_harness_key_row(key) == int(r)
            assert np.float32(harness.landmark_associate_harness_key_distance(key)).tobytes() == np.float32(x).tobytes()
    ks = sorted(int(la.keys(np.float32([x]), [r])[0]) for x in d for r in rows)
    assert all(harness.landmark_associate_harness_key_before(a, b) == 1 and harness.landmark_associate_harness_key_before(b, a) == 0
               for a, b in zip(ks, ks[1:]))
    assert harness.landmark_associate_harness_unclaimed() == 2**64 - 1 > ks[-1]


@pytest.mark.parametrize("k", range(len(la.CASES)))
def test_the_header_claim_gives_the_reference_winners(harness, k):
    """The header's key, order and cut over the matcher-accepted rows of a case, fed in ascending, descending and shuffled order."""
    frame, desc = la.arrays(k)
    n = len(desc)
    for ratio, cut in ((0.3, np.inf), (0.5, 1.0)):
        j, i, d = la.accepted(frame, desc, ratio)                       # before the distance cut: the header applies it
        ref = la.associate(frame, desc, ratio, cut)
        for order in (np.arange(len(j)), np.arange(len(j))[::-1], np.random.default_rng(k).permutation(len(j))):
            jj, ii, dd = (np.ascontiguousarray(a[order]) for a in (j.astype(np.int32), i.astype(np.int32), d))
            slots = np.zeros(n, dtype=np.uint64)
            acc = harness.landmark_associate_harness_claim(n, len(jj), jj.ctypes.data_as(C.POINTER(C.c_int)), ii.ctypes.data_as(C.POINTER(C.c_int)),
                                                           dd.ctypes.data_as(C.POINTER(C.c_float)), float(cut), slots.ctypes.data_as(C.POINTER(C.c_ulonglong)))
            claimed = np.flatnonzero(slots != np.uint64(2**64 - 1))
            assert acc == ref.n_accepted and np.array_equal(claimed, ref.idx)
            assert np.array_equal((slots[claimed] & np.uint64(0xffffffff)).astype(np.int32), ref.rows)
            assert np.array_equal((slots[claimed] >> np.uint64(32)).astype(np.uint32).view(np.float32), ref.distance)


def test_the_header_checks(harness):
    co, cr, cs = harness.landmark_associate_harness_check_options, harness.landmark_associate_harness_check_rows, harness.landmark_associate_harness_check_sizes
    inf, nan = float("inf"), float("nan")
    assert [co(0.3, inf), co(1e-30, 1e-30), co(1.5, 1.0)] == [1, 1, 1]
    assert [co(0.0, inf), co(-0.3, inf), co(inf, inf), co(nan, inf), co(0.3, 0.0), co(0.3, -1.0), co(0.3, -inf), co(0.3, nan)] == [0] * 8
    assert [cr(1, 4), cr(256, 1024), cr(36, 148), cr(5, 4096)] == [1] * 4
    assert [cr(0, 4), cr(-1, 4), cr(257, 2048), cr(36, 140), cr(36, 146), cr(1, 0)] == [0] * 6
    assert [cs(0, 0), cs(2**31 - 1, 2**31 - 1), cs(2**31, 1), cs(1, 2**31), cs(2**64 - 1, 2**64 - 1)] == [1, 1, 0, 0, 0]


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "landmark_associate_sanitize_main"
    src = ROOT / "tests" / "harness" / "landmark_associate_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "landmark associate host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
