"""CPU: the four entry points of the batched structure (sba_batch_structure_joint, _joint_device, _order_stats, _keep_below) are
declared in include/sba_hip.h, exported by the library and bound in _cabi.SIGNATURES; the ABI version stays 2 (additions); with
a NULL handle every whole-call refusal comes back as SBA_ERR_INVALID_ARG with a message and with nothing written; the source
places those checks ahead of the first hipSetDevice; BatchJointStructure.pair(g) slices rows by the offsets."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_batch_structure_joint", "sba_batch_structure_joint_device", "sba_batch_structure_order_stats",
         "sba_batch_structure_keep_below")
_szp, _ip = C.POINTER(C.c_size_t), C.POINTER(C.c_int)
_head = [C.c_void_p, cabi._dp, cabi._dp, C.POINTER(cabi.LmOptions), C.c_double]       # handle, rot, tran, options, threshold
ARGS = {
    NAMES[0]: _head + [C.POINTER(cabi.JointCov), cabi._dp, cabi._dp, cabi._dp, _ip],
    NAMES[1]: _head + [C.POINTER(cabi.JointCov), C.c_void_p, C.c_void_p, C.c_void_p, _ip],
    NAMES[2]: _head + [_szp, C.c_int, cabi._dp, _ip],
    NAMES[3]: _head + [_szp, cabi._dp, cabi._dp, _szp, C.c_void_p, _ip],
}


@pytest.fixture(scope="module")
def lib():
    return cabi.load_library()


def test_declared_exported_and_bound(lib):
    header = open(os.path.join(ROOT, "include", "sba_hip.h")).read()
    assert re.search(r"^#define SBA_ABI_VERSION 2\b", header, flags=re.M)
    for name in NAMES:
        assert re.search(r"^int %s\(sba_batch\* b, const double\* rot, const double\* tran, const sba_lm_options\* opt,$" % name,
                         header, flags=re.M), name
        assert name in cabi.SIGNATURES and cabi.SIGNATURES[name][0] is C.c_int
        assert cabi.SIGNATURES[name][1] == ARGS[name], name
        assert getattr(lib, name) is not None
    assert lib.sba_abi_version() == 2 and cabi.ABI_VERSION == 2        # additions only
    for method in ("structure_joint", "structure_joint_into", "structure_order_stats", "structure_keep_below"):
        assert hasattr(api.Batch, method)
    assert hasattr(api, "BatchJointStructure")
    # the header says whose contract the per-pair failures follow, and names the two switches
    doc = header[header.index("/* sba_batch_structure_joint:"):header.index("int sba_batch_structure_joint(")]
    assert "the contract of sba_batch_solve_joint" in doc and "SBA_BATCH_DEVICE_COV" in doc and "SBA_BATCH_STRUCTURE_BPP" in doc


def _refused(lib, rc):
    assert rc == cabi.SBA_ERR_INVALID_ARG
    assert cabi.last_error(lib) != ""


class _Outputs:
    """Sentinel-filled outputs of every kind the four functions write."""
    def __init__(self):
        self.out = (cabi.JointCov * 1)()
        self.out[0].dim = -7
        self.xyz = (C.c_double * 3)(-7.0, -7.0, -7.0)
        self.cov = (C.c_double * 6)(*([-7.0] * 6))
        self.score = (C.c_double * 1)(-7.0)
        self.st = (C.c_int * 1)(-7)
        self.values = (C.c_double * 8)(*([-7.0] * 8))
        self.thr = (C.c_double * 1)(-7.0)
        self.kept = (C.c_size_t * 1)(7)
        self.idx = (C.c_longlong * 1)(-7)

    def untouched(self):
        return (self.out[0].dim == -7 and list(self.xyz) == [-7.0] * 3 and list(self.cov) == [-7.0] * 6 and self.score[0] == -7.0
                and self.st[0] == -7 and list(self.values) == [-7.0] * 8 and self.thr[0] == -7.0 and self.kept[0] == 7
                and self.idx[0] == -7)


def test_nonsense_arguments_are_refused_without_a_device(lib):
    """A NULL handle throughout: nothing here may reach a device."""
    z3 = (C.c_double * 3)(0, 0, 1)
    o = _Outputs()
    rank = (C.c_size_t * 1)(0)
    scale = (C.c_double * 1)(4.0)
    joint, device, stats, keep = (getattr(lib, n) for n in NAMES)
    idx = C.cast(o.idx, C.c_void_p)
    for f in (joint, device):
        dst = (o.xyz, o.cov, o.score) if f is joint else (None, None, None)
        _refused(lib, f(None, z3, z3, None, 0.0, o.out, *dst, o.st))
        _refused(lib, f(C.c_void_p(0), z3, z3, None, 0.0, o.out, *dst, o.st))
        _refused(lib, f(None, z3, z3, None, 0.0, None, None, None, None, None))          # a NULL out
        _refused(lib, f(None, None, None, None, 0.0, o.out, *dst, o.st))
        for bad in (-1e-300, -1.0, -math.inf, math.nan):
            _refused(lib, f(None, z3, z3, None, bad, o.out, *dst, o.st))
    _refused(lib, stats(None, z3, z3, None, 0.0, rank, 1, o.values, o.st))
    _refused(lib, stats(None, z3, z3, None, 0.0, None, 1, o.values, o.st))                # NULL ranks
    _refused(lib, stats(None, z3, z3, None, 0.0, rank, 1, None, o.st))                    # NULL values
    for bad in (0, -1, 9):
        _refused(lib, stats(None, z3, z3, None, 0.0, rank, bad, o.values, o.st))          # num_ranks outside 1 ... 8
    for bad in (-1.0, math.nan):
        _refused(lib, stats(None, z3, z3, None, bad, rank, 1, o.values, o.st))
    _refused(lib, keep(None, z3, z3, None, 0.0, rank, scale, o.thr, o.kept, idx, o.st))
    _refused(lib, keep(None, z3, z3, None, 0.0, None, scale, o.thr, o.kept, idx, o.st))   # NULL rank
    _refused(lib, keep(None, z3, z3, None, 0.0, rank, None, o.thr, o.kept, idx, o.st))    # NULL scale
    _refused(lib, keep(None, z3, z3, None, 0.0, rank, scale, None, o.kept, idx, o.st))    # NULL threshold
    _refused(lib, keep(None, z3, z3, None, 0.0, rank, scale, o.thr, None, idx, o.st))     # NULL n_kept
    for bad in (-1.0, math.nan):
        _refused(lib, keep(None, z3, z3, None, bad, rank, scale, o.thr, o.kept, idx, o.st))
    assert o.untouched()


def _body(src, name):
    body = src[src.index("int %s(" % name):]
    return body[:body.index("\n}\n")]


def test_the_refusals_come_before_the_first_device_call():
    """Every whole-call refusal is in the entry point's own text (or in check_call / check_ranks, which touch no device),
    ahead of its first HIP call (a live handle needs a device: tests/test_gpu_batch_structure.py sends them through one)."""
    src = open(os.path.join(ROOT, "spherical_bundle_adjuster_amd", "csrc", "sba_batch_structure.cpp")).read()
    helpers = src[:src.index('extern "C"')]
    for helper, needles in (("int check_call(", ("if (!b)", "!(min_sin2_parallax >= 0.0)", "joint_check(b, rot, tran)")),
                            ("int check_ranks(", (">= b->n[g]",))):
        text = helpers[helpers.index(helper):]
        text = text[:text.index("\n}\n")]
        assert "hip" not in text, helper
        for needle in needles:
            assert needle in text, (helper, needle)
    want = {
        NAMES[0]: ("check_call(b, rot, tran, min_sin2_parallax)", "if (!out)"),
        NAMES[1]: ("check_call(b, rot, tran, min_sin2_parallax)", "if (!out)", "!aligned16(xyz) || !aligned16(xyz_cov) || !aligned16(score)"),
        NAMES[2]: ("check_call(b, rot, tran, min_sin2_parallax)", "!ranks || !values", "num_ranks < 1 || num_ranks > sba::kSelectMaxRanks",
                   "check_ranks(b, ranks, num_ranks)"),
        NAMES[3]: ("check_call(b, rot, tran, min_sin2_parallax)", "!rank || !scale || !threshold || !n_kept", "check_ranks(b, rank, 1)",
                   "!std::isfinite(scale[g]) || scale[g] < 0.0"),
    }
    for name, needles in want.items():
        body = _body(src, name)
        first_hip = body.index("hipSetDevice")
        assert first_hip == min(m.start() for m in re.finditer(r"\bhip[A-Z]\w*\(", body)), name
        for needle in needles:
            assert 0 <= body.index(needle) < first_hip, (name, needle)


def _result(xyz=True):
    B = 3
    pose = api.BatchJointCovariance(np.stack([np.eye(6) * (g + 1) for g in range(B)]), None, cost=np.array([3.0, 3.0, 0.0]),
                                    sum_w=np.array([10.0, 5.0, 0.0]), n_used=np.array([11, 5, 0]), n_degenerate=np.array([1, 0, 0]),
                                    dim=np.array([5, 5, 5], dtype=np.int32), dof=np.array([6, 0, -5], dtype=np.int32),
                                    status=np.array([0, 0, cabi.SBA_ERR_NUMERIC], dtype=np.int32), offsets=np.array([0, 4, 6, 6]))
    X = np.arange(18, dtype=np.float64).reshape(6, 3) if xyz else None
    return api.BatchJointStructure(X, np.arange(36, dtype=np.float64).reshape(6, 6), None, pose)


def test_result_type_pair_slices_rows_by_the_offsets():
    r = _result()
    p0, p1, p2 = r.pair(0), r.pair(1), r.pair(2)
    assert all(isinstance(p, api.JointStructure) for p in (p0, p1, p2))
    assert np.array_equal(p0.xyz, r.xyz[0:4]) and np.array_equal(p1.xyz, r.xyz[4:6]) and p2.xyz.shape == (0, 3)      # an empty pair
    assert np.array_equal(p0.cov, r.cov[0:4]) and np.array_equal(p1.cov, r.cov[4:6]) and p2.cov.shape == (0, 6)
    assert p0.score is None and p1.score is None and p2.score is None                                                 # a None output
    assert np.array_equal(p1.pose.cov, 2 * np.eye(6)) and p1.pose.depth_cov is None
    assert (p0.cost, p0.sum_w, p0.n_used, p0.n_degenerate, p0.dim, p0.dof) == (3.0, 10.0, 11, 1, 5, 6)
    assert p0.sigma2 == 1.0 and math.isnan(p1.sigma2)
    # the batch's own pass-through
    assert np.array_equal(r.offsets, [0, 4, 6, 6]) and np.array_equal(r.status, [0, 0, cabi.SBA_ERR_NUMERIC])
    assert np.array_equal(r.n_used, [11, 5, 0]) and r.sigma2.shape == (3,) and r.sigma2[0] == 1.0
    with pytest.raises(AttributeError):
        r.nothing
    assert _result(xyz=False).pair(1).xyz is None
