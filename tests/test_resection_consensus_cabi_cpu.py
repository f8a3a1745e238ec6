"""CPU: the two entry points of the robust resection guess (sba_problem_score_resection,
sba_problem_resection_guess_consensus) are declared in include/sba_hip.h, exported by the library and bound in
_cabi.SIGNATURES; the ABI version stays 2 (additions); the two records have the header's layout; NULL arguments come back as a
negative status with a message before any device is touched and nothing is written; Problem carries the methods; without a
device the handle itself fails loudly.  (The refusals that need a handle -- its state, out-of-range values, non-finite
candidates, too few matches, no finishing trial -- are in tests/test_gpu_resection_consensus.py: a handle needs a device.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("sba_problem_score_resection", "sba_problem_resection_guess_consensus")


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
    assert [len(cabi.SIGNATURES[n][1]) for n in NAMES] == [6, 8]
    # options: two ints, a 64-bit seed, a double, an int (padded to 8); info: five 64-bit counts, an int (padded), the guess
    # record of sba_problem_resection_guess, a double
    assert C.sizeof(cabi.ResectionConsensusOptions) == 32
    assert C.sizeof(cabi.ResectionConsensusInfo) == 5 * 8 + 8 + C.sizeof(cabi.ResectionGuessInfo) + 8 == 128
    assert cabi.ResectionConsensusInfo.refit.offset == 48 and cabi.ResectionConsensusInfo.n_behind.offset == 120
    assert [f[0] for f in cabi.ResectionConsensusOptions._fields_] == ["trials", "sample_size", "seed", "threshold", "refit"]
    opts = header[header.index("typedef struct sba_resection_consensus_options"):header.index("} sba_resection_consensus_options;")]
    assert [m for m in re.findall(r"\b(trials|sample_size|seed|threshold|refit)\b;", opts)] == ["trials", "sample_size", "seed", "threshold", "refit"]
    info = header[header.index("typedef struct sba_resection_consensus_info"):header.index("} sba_resection_consensus_info;")]
    for field in ("n", "n_inlier", "best_trial", "best_trial_inliers", "n_valid_trials", "refit_used", "refit", "n_behind"):
        assert re.search(r"\b%s\b" % field, info), field
    for method in ("score_resection", "resection_guess_consensus"):
        assert hasattr(api.Problem, method), method


def _refused(lib, rc):
    assert rc < 0
    assert cabi.last_error(lib) != ""
    return rc


def test_null_arguments_are_refused_without_a_device(lib):
    """Every argument check comes before the first device call: there is no device here, and nothing is written."""
    z = (C.c_double * 6)(0, 0, 1, 0, 0, 1)
    counts = np.full(4, -7, dtype=np.int64)
    cp = counts.ctypes.data_as(C.POINTER(C.c_longlong))
    f = lib.sba_problem_score_resection
    for args in ((None, z, z, 2, 0.05, cp), (None, None, z, 2, 0.05, cp), (None, z, None, 2, 0.05, cp), (None, z, z, 2, 0.05, None),
                 (None, z, z, 0, 0.05, cp), (None, z, z, 2, float("nan"), cp), (None, z, z, 2, -1.0, cp)):
        assert _refused(lib, f(*args)) == cabi.SBA_ERR_INVALID_ARG
    opt = cabi.ResectionConsensusOptions(128, 6, 7, 0.05, 1)
    bad = cabi.ResectionConsensusOptions(4096, 3, 7, -1.0, 1)
    info = cabi.ResectionConsensusInfo()
    info.n = -7
    r3, t3 = (C.c_double * 3)(-7, -7, -7), (C.c_double * 3)(-7, -7, -7)
    tr, tt = np.full((128, 3), -7.0), np.full((128, 3), -7.0)
    ti = np.full(128, -7, dtype=np.int64)
    tip = ti.ctypes.data_as(C.POINTER(C.c_longlong))
    f = lib.sba_problem_resection_guess_consensus
    dp = lambda a: a.ctypes.data_as(cabi._dp)
    for args in ((None, C.byref(opt), r3, t3, C.byref(info), tip, dp(tr), dp(tt)), (None, None, r3, t3, C.byref(info), None, None, None),
                 (None, C.byref(opt), None, t3, C.byref(info), None, None, None), (None, C.byref(opt), r3, None, C.byref(info), None, None, None),
                 (None, C.byref(opt), r3, t3, None, None, None, None), (None, C.byref(bad), r3, t3, C.byref(info), tip, dp(tr), dp(tt))):
        assert _refused(lib, f(*args)) == cabi.SBA_ERR_INVALID_ARG
    assert (counts == -7).all() and info.n == -7 and (ti == -7).all() and (tr == -7.0).all() and (tt == -7.0).all()
    assert list(r3) == [-7.0] * 3 and list(t3) == [-7.0] * 3 and list(z) == [0, 0, 1, 0, 0, 1]           # nothing written
    assert (opt.trials, opt.sample_size, opt.seed, opt.threshold, opt.refit) == (128, 6, 7, 0.05, 1)


def _has_gpu():
    try:
        return api.device_count() > 0
    except Exception:
        return False


@pytest.mark.skipif(_has_gpu(), reason="only meaningful on a box without a GPU")
def test_fails_loudly_without_device():
    """There is no CPU path to a score: the handle the methods need cannot be made."""
    with pytest.raises(api.SbaError) as ei:
        with api.Problem(0) as p:
            p.resection_guess_consensus(0.05)
    assert ei.value.code == cabi.SBA_ERR_NO_DEVICE


def test_result_type_and_argument_shapes():
    g = api.ResectionConsensus(np.zeros(3), np.zeros(3), 65, 43, 3, 43, 128, True, None, 0.0, None, None, None)
    assert g.n_inlier == 43 and g.refit_used and g.trial_inliers is None
