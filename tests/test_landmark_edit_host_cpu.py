"""CPU: the landmark map's edits on the reference alone and on the product's host side.

What the GPU tests (tests/test_gpu_landmark_edit.py) rest on, over the cases they run: csrc/sba_landmarks_edit.hpp, the very text the
kernels call, through a g++-built harness gives the score and the class of the numpy reference BIT FOR BIT; no score lies within
1e-9 relative of any max_score used, so the classification on the device cannot be ambiguous; the index, option and size checks
behave as specified; and the same functions once under AddressSanitizer and UBSan in a program of its own.  The maps are the GPU
test's own, fused on the CPU by csrc/sba_landmarks.hpp (tests/landmark_edit_reference.py: cpu_state)."""
import ctypes as C
import subprocess

import numpy as np
import pytest

import landmark_edit_reference as le
from helpers import ROOT

CASES = [(n, False) for n in le.SIZES + le.LONG] + [(n, True) for n in (257, 2049, 4097, 6145)]


def _cuts(state):
    """(max_score, min_count, mask) of every prune by criteria the GPU test runs on this map."""
    X, Cv, k = state
    n = len(X)
    with np.errstate(all="ignore"):
        cut = le.median_cut(le.scores(X, Cv))
    half = le.mask("half", n)
    return cut, [(np.inf, 0, None), (cut, 0, None), (np.inf, 1, None), (np.inf, 2, None), (np.inf, 0, half), (cut, 1, half), (cut, 2, half),
                 (0.0, 0, None)]


@pytest.mark.parametrize("n,planted", CASES)
def test_score_and_class_equal_the_reference_bit_for_bit(n, planted):
    state = le.cpu_state(n, planted)
    X, Cv, k = state
    s_ref = le.scores(X, Cv)
    s_got = le.harness_scores(X, Cv)
    assert s_got.tobytes() == s_ref.tobytes()
    cut, cuts = _cuts(state)
    assert le.margin_ok(s_ref, cut), (n, cut)                      # no score within 1e-9 relative of the cut
    seen = np.zeros(5, dtype=int)
    for max_score, min_count, mask in cuts:
        ref = le.classify(X, Cv, k, max_score, min_count, mask)
        got = le.harness_classes(X, Cv, k, max_score, min_count, mask)
        assert np.array_equal(got, ref), (n, max_score, min_count)
        kept, counts = le.prune(X, Cv, k, max_score, min_count, mask)
        assert counts[0] == n and sum(counts[1:]) == n and len(kept) == counts[5] and (np.diff(kept) > 0).all()
        seen += np.array(counts[1:])
    if n >= 255:
        assert (seen[1:] > 0).all()                                 # every class but invalid occurs on every map ...
        assert (seen[0] > 0) == planted                             # ... and invalid exactly where it was planted
        assert k.max() == 2 and (k == 0).any() and (k == 1).any()   # the counts differ per landmark
    if planted:
        rows = le.planted_rows(n)
        cls = le.classify(X, Cv, k)
        assert all(cls[i] == le.INVALID for name in ("NaN in X", "inf in Sigma", "negative variance") for i in rows[name])
        assert np.isposinf(s_ref[rows["X = 0"]]).all() and (cls[rows["X = 0"]] == le.KEPT).all()
        assert (le.classify(X, Cv, k, 1e300)[rows["X = 0"]] == le.UNCERTAIN).all()
        where = sorted(i for v in rows.values() for i in v)
        assert len(where) == 15 and len({i // 64 for i in where}) >= min(10, (n + 63) // 64 - 1)               # spread over the waves ...
        assert {i // le.TILE for i in where} == set(range((n + le.TILE - 1) // le.TILE))                        # ... and every tile


def test_the_edits_of_the_reference_are_indexing_and_concatenation():
    state = le.cpu_state(257)
    kept, counts = le.prune(*state, mask=le.mask("alternating", 257))
    assert kept.tolist() == list(range(0, 257, 2)) and counts == (257, 0, 0, 0, 128, 129)
    Xa, Ca = le.extra_rows(5)
    X2, C2, k2 = le.append(le.take(state, kept), Xa, Ca, 1.3)
    assert len(X2) == 134 and X2[129:].tobytes() == Xa.tobytes() and C2[129:].tobytes() == (1.3 * Ca).tobytes() and not k2[129:].any()
    assert le.state_bytes((X2[:129], C2[:129], k2[:129])) == le.state_bytes(le.take(state, kept))
    for name in le.MASKS:
        for n in (3, 257, 4097):
            m = le.mask(name, n)
            assert m.shape == (n,) and m.dtype == bool
    assert {int(le.mask(name, 4097).sum()) % 2 for name in le.MASKS} == {0, 1}           # kept counts of both parities
    m = le.mask("straddle", 4097)
    assert m[le.TILE - 1] and m[le.TILE] and not m[0]
    assert not le.mask("tile", 4097)[le.TILE:2 * le.TILE].any() and le.mask("tile", 4097)[:le.TILE].all()


def test_option_index_and_size_checks():
    h = le.harness()
    assert [h.landmark_edit_harness_check_max_score(v) for v in (0.0, 1e-300, 2.5, np.inf, -1e-300, -1.0, -np.inf, np.nan)] == [1, 1, 1, 1, 0, 0, 0, 0]

    def ci(idx, m, n):
        a = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64)
        return h.landmark_edit_harness_check_gather_index(None if a is None else a.ctypes.data_as(C.POINTER(C.c_int64)), m, n)
    assert ci([9, 0, 3, 3, 2], 5, 10) == 1 and ci(np.arange(10)[::-1], 10, 10) == 1 and ci([], 0, 10) == 1 and ci(None, 0, 0) == 1
    assert ci([0] * 40, 40, 1) == 1                    # more rows than landmarks: repeats are allowed
    assert ci([0, 10, 3], 3, 10) == 0                  # == n
    assert ci([0, -1, 3], 3, 10) == 0
    assert ci([0], 1, 0) == 0                          # an empty map has no rows
    assert ci([2 ** 63 - 1], 1, 10) == 0 and ci([-2 ** 63], 1, 10) == 0
    assert ci(None, 3, 10) == 0                        # NULL with m > 0
    top = 2 ** 64 - 1
    cs = h.landmark_edit_harness_check_sizes
    assert cs(0, 0) == 1 and cs(10 ** 7, 10 ** 7) == 1 and cs(top // 256, 0) == 1
    assert cs(top, 1) == 0 and cs(1, top) == 0 and cs(top // 2, top // 2 + 2) == 0 and cs(top // 256, 1) == 0 and cs(0, top // 64) == 0


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "landmark_edit_sanitize_main"
    src = ROOT / "tests" / "harness" / "landmark_edit_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "landmark edit host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
