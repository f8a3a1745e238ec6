"""CPU: the host side of the robust resection guess (csrc/sba_resection_consensus.hpp compiled with g++,
tests/harness/resection_consensus_harness.cpp) against the restatements of tests/resection_consensus_reference.py: the sampler
index for index, the moments of a row list, the pick rule; the same code under the address and undefined-behaviour
sanitizers in a program of its own; and, on the reference alone, the conditions the GPU tests of the consensus rest on."""
import subprocess

import numpy as np
import pytest

import resection_consensus_reference as cr
import resection_reference as rr
from helpers import REL_TOL_F64, ROOT

TRIALS = 128
SEED = 7
TAU = 0.05


def test_limits():
    assert [cr.harness().consensus_harness_limit(k) for k in range(6)] == [1024, 64, 128, 6, 6, 12]


@pytest.mark.parametrize("n", [6, 7, 65, 513, 10 ** 7])
def test_sampler_equals_the_restatement(n):
    by_size = {}
    for m in (6, 8, 64):
        if m > n:
            continue
        got = cr.harness_sample(SEED, TRIALS, n, m)
        ref = cr.sample(SEED, TRIALS, n, m)
        assert np.array_equal(got, ref), (n, m)
        assert got.min() >= 0 and got.max() < n
        assert all(len(set(row)) == m for row in got.tolist())
        by_size[m] = got
    if 8 in by_size:
        assert np.array_equal(by_size[8][:, :6], by_size[6])          # a longer sample extends a shorter one
    if 64 in by_size:
        assert np.array_equal(by_size[64][:, :8], by_size[8])
    other = cr.harness_sample(SEED + 1, TRIALS, n, 6)
    if n > 7:
        assert not np.array_equal(other, by_size[6])                   # another seed draws other trials
    if n == 6:
        assert all(sorted(row) == list(range(6)) for row in by_size[6].tolist())


def test_sampler_seeds_like_the_group_sampler():
    """seed * 0x2545F4914F6CDD1D + trial * 0xD6E8FEB86659FD93 + 1, wrapping at 64 bits, also for a seed with the top bit set."""
    for seed in (0, 1, (1 << 64) - 1, 0x8000000000000001):
        assert np.array_equal(cr.harness_sample(seed, 4, 1000, 6), cr.sample(seed, 4, 1000, 6)), seed


@pytest.mark.parametrize("m", [6, 8, 64])
def test_row_moments_equal_the_reference(m):
    s = cr.noisy_scene(513)
    idx = cr.sample(SEED, 3, 513, m)[2]
    mom = cr.harness_row_moments(np.concatenate([s.X[idx], s.y[idx]], axis=1))
    ref = rr.moments(s.X[idx], s.y[idx])
    assert mom[60] == m
    assert np.abs(mom[:60] - ref.astype(np.float64)).max() <= REL_TOL_F64 * float(np.abs(ref).max())
    # a whole trial = these moments through the DLT finish
    rc, rot, tran, cond = cr.harness_trial(np.concatenate([s.X[idx], s.y[idx]], axis=1))
    rc2, rot2, tran2, *_ = rr.harness_dlt(mom[:60], m)
    assert rc == rc2 == 0 and np.array_equal(rot, rot2) and np.array_equal(tran, tran2) and cond > 0


def test_pick_rule():
    assert cr.harness_pick([3, 9, 9, 2]) == 1                          # ties: the lowest trial index
    assert cr.harness_pick([-1, 4, -1, 4]) == 1                        # refused trials never win
    assert cr.harness_pick([-1, -1, 0]) == 2                           # a count of zero beats a refusal
    assert cr.harness_pick([-1, -1, -1]) == -1                         # no trial finished
    assert cr.harness_pick([5]) == 0
    assert cr.harness_pick(np.arange(1024)) == 1023


def test_host_code_under_asan_and_ubsan(tmp_path):
    exe = tmp_path / "resection_consensus_sanitize_main"
    src = ROOT / "tests" / "harness" / "resection_consensus_sanitize_main.cpp"
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-fno-omit-frame-pointer", "-o", str(exe), str(src)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120,
                       env={"ASAN_OPTIONS": "detect_leaks=1:abort_on_error=0", "UBSAN_OPTIONS": "print_stacktrace=1"})
    assert r.returncode == 0 and "resection consensus host checks passed" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("n", [65, 513])
def test_the_conditions_the_gpu_tests_rest_on(n, f32):
    """On the noisy scenes with every third row a wrong match: some trial draws inliers only, the best trial's count is the
    number of non-planted rows, and no match sits on the threshold at any trial's pose."""
    s = cr.noisy_scene(n)
    X, y = rr.planes(s, f32)
    good = cr.inlier_rows(n)
    st, rot, tran, cond, idx = cr.harness_trials(n, f32)
    clean = np.isin(idx, good).all(axis=1)
    assert clean.sum() >= 1, "no all-inlier trial"
    print(f"n={n}: {int(clean.sum())} all-inlier trials, {int((st == 0).sum())} valid")
    ok = np.flatnonzero(st == 0)
    inl, amb = cr.counts(X, y, rot[ok], tran[ok], TAU)
    assert amb.max() == 0
    full = np.full(TRIALS, -1, dtype=np.int64)
    full[ok] = inl
    best = cr.harness_pick(full)
    assert full[best] == len(good)
    # the pick's inliers are exactly the non-planted rows
    assert np.array_equal(np.flatnonzero(cr.sq_residuals(X, y, rot[best], tran[best]) <= TAU * TAU), good)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
def test_no_match_is_ambiguous_on_the_scoring_scenes(f32):
    """What lets the GPU test ask for EQUAL counts: at none of the candidates of any scoring scene does a match sit within
    1e-9 tau^2 of the threshold; and the candidates spread the counts from all inliers to none."""
    for n in cr.SCORE_SIZES[f32] + (cr.SCORE_LONG[f32],):
        inl, amb = cr.score_reference(n, f32)
        assert amb.max() == 0, n
        assert inl.max() <= n
        if n >= 63:
            assert inl[0] >= 0.85 * n and inl.min() == 0 and len(set(inl.tolist())) >= 10, (n, inl[:8])
    inl, amb = cr.score_reference(65, f32, 1024)
    assert amb.max() == 0 and np.array_equal(inl[:200], cr.score_reference(65, f32)[0])
