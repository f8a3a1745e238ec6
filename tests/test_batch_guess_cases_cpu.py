"""CPU: the cases the GPU test of the batched guess (test_gpu_batch_guess.py) runs, on numpy group moments -- the host's
consensus pick (csrc/sba_epipolar.hpp consensus_pick) against its plain restatement (guess_cases.consensus_reference) at every
candidate count the device kernel treats differently, and the evidence that the scenes reach those counts."""
import numpy as np
import pytest

import guess_cases as gc
from spherical_bundle_adjuster_amd import api
from test_initial_guess_cpu import group_moments


@pytest.fixture(scope="module")
def cases():
    """{scene name: [(sweep entry, candidates of the harness, reference pick, reference means)]} and the scenes' moments."""
    out, moments = {}, {}
    for s in gc.SCENES:
        x1, x2 = gc.make_scene(s)
        G, _, _ = group_moments(x1, x2)
        moments[s.name] = G
        rows = []
        for tr, fr, sd in gc.SWEEP:
            e, t, valid, avg, pick = gc.candidates(G, tr, fr, sd)
            pick_ref, avgs_ref = gc.consensus_reference(e[valid])
            rows.append(((tr, fr, sd), (e, t, valid, avg, pick), pick_ref, avgs_ref))
        out[s.name] = rows
    return out, moments


@pytest.mark.parametrize("scene", [s.name for s in gc.SCENES])
def test_host_consensus_equals_the_restatement(cases, scene):
    """Per case of the sweep: the product's pick is the restatement's, every trimmed mean (the picked one included) has the
    restatement's bits, and sba_initial_guess_from_moments returns that candidate and that count.  No candidate, valid or
    rejected, sits within 1e-5 of the validity threshold, so the device's last-bit differences cannot change the count."""
    rows, moments = cases[0][scene], cases[1][scene]
    for (tr, fr, sd), (e, t, valid, avg, pick), pick_ref, avgs_ref in rows:
        what = (scene, tr, fr, sd)
        assert gc.threshold_clear(e), what
        r = int(valid.sum())
        assert pick == pick_ref, what
        assert len(avg) == len(avgs_ref) == r and np.array_equal(avg, avgs_ref, equal_nan=True), what
        if r == 0:
            with pytest.raises(api.SbaError):
                api.initial_guess_from_moments(moments, tr, fr, sd)
            continue
        # the picked mean, bit for bit (means are sums of non-negative terms: == is bit equality); r = 1: 0 / 0, a NaN in both
        assert (np.isnan(avg[pick]) and np.isnan(avgs_ref[pick_ref])) if r == 1 else avg[pick] == avgs_ref[pick_ref], what
        ea, ta, na = api.initial_guess_from_moments(moments, tr, fr, sd)
        assert na == r and np.array_equal(ea, e[valid][pick].astype(np.float64)) and np.array_equal(ta, t[valid][pick].astype(np.float64)), what


def test_sweep_reaches_every_candidate_count_and_is_mostly_decided(cases, capsys):
    """The candidate counts the device consensus treats differently are all reached on non-empty scenes (0, 1, 2..5, around
    every multiple of 64, the full buffer, both parities in every key slot), and in at most 10 % of the cases two candidates'
    means are too close for device and host to be held to the same pick."""
    counts, undecided, total = [], 0, 0
    for rows in cases[0].values():
        for _, (e, t, valid, avg, pick), _, avgs_ref in rows:
            counts.append(int(valid.sum()))
            undecided += not gc.decided(avgs_ref)
            total += 1
    with capsys.disabled():
        print(f"\nguess cases: {total}, not decided {undecided} ({100.0 * undecided / total:.1f} %), candidate counts seen: {sorted(set(counts))}")
    assert total == len(gc.SCENES) * len(gc.SWEEP)
    assert gc.coverage_gaps(counts) == []
    assert undecided <= 0.10 * total


def test_restatement_on_hand_made_candidates():
    """The restatement itself on cases small enough to check by hand: r = 1 (NaN mean, pick 0), r = 2 (lo = 0, hi = 1: both
    means are 0 / 1, first wins), r = 5 (lo = 1, hi = 4), identical candidates (all means equal: the first wins)."""
    assert gc.consensus_reference(np.zeros((0, 3), np.float32)) == (-1, pytest.approx(np.zeros(0)))
    pick, avgs = gc.consensus_reference(np.array([[0.1, 0.2, 0.3]], np.float32))
    assert pick == 0 and np.isnan(avgs).all()
    pick, avgs = gc.consensus_reference(np.array([[0, 0, 0], [3, 4, 0]], np.float32))
    assert pick == 0 and avgs.tolist() == [0.0, 0.0]
    e = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0], [3, 0, 0], [10, 0, 0]], np.float32)
    pick, avgs = gc.consensus_reference(e)        # sorted rows, entries 1..3: [1,2,3] [1,1,2] [1,1,2] [1,2,3] [7,8,9]
    assert avgs.tolist() == [2.0, 4.0 / 3.0, 4.0 / 3.0, 2.0, 8.0] and pick == 1
    assert gc.decided(avgs) is False and gc.decided([1.0, 1.0 + 2e-6, 3.0]) and not gc.decided([1.0, 1.0 + 5e-7, 3.0])
    pick, avgs = gc.consensus_reference(np.tile(np.array([[0.5, -0.25, 1.0]], np.float32), (7, 1)))
    assert pick == 0 and (avgs == 0.0).all() and gc.decided(avgs)
    assert gc.threshold_clear([[0.1, 1.5699, 0.0], [3.0, 1.57, 0.2]]) and not gc.threshold_clear([[0.1, -1.570004, 0.0]])
