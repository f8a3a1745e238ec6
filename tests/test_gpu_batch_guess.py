"""GPU (-m gpu): the on-device trials and consensus pick of a batch (csrc/sba_epipolar.hip batch_guess_kernel) across trial
counts, subset fractions and -- above all -- candidate counts: the rank sort's key slots per lane, the padding to an even
count, the 20-80 % bounds at r = 1..5, the double-buffered sorted distances aliased onto the trial records, the full buffer
at r = 256, a non-empty pair without any candidate.  Reference: the host's per-trial code on the DEVICE'S OWN group moments
(tests/harness/epi_harness.cpp) and a plain restatement of the consensus (guess_cases.consensus_reference).  Also the moments
pass at its 1024-match step edges, position independence, and the pipeline with a pair that has no candidate."""
import os

import numpy as np
import pytest

import guess_cases as gc
from helpers import make_pairs
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api
from test_initial_guess_cpu import group_moments

pytestmark = pytest.mark.gpu

# the one libm call of a trial (double atan2, rounded to float) may differ between device and host in the last float bit
EULER_TOL, TRAN_TOL = 2.5e-7, 1.2e-7
EMPTY_AT = 3                     # where the empty pair sits among the scenes


def _batch_arrays(order):
    """x1, x2, offsets of the scenes in `order` (None: an empty pair)."""
    xs = [gc.make_scene(s) if s is not None else (np.zeros((0, 3)), np.zeros((0, 3))) for s in order]
    off = np.concatenate([[0], np.cumsum([len(a) for a, _ in xs])]).astype(np.uint64)
    return np.concatenate([a for a, _ in xs]), np.concatenate([c for _, c in xs]), off


def _order():
    order = list(gc.SCENES)
    order.insert(EMPTY_AT, None)
    return order


class _HostPath:
    """SBA_BATCH_DEVICE_GUESS=0 for the duration of the block."""
    def __enter__(self):
        self.old = os.environ.get("SBA_BATCH_DEVICE_GUESS")
        os.environ["SBA_BATCH_DEVICE_GUESS"] = "0"

    def __exit__(self, *exc):
        if self.old is None:
            del os.environ["SBA_BATCH_DEVICE_GUESS"]
        else:
            os.environ["SBA_BATCH_DEVICE_GUESS"] = self.old


@pytest.fixture(scope="module")
def runs():
    """One batch of all scenes plus an empty pair, f64 planes: the device's moments, and for every entry of the sweep the
    device's guess (twice) and the host path's guess on the same batch; 129 trials (more than the kernel holds) both ways."""
    assert "SBA_BATCH_DEVICE_GUESS" not in os.environ
    order = _order()
    x1, x2, off = _batch_arrays(order)
    out = {"order": order, "dev": {}, "dev2": {}, "host": {}}
    with api.Batch(0) as b:
        b.upload(x1, x2, off)
        out["gm"] = b.epipolar_moments()
        for sw in gc.SWEEP:
            out["dev"][sw] = b.initial_guess(*sw, check=False)
            out["dev2"][sw] = b.initial_guess(*sw, check=False)
        out["over"] = {sd: b.initial_guess(129, 0.25, sd, check=False) for sd in gc.SEEDS}
        with _HostPath():
            for sw in gc.SWEEP:
                out["host"][sw] = b.initial_guess(*sw, check=False)
            out["over_host"] = {sd: b.initial_guess(129, 0.25, sd, check=False) for sd in gc.SEEDS}
    return out


def _reference(gm, order, sweep):
    """{(pair, sweep entry): (euler_all, tran_all, valid, pick_ref, avgs_ref)} from the harness on the moments `gm`."""
    ref = {}
    for g, s in enumerate(order):
        for sw in sweep:
            e, t, valid, avg, pick = gc.candidates(gm[g], *sw)
            pick_ref, avgs_ref = gc.consensus_reference(e[valid])
            assert pick == pick_ref and np.array_equal(avg, avgs_ref, equal_nan=True), (g, sw)      # host == restatement, as on the CPU
            ref[(g, sw)] = (e, t, valid, pick_ref, avgs_ref)
    return ref


@pytest.fixture(scope="module")
def refs(runs):
    return _reference(runs["gm"], runs["order"], gc.SWEEP)


def _check_against_reference(got, ref, order, sw):
    """The device's guess `got` of every pair for sweep entry `sw` against the reference.  Returns (cases, not decided)."""
    e_dev, t_dev, nc_dev, st_dev = got
    undecided = 0
    for g, s in enumerate(order):
        e, t, valid, pick_ref, avgs_ref = ref[(g, sw)]
        what = (s.name if s else "empty", sw)
        assert gc.threshold_clear(e), what
        r = int(valid.sum())
        assert nc_dev[g] == r and st_dev[g] == (0 if r > 0 else cabi.SBA_ERR_NUMERIC), (what, nc_dev[g], r, st_dev[g])
        if r == 0:
            assert not e_dev[g].any() and not t_dev[g].any(), what
            continue
        ev, tv = e[valid].astype(np.float64), t[valid].astype(np.float64)
        if gc.decided(avgs_ref):
            assert np.abs(e_dev[g] - ev[pick_ref]).max() <= EULER_TOL and np.abs(t_dev[g] - tv[pick_ref]).max() <= TRAN_TOL, \
                (what, r, pick_ref, e_dev[g], ev[pick_ref], t_dev[g], tv[pick_ref])
        else:
            undecided += 1
            near = np.flatnonzero(avgs_ref <= np.nanmin(avgs_ref) + gc.DECIDED_GAP)
            ok = [(np.abs(e_dev[g] - ev[k]).max() <= EULER_TOL and np.abs(t_dev[g] - tv[k]).max() <= TRAN_TOL) for k in near]
            assert any(ok), (what, r, near.tolist(), e_dev[g], t_dev[g])
    return len(order), undecided


def test_device_guess_is_repeatable(runs):
    for sw in gc.SWEEP:
        for a, c in zip(runs["dev"][sw], runs["dev2"][sw]):
            assert np.array_equal(a, c), sw


@pytest.mark.parametrize("sw", gc.SWEEP, ids=[f"trials{tr}-fraction{fr}-seed{sd}" for tr, fr, sd in gc.SWEEP])
def test_device_guess_matches_the_reference(runs, refs, sw):
    """Per entry of the sweep, every scene: candidate count and status exactly; the picked candidate within the one-libm-call
    bounds of the reference's pick where the means decide it, else of some candidate whose mean is within 1e-6 of the smallest."""
    _check_against_reference(runs["dev"][sw], refs, runs["order"], sw)


def test_device_guess_over_the_whole_sweep(runs, refs, capsys):
    """Over the whole sweep: at most 10 % of the cases are not decided by their means; at least 90 % of the compared cases
    (a candidate exists) are bit-equal to the host path on the same batch; and the DEVICE'S candidate counts reach every
    count the consensus treats differently -- on non-empty pairs."""
    order = runs["order"]
    total = undecided = compared = equal = 0
    counts = []
    for sw in gc.SWEEP:
        n, u = _check_against_reference(runs["dev"][sw], refs, order, sw)
        total += n; undecided += u
        e_d, t_d, nc_d, st_d = runs["dev"][sw]
        e_h, t_h, nc_h, st_h = runs["host"][sw]
        assert np.array_equal(nc_d, nc_h) and np.array_equal(st_d, st_h), sw
        for g, s in enumerate(order):
            if s is not None:
                counts.append(int(nc_d[g]))
            if nc_d[g] > 0:
                compared += 1
                equal += bool(np.array_equal(e_d[g], e_h[g]) and np.array_equal(t_d[g], t_h[g]))
    with capsys.disabled():
        print(f"\ndevice guess cases: {total}, not decided {undecided} ({100.0 * undecided / total:.1f} %), bit-equal to the host "
              f"{equal} of {compared} ({100.0 * equal / compared:.1f} %), candidate counts seen: {sorted(set(counts))}")
    assert undecided <= 0.10 * total
    assert equal >= 0.90 * compared
    assert gc.coverage_gaps(counts) == []


def test_host_path_on_the_same_batch_equals_the_harness(runs, refs):
    """SBA_BATCH_DEVICE_GUESS=0: the host loop on the device's moments is the harness' result, exactly; 129 trials -- more than
    the kernel holds -- take that path without the variable and give the same bits."""
    order = runs["order"]
    for sw in gc.SWEEP:
        e_h, t_h, nc_h, st_h = runs["host"][sw]
        for g, s in enumerate(order):
            e, t, valid, pick_ref, _ = refs[(g, sw)]
            r = int(valid.sum())
            assert nc_h[g] == r and st_h[g] == (0 if r > 0 else cabi.SBA_ERR_NUMERIC), (g, sw)
            want_e = e[valid][pick_ref].astype(np.float64) if r else np.zeros(3)
            want_t = t[valid][pick_ref].astype(np.float64) if r else np.zeros(3)
            assert np.array_equal(e_h[g], want_e) and np.array_equal(t_h[g], want_t), (g, sw)
    for sd in gc.SEEDS:
        for a, c in zip(runs["over"][sd], runs["over_host"][sd]):
            assert np.array_equal(a, c), sd
        e_o, t_o, nc_o, st_o = runs["over"][sd]
        for g, s in enumerate(order):
            e, t, valid, avg, pick = gc.candidates(runs["gm"][g], 129, 0.25, sd)
            assert nc_o[g] == int(valid.sum()), (g, sd)
            if pick >= 0:
                assert np.array_equal(e_o[g], e[valid][pick].astype(np.float64)) and np.array_equal(t_o[g], t[valid][pick].astype(np.float64)), (g, sd)


def test_device_guess_on_f32_planes():
    """f32 planes feed the same consensus from other moments: three trial counts against the reference on THOSE moments."""
    order = _order()
    x1, x2, off = _batch_arrays(order)
    sweep = [(5, 0.25, 3), (97, 0.25, 11), (128, 0.25, 3)]
    with api.Batch(0) as b:
        b.upload(x1, x2, off, store=api.STORE_F32)
        gm = b.epipolar_moments()
        got = {sw: b.initial_guess(*sw, check=False) for sw in sweep}
    ref = _reference(gm, order, sweep)
    for sw in sweep:
        _check_against_reference(got[sw], ref, order, sw)
    assert {256, 5} <= {int(c) for sw in sweep for c in got[sw][2]}


def test_guess_does_not_depend_on_the_position_in_the_batch(runs):
    """The same pairs uploaded in reverse order: moments and every output of the guess are the reverse, bit for bit."""
    order = runs["order"][::-1]
    x1, x2, off = _batch_arrays(order)
    with api.Batch(0) as b:
        b.upload(x1, x2, off)
        assert np.array_equal(b.epipolar_moments(), runs["gm"][::-1])
        for sw in [(5, 0.25, 3), (97, 0.25, 11), (128, 0.25, 3), (128, 0.02, 11)]:
            for a, c in zip(b.initial_guess(*sw, check=False), runs["dev"][sw]):
                assert np.array_equal(a, c[::-1]), sw


@pytest.mark.parametrize("store", [api.STORE_F64, api.STORE_F32], ids=["f64", "f32"])
@pytest.mark.parametrize("layout", ["0", "1"], ids=["contiguous", "interleaved"])
def test_batch_moments_at_the_step_edges(store, layout, monkeypatch):
    """batch_epipolar_moments_kernel: 512 lanes take 1024 matches per step and load two steps ahead -- pairs that end one
    match before, at and after one, two and three steps, against numpy on the stored coordinates and against the
    single-problem pass on the pair alone."""
    monkeypatch.setenv("SBA_BATCH_INTERLEAVE", layout)
    sizes = [1023, 1024, 1025, 2047, 2048, 2049, 3071, 3072, 3073]
    cs, off, x1, x2, d12 = make_pairs(sizes, seed0=8800)
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d12, store=store)
        gm = b.epipolar_moments()
    for g, c in enumerate(cs):
        a1, a2 = ((c.x1, c.x2) if store == api.STORE_F64 else
                  (c.x1.astype(np.float32).astype(np.float64), c.x2.astype(np.float32).astype(np.float64)))
        ref, _, _ = group_moments(a1, a2)
        assert np.abs(gm[g] - ref).max() <= 1e-12 * max(np.abs(ref).max(), 1.0), (g, sizes[g])
        with api.Problem(0) as p:
            p.upload(c.x1, c.x2, c.d12, store=store)
            gs = p.epipolar_moments()
        assert np.abs(gm[g] - gs).max() <= 1e-12 * max(np.abs(gs).max(), 1.0), (g, sizes[g])


def test_pipeline_keeps_the_start_values_of_a_pair_without_candidates():
    """sba_batch_solve_problem with 128 trials on a batch holding a pair without any candidate and a pair that fills the
    consensus buffer (256): the first reports SBA_ERR_NUMERIC and 0 candidates and runs its stages from the caller's start
    values -- bit-equal to the pipeline without the guess from those values -- every other pair succeeds."""
    by_name = {s.name: s for s in gc.SCENES}
    order = [by_name["none_158"], by_name["both_clean"], by_name["clean_300"]]
    x1, x2, off = _batch_arrays(order)
    d0 = np.full((int(off[-1]), 2), 6.0)
    rot0 = np.tile(np.array([0.1, -0.2, 0.05]), (3, 1)); tran0 = np.tile(np.array([0.0, 0.6, 0.8]), (3, 1))
    with api.Batch(0) as b:
        b.upload(x1, x2, off, d0)
        e, t, nc, st = b.initial_guess(128, 0.25, 3, check=False)
        assert nc.tolist() == [0, 256, 128] and st.tolist() == [cabi.SBA_ERR_NUMERIC, 0, 0]
        res = b.solve_problem(rot=rot0, tran=tran0, use_initial_guess=True, trials=128, seed=3, want_depths=True, check=False)
        # the same pipeline from explicit start values: the caller's for the pair without candidates, the guess for the others
        rot1, tran1 = rot0.copy(), tran0.copy()
        rot1[1:], tran1[1:] = -e[1:], t[1:]
        b.upload(x1, x2, off, d0)
        res2 = b.solve_problem(rot=rot1, tran=tran1, use_initial_guess=False, want_depths=True)
    assert res["status"].tolist() == [cabi.SBA_ERR_NUMERIC, 0, 0] and res["guess_candidates"].tolist() == [0, 256, 128]
    assert res2["status"][1:].tolist() == [0, 0]
    lo, hi = int(off[0]), int(off[1])
    assert np.array_equal(res["rot"][0], res2["rot"][0]) and np.array_equal(res["tran"][0], res2["tran"][0])
    assert np.array_equal(res["d_uniform"][0], res2["d_uniform"][0]) and np.array_equal(res["d12"][lo:hi], res2["d12"][lo:hi])
    assert not np.array_equal(res["rot"][0], rot0[0])                 # the stages really ran for that pair
    # ... and the pairs that have a guess start from it, as in the pipeline from explicit start values
    assert np.array_equal(res["rot"], res2["rot"]) and np.array_equal(res["tran"], res2["tran"])
