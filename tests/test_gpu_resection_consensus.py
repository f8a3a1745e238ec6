"""GPU: the robust resection guess (Problem.score_resection / resection_guess_consensus) against the long-double counts and the
harness-driven trials of tests/resection_consensus_reference.py, on the scenes tests/test_resection_consensus_host_cpu.py
qualifies (no match within 1e-9 tau^2 of the threshold at any candidate, an all-inlier trial among the 128): scoring at the
vector-per-lane, block and counter-register edges of both plane types and over several grid-stride steps (SBA_RESECT_GRID=1);
the refit's moments over the inliers only; the consensus call trial by trial; the solve from the guess against the solve from
the truth; refusals."""
import numpy as np
import pytest

import resection_consensus_reference as cr
import resection_reference as rr
from helpers import RT_TOL_F32, RT_TOL_F64
from spherical_bundle_adjuster_amd import _cabi as cabi
from spherical_bundle_adjuster_amd import api

pytestmark = pytest.mark.gpu

STORES = [api.STORE_F64, api.STORE_F32]
IDS = ["f64", "f32"]
TAU, SEED, TRIALS = 0.05, 7, 128          # the consensus scenes (tests/test_resection_consensus_host_cpu.py)


def _f32(store):
    return store == api.STORE_F32


def _rt(store):
    return RT_TOL_F32 if _f32(store) else RT_TOL_F64


def _outliers_by_eval(p, rots, trans, tau):
    opt = api.default_lm_options(huber_delta=tau)
    return np.array([p.eval_resection(r, t, opt).n_outlier for r, t in zip(rots, trans)])


def _check_scores(p, n, store, counts=cr.SCORE_COUNTS, what=""):
    s = cr.score_scene(n)
    rots, trans = cr.score_candidates(n)
    ref, amb = cr.score_reference(n, _f32(store))
    assert amb.max() == 0
    p.upload_landmarks(s.X, s.y, store=store)
    by_eval = n - _outliers_by_eval(p, rots, trans, cr.SCORE_TAU)
    for count in counts:
        got = p.score_resection(rots[:count], trans[:count], cr.SCORE_TAU)
        assert got.dtype == np.int64 and np.array_equal(got, ref[:count]), (what, n, count, got, ref[:count])
        assert np.array_equal(got, by_eval[:count]), (what, n, count)
        # padding slots are never counted: with everything an inlier every count is exactly n
        assert np.array_equal(p.score_resection(rots[:count], trans[:count], 1e30), np.full(count, n)), (what, n, count)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_scores_against_long_double(store):
    with api.Problem(0) as p:
        for n in cr.SCORE_SIZES[_f32(store)]:
            _check_scores(p, n, store)
        # every counter register of a lane: 1024 candidates, once
        rots, trans = cr.score_candidates(65, 1024)
        ref, amb = cr.score_reference(65, _f32(store), 1024)
        assert amb.max() == 0
        s = cr.score_scene(65)
        p.upload_landmarks(s.X, s.y, store=store)
        got = p.score_resection(rots, trans, cr.SCORE_TAU)
        assert np.array_equal(got, ref) and len(set(got.tolist())) >= 10
        assert np.array_equal(p.score_resection(rots, trans, 1e30), np.full(1024, 65))
        # an empty handle scores zeros
        p.upload_landmarks(np.zeros((0, 3)), np.zeros((0, 3)), store=store)
        assert np.array_equal(p.score_resection(rots[:3], trans[:3], cr.SCORE_TAU), np.zeros(3, dtype=np.int64))


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_scores_do_not_depend_on_the_grid(monkeypatch, store):
    n = cr.SCORE_LONG[_f32(store)]
    s = cr.score_scene(n)
    rots, trans = cr.score_candidates(n)
    ref, amb = cr.score_reference(n, _f32(store))
    assert amb.max() == 0
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, s.y, store=store)
        wide = p.score_resection(rots, trans, cr.SCORE_TAU)
        monkeypatch.setenv("SBA_RESECT_GRID", "1")
        one = p.score_resection(rots, trans, cr.SCORE_TAU)
        assert np.array_equal(one, wide) and np.array_equal(one, ref)
        assert np.array_equal(p.score_resection(rots, trans, 1e30), np.full(len(rots), n))
        monkeypatch.setenv("SBA_RESECT_GRID", "2")
        assert np.array_equal(p.score_resection(rots, trans, cr.SCORE_TAU), ref)
        _check_scores(p, 513, store, counts=(65,), what="two blocks")


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("n", [65, 513])
def test_refit_moments_cover_the_inliers_only(monkeypatch, n, store):
    """Noise-free with every third row a wrong match, tau = 1e-3: the refit is the DLT of exactly the non-planted rows."""
    s = cr.exact_scene(n)
    X, y = rr.planes(s, _f32(store))
    good = cr.inlier_rows(n)
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, s.y, store=store)
        for grid in (None, "1"):
            if grid:
                monkeypatch.setenv("SBA_RESECT_GRID", grid)
            g = p.resection_guess_consensus(1e-3, trials=TRIALS, seed=SEED, per_trial=True)
            assert g.refit.n == len(good) and g.n_inlier == len(good) and g.best_trial_inliers == len(good) and g.n == n
            # the wrong matches have random bearings: about half of them lie behind theirs; no other match does
            assert g.refit_used and g.n_behind == rr.sums(X, y, g.rot, g.tran, 0.0).n_behind
            assert (p.resection_depths(g.rot, g.tran)[good] > 0).all()
            if _f32(store):
                ref = rr.dlt(rr.moments(X[good], y[good]).astype(np.float64))
                want = (ref.rot, ref.tran)
            else:
                want = (s.rot, s.tran)
            assert np.abs(g.rot - want[0]).max() <= _rt(store) and np.abs(g.tran - want[1]).max() <= _rt(store), (n, grid)
            assert g.refit.lambda2 > 0 and g.refit.lambda12 > g.refit.lambda2


def _bytes(g):
    return b"".join(np.ascontiguousarray(a).tobytes() for a in (
        g.rot, g.tran, np.array([g.n, g.n_inlier, g.best_trial, g.best_trial_inliers, g.n_valid_trials, int(g.refit_used)]),
        np.array([g.n_behind, g.refit.lambda1, g.refit.lambda2, g.refit.lambda12, g.refit.scale, g.refit.n]), g.refit.sv,
        g.trial_inliers, g.trial_rot, g.trial_tran))


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("n", [65, 513])
def test_consensus_trial_by_trial(n, store):
    s = cr.noisy_scene(n)
    X, y = rr.planes(s, _f32(store))
    good = cr.inlier_rows(n)
    st, h_rot, h_tran, cond, _ = cr.harness_trials(n, _f32(store))
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, s.y, store=store)
        g = p.resection_guess_consensus(TAU, trials=TRIALS, sample_size=6, seed=SEED, per_trial=True)
        # the trials: valid where the harness's are, the same poses where the sample fixes the pose well
        assert np.array_equal(g.trial_inliers >= 0, st == 0) and g.n_valid_trials == int((st == 0).sum())
        well = np.flatnonzero((st == 0) & (cond >= 1e-5))
        assert len(well) >= TRIALS // 2
        assert np.abs(g.trial_rot[well] - h_rot[well]).max() <= _rt(store) and np.abs(g.trial_tran[well] - h_tran[well]).max() <= _rt(store)
        # the counts: long double at the poses the call itself returned
        ok = np.flatnonzero(g.trial_inliers >= 0)
        ref, amb = cr.counts(X, y, g.trial_rot[ok], g.trial_tran[ok], TAU)
        assert amb.max() == 0
        assert np.array_equal(g.trial_inliers[ok], ref)
        assert g.best_trial == int(np.argmax(g.trial_inliers)) and g.best_trial_inliers == g.trial_inliers.max() == len(good)
        # the returned pose: the refit over the pick's inliers
        ref, amb = cr.counts(X, y, g.rot, g.tran, TAU)
        assert amb[0] == 0 and g.n_inlier == ref[0] and g.n_inlier >= g.best_trial_inliers
        assert g.refit_used and g.refit.n == g.best_trial_inliers and g.n == n
        assert g.n_behind == rr.sums(X, y, g.rot, g.tran, 0.0).n_behind
        dlt = rr.dlt(rr.moments(X[good], y[good]).astype(np.float64))
        assert np.abs(g.rot - dlt.rot).max() <= _rt(store) and np.abs(g.tran - dlt.tran).max() <= _rt(store)
        # without the refit: the pick itself
        plain = p.resection_guess_consensus(TAU, trials=TRIALS, seed=SEED, refit=False)
        assert not plain.refit_used and plain.refit is None and plain.trial_inliers is None
        assert np.array_equal(plain.rot, g.trial_rot[g.best_trial]) and np.array_equal(plain.tran, g.trial_tran[g.best_trial])
        assert plain.n_inlier == g.best_trial_inliers
        # the same bytes on every call and for every number of host threads; another seed draws other trials
        again = p.resection_guess_consensus(TAU, trials=TRIALS, sample_size=6, seed=SEED, per_trial=True)
        assert _bytes(again) == _bytes(g)
        try:
            api.set_host_threads(5)
            five = p.resection_guess_consensus(TAU, trials=TRIALS, sample_size=6, seed=SEED, per_trial=True)
        finally:
            api.set_host_threads(1)                         # the library's default
        one = p.resection_guess_consensus(TAU, trials=TRIALS, sample_size=6, seed=SEED, per_trial=True)
        assert _bytes(one) == _bytes(g) and _bytes(five) == _bytes(g)
        other = p.resection_guess_consensus(TAU, trials=TRIALS, sample_size=6, seed=SEED + 1, per_trial=True)
        assert not np.array_equal(other.trial_rot, g.trial_rot) and other.n_inlier == g.n_inlier
        # defaults: trials = 0 and sample_size = 0 mean 128 and 6; longer samples and fewer trials run too
        dflt = p.resection_guess_consensus(TAU, trials=0, sample_size=0, seed=SEED, per_trial=True)
        assert _bytes(dflt) == _bytes(g)
        few = p.resection_guess_consensus(TAU, trials=1, sample_size=64, seed=SEED, per_trial=True)
        assert few.trial_inliers.shape == (1,) and few.best_trial == 0


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("n", [65, 513])
def test_the_solve_from_the_guess_ends_where_the_solve_from_the_truth_ends(n, store):
    """The point of it all.  With 30 % wrong matches the plain DLT start leaves the Huber LM in a wrong minimum (n = 65) or far
    from it; from the consensus guess it ends where it ends from the truth, within a tenth of that end's own distance to the truth."""
    s = cr.noisy_scene(n)
    opt = api.default_lm_options(huber_delta=TAU)
    with api.Problem(0) as p:
        p.upload_landmarks(s.X, s.y, store=store)
        g = p.resection_guess_consensus(TAU, trials=TRIALS, seed=SEED)
        r, t, sm, nb = p.solve_resection(g.rot, g.tran, opt)
        r0, t0, sm0, nb0 = p.solve_resection(s.rot, s.tran, opt)
        own = max(np.abs(r0 - s.rot).max(), np.abs(t0 - s.tran).max())
        apart = max(np.abs(r - r0).max(), np.abs(t - t0).max())
        print(f"n={n}: the solves end {apart:.3g} apart, {own:.3g} from the truth: ratio {apart / own:.3g}")
        assert own > 0 and apart <= 0.1 * own, (apart, own, sm, sm0)
        # n_behind counts over ALL matches, and a wrong match with its random bearing lies behind it as often as not: the count
        # is the reference's at the result, and it is zero over the matches that are not planted
        X, y = rr.planes(s, _f32(store))
        assert nb == rr.sums(X, y, r, t, TAU).n_behind and nb0 == rr.sums(X, y, r0, t0, TAU).n_behind
        assert (p.resection_depths(r, t)[cr.inlier_rows(n)] > 0).all()


def test_refusals_leave_the_handle_usable():
    s, flat, five = cr.noisy_scene(65), rr.make_scene(65, 5, planar=True), rr.make_scene(5, 5)
    rots, trans = np.stack([s.rot, s.rot]), np.stack([s.tran, s.tran])
    with api.Problem(0) as p:
        calls = (lambda: p.score_resection(rots, trans, TAU), lambda: p.resection_guess_consensus(TAU))

        def refused(code, which=calls):
            for call in which:
                with pytest.raises(api.SbaError) as ei:
                    call()
                assert ei.value.code == code

        refused(cabi.SBA_ERR_NOT_UPLOADED)
        p.upload(s.X, s.y)                                 # no per-match depths: no landmarks
        refused(cabi.SBA_ERR_UNSUPPORTED)
        p.upload_landmarks(s.X, s.y)
        p.set_shard(0, 2)
        refused(cabi.SBA_ERR_UNSUPPORTED)
        p.set_shard(0, 1)
        big = np.zeros((1025, 3))
        bad = rots.copy()
        bad[1, 2] = np.nan
        refused(cabi.SBA_ERR_INVALID_ARG, [lambda v=v: p.score_resection(rots, trans, v) for v in (0.0, -1.0, np.nan, np.inf)] +
                [lambda v=v: p.resection_guess_consensus(v) for v in (0.0, -1.0, np.nan, np.inf)] +
                [lambda: p.score_resection(big, big, TAU), lambda: p.score_resection(big[:0], big[:0], TAU),
                 lambda: p.resection_guess_consensus(TAU, trials=1025), lambda: p.resection_guess_consensus(TAU, trials=-1),
                 lambda: p.resection_guess_consensus(TAU, sample_size=5), lambda: p.resection_guess_consensus(TAU, sample_size=65)])
        refused(cabi.SBA_ERR_NUMERIC, (lambda: p.score_resection(bad, trans, TAU), lambda: p.score_resection(rots, bad, TAU)))
        assert np.isfinite(p.eval_resection(s.rot, s.tran).cost)
        # fewer matches than a sample; a planar scene on which every trial refuses
        for scene, kw in ((five, {}), (s, dict(sample_size=64, trials=2)), (flat, {})):
            p.upload_landmarks(scene.X[:60] if kw else scene.X, scene.y[:60] if kw else scene.y)
            with pytest.raises(api.SbaError) as ei:
                p.resection_guess_consensus(TAU, **kw)
            assert ei.value.code == cabi.SBA_ERR_NUMERIC
            assert np.isfinite(p.eval_resection(scene.rot, scene.tran).cost)
            assert p.score_resection(rots, trans, TAU).shape == (2,)
        p.upload_landmarks(s.X, s.y)
        assert p.resection_guess_consensus(TAU, seed=SEED).n_inlier == len(cr.inlier_rows(65))
