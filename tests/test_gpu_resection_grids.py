"""GPU: the nine resection kernels where their grid-stride loops iterate on several blocks and where the grids sit at their
production caps, against the long-double references of tests/resection_reference.py, tests/resection_consensus_reference.py and
tests/resection_weighted_reference.py on the cases of tests/resection_grid_cases.py, which tests/test_resection_grid_cases_cpu.py
qualifies (shapes, planted positions, no match on a threshold, float64 numpy within the same bounds).

Small capped grids: SBA_RESECT_GRID = 2, 3 and 5 at sizes where two full steps are followed by a third with G - 2 full blocks,
one block of one wave plus six lanes and an idle block, the last vector holding one match -- and the same data with the switch
unset.  Every entry point of the family is compared with long double; the passes without a reduction and the score counts return
the same bytes for every grid, each reducing pass the same bytes on a second run.  Rows of zero weight planted on the first and
last lane of every wave of a block, in the last block, in the partial wave of the ragged step and at the very last match are
counted exactly for every grid.  Production caps: sizes from the device's CU count that fill the 2-per-CU grid of the reduce
passes (one per CU for the moments passes and the f32 weighted reduce pass, every resident block for the score pass) and go on
into a second, ragged step, so that joint_finalize_kernel folds 2 * CUs rows of 31 and CUs rows of 61."""
import numpy as np
import pytest

import resection_consensus_reference as cr
import resection_grid_cases as gc
import resection_reference as rr
import resection_weighted_reference as wr
from helpers import REL_TOL_F32, REL_TOL_F64, RT_TOL_F32, RT_TOL_F64, assert_normal_eq_close
from spherical_bundle_adjuster_amd import api
from test_gpu_resection_weighted import _row_bound

pytestmark = pytest.mark.gpu

STORES = [api.STORE_F64, api.STORE_F32]
IDS = ["f64", "f32"]
ALL_GRIDS = (None, 1, 2, 3, 5)
SEED, TRIALS = 7, 128                      # the consensus call (tests/test_gpu_resection_consensus.py)


def _f32(store):
    return store == api.STORE_F32


def _rel(store):
    return REL_TOL_F32 if _f32(store) else REL_TOL_F64


def _rt(store):
    return RT_TOL_F32 if _f32(store) else RT_TOL_F64


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _set_grid(monkeypatch, grid):
    if grid is None:
        monkeypatch.delenv("SBA_RESECT_GRID", raising=False)
    else:
        monkeypatch.setenv("SBA_RESECT_GRID", str(grid))


def _bytes(*arrays):
    return b"".join(np.ascontiguousarray(a, dtype=np.float64).tobytes() for a in arrays)


def _eq_bytes(e):
    return _bytes(e.H, e.g, [e.cost, e.sum_w, e.n_outlier, e.n_behind])


def _check(got, ref, rel, what):
    assert_normal_eq_close(got, ref, rel, what)
    assert (got.n_outlier, got.n_behind) == (ref.n_outlier, ref.n_behind), what
    assert abs(got.sum_w - ref.sum_w) <= rel * max(ref.sum_w, 1e-300), what
    assert np.array_equal(got.H, got.H.T), what


# ---- the unweighted passes ----------------------------------------------------------------------------------------------------
def _check_eval(p, n, store, deltas, what):
    """eval_resection at the handle's current grid against long double; exact counts; the same bytes on a second run."""
    for delta in deltas:
        s = gc.eval_scene(n, delta > 0)
        p.upload_landmarks(s.X, s.y, store=store)
        opt = api.default_lm_options(huber_delta=delta)
        got = p.eval_resection(*gc.eval_pose(n), opt)
        ref = gc.eval_reference(n, _f32(store), delta)
        _check(got, ref, _rel(store), f"{what} n={n} delta={delta}")
        if delta == 0.0:
            assert got.sum_w == n and got.n_outlier == 0, what
        else:
            assert got.n_outlier >= 1 and got.sum_w < n, what
        assert _eq_bytes(p.eval_resection(*gc.eval_pose(n), opt)) == _eq_bytes(got), what


def _check_moments(p, n, store, what):
    """resection_guess(moments=True) on the handle's data (eval_scene(n, False)): the 60 sums and the count; a second run."""
    g = p.resection_guess(moments=True)
    ref = gc.moments_reference(n, _f32(store))
    # f64 arithmetic on both sides of the same (rounded) inputs: the f64 bound for either plane type
    assert np.abs(g.moments - ref.astype(np.float64)).max() <= REL_TOL_F64 * float(np.abs(ref).max()), what
    assert g.n == n, what
    again = p.resection_guess(moments=True)
    assert _bytes(again.moments, again.rot, again.tran, [again.n]) == _bytes(g.moments, g.rot, g.tran, [g.n]), what


def _check_depths(p, n, store, what):
    d = p.resection_depths(*gc.eval_pose(n))
    X, _ = rr.planes(gc.eval_scene(n, False), _f32(store))
    err = np.abs(d - gc.depths_reference(n, _f32(store)).astype(np.float64))
    assert err.max() <= _rel(store) * np.abs(X).max(), (what, int(err.argmax()), err.max())
    return d


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("grid", gc.GRIDS)
def test_eval_moments_and_depths_at_small_grids(monkeypatch, grid, store):
    n = gc.small_n(grid, _f32(store))
    with api.Problem(0) as p:
        for g in (grid, None):
            _set_grid(monkeypatch, g)
            what = f"grid={g}"
            _check_eval(p, n, store, (gc.EVAL_DELTA, 0.0), what)        # leaves eval_scene(n, False) on the handle
            _check_moments(p, n, store, what)
            _check_depths(p, n, store, what)


# ---- the consensus passes -----------------------------------------------------------------------------------------------------
def _check_scores(p, n, store, count, what):
    s = cr.score_scene(n)
    rots, trans = cr.score_candidates(n, count)
    ref, amb = gc.score_reference(n, _f32(store), count)
    assert amb.max() == 0
    p.upload_landmarks(s.X, s.y, store=store)
    got = p.score_resection(rots, trans, cr.SCORE_TAU)
    assert got.dtype == np.int64 and np.array_equal(got, ref), (what, n, got, ref)
    # padding slots are never counted: with everything an inlier every count is exactly n
    assert np.array_equal(p.score_resection(rots, trans, 1e30), np.full(count, n)), (what, n)
    return got


def _check_refit(p, n, store, what, behind_dtype=rr.LD):
    """The consensus call on the noise-free scene with every third row a wrong match, as
    tests/test_gpu_resection_consensus.py::test_refit_moments_cover_the_inliers_only checks it."""
    s = cr.exact_scene(n)
    X, y = rr.planes(s, _f32(store))
    good = cr.inlier_rows(n)
    p.upload_landmarks(s.X, s.y, store=store)
    g = p.resection_guess_consensus(gc.REFIT_TAU, trials=TRIALS, seed=SEED, per_trial=True)
    assert g.refit.n == len(good) and g.n_inlier == len(good) and g.best_trial_inliers == len(good) and g.n == n, what
    assert g.refit_used and g.n_behind == rr.sums(X, y, g.rot, g.tran, 0.0, behind_dtype).n_behind, what
    assert (p.resection_depths(g.rot, g.tran)[good] > 0).all(), what
    if _f32(store):
        ref = gc.refit_reference(n, True)
        want = (ref.rot, ref.tran)
    else:
        want = (s.rot, s.tran)
    assert np.abs(g.rot - want[0]).max() <= _rt(store) and np.abs(g.tran - want[1]).max() <= _rt(store), what
    assert g.refit.lambda2 > 0 and g.refit.lambda12 > g.refit.lambda2, what
    return g


def _guess_bytes(g):
    return _bytes(g.rot, g.tran, [g.n, g.n_inlier, g.best_trial, g.best_trial_inliers, g.n_behind, g.refit.n, g.refit.lambda1,
                                  g.refit.lambda2, g.refit.lambda12, g.refit.scale], g.refit.sv, g.trial_inliers)


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("grid", gc.GRIDS)
def test_scores_and_consensus_refit_at_small_grids(monkeypatch, grid, store):
    n = gc.small_n(grid, _f32(store))
    with api.Problem(0) as p:
        for g in (grid, None):
            _set_grid(monkeypatch, g)
            what = f"grid={g}"
            _check_scores(p, n, store, gc.SCORE_COUNT, what)
            first = _check_refit(p, n, store, what)
            again = p.resection_guess_consensus(gc.REFIT_TAU, trials=TRIALS, seed=SEED, per_trial=True)
            assert _guess_bytes(again) == _guess_bytes(first), what      # the inlier moments pass: the same bytes on a second run


# ---- the weighted passes ------------------------------------------------------------------------------------------------------
def _check_weighted(p, n, store, deltas, what):
    """freeze_resection_weights, resection_weights and eval_resection_weighted at the handle's current grid."""
    for delta in deltas:
        c = gc.weighted_case(n, delta)
        ref, M, _ = gc.weighted_reference(n, _f32(store), delta)
        p.upload_landmarks(c.scene.X, c.scene.y, store=store)
        p.set_landmark_covariances(c.cov, wr.COV_SCALE)
        assert p.freeze_resection_weights(c.rot_w, c.tran_w, c.bearing_sigma) == 0, what
        rows = p.resection_weights()
        assert rows.shape == (n, 6)
        err = wr.row_error(rows, M)
        assert err <= _row_bound(), f"{what} delta={delta}: M row error {err:.3e}, bound {_row_bound():.3e}"
        opt = api.default_lm_options(huber_delta=delta)
        got = p.eval_resection_weighted(c.rot, c.tran, opt)
        _check(got, ref, _rel(store), f"{what} n={n} delta={delta}")
        assert np.isfinite(got.H).all() and np.isfinite(got.g).all() and np.isfinite(got.cost), what
        if delta == 0.0:
            assert got.sum_w == n and got.n_outlier == 0, what
        else:
            assert got.n_outlier >= 1 and got.sum_w < n, what
        assert _eq_bytes(p.eval_resection_weighted(c.rot, c.tran, opt)) == _eq_bytes(got), what
        assert p.freeze_resection_weights(c.rot_w, c.tran_w, c.bearing_sigma) == 0, what
        assert p.resection_weights().tobytes() == rows.tobytes(), what


@pytest.mark.parametrize("store", STORES, ids=IDS)
@pytest.mark.parametrize("grid", gc.GRIDS)
def test_weighted_freeze_rows_and_eval_at_small_grids(monkeypatch, grid, store):
    n = gc.small_n(grid, _f32(store))
    with api.Problem(0) as p:
        for g in (grid, None):
            _set_grid(monkeypatch, g)
            _check_weighted(p, n, store, (0.0, wr.DELTA), f"grid={g}")


# ---- what the code promises not to depend on the grid -------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_passes_without_a_reduction_return_the_same_bytes_for_every_grid(monkeypatch, store):
    """Depths, weight rows, n_zero_weight (the planted rows of the zero-weight case) and the score counts for SBA_RESECT_GRID
    unset, 1, 2, 3 and 5: one to eight steps per block."""
    f32 = _f32(store)
    n = gc.small_n(gc.ZERO_GRID, f32)
    z = gc.zero_case(f32)
    s = gc.eval_scene(n, False)
    seen = []
    with api.Problem(0) as p:
        for g in ALL_GRIDS:
            _set_grid(monkeypatch, g)
            p.upload_landmarks(s.X, s.y, store=store)
            d = _check_depths(p, n, store, f"grid={g}")
            counts = _check_scores(p, n, store, gc.SCORE_COUNT, f"grid={g}")
            p.upload_landmarks(z.scene.X, z.y, store=store)
            p.set_landmark_covariances(z.cov, wr.COV_SCALE)
            n_zero = p.freeze_resection_weights(z.rot_w, z.tran_w, z.bearing_sigma)
            seen.append((d.tobytes(), counts.tobytes(), p.resection_weights().tobytes(), n_zero))
    assert all(k == seen[0] for k in seen[1:]), [tuple(a == b for a, b in zip(k, seen[0])) for k in seen]
    assert seen[0][3] == len(z.rows)


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_planted_zero_weights_are_counted_on_every_lane_and_step(monkeypatch, store):
    f32 = _f32(store)
    z = gc.zero_case(f32)
    n, dead, live = z.n, z.rows, z.live
    ref, M = gc.zero_reference(f32)
    opt = api.default_lm_options(huber_delta=z.delta)
    with api.Problem(0) as p:
        p.upload_landmarks(z.scene.X, z.y, store=store)
        p.set_landmark_covariances(z.cov, wr.COV_SCALE)
        for g in (None, 1, gc.ZERO_GRID):
            _set_grid(monkeypatch, g)
            what = f"grid={g}"
            assert p.freeze_resection_weights(z.rot_w, z.tran_w, z.bearing_sigma) == len(dead), what
            assert p.freeze_resection_weights(z.rot_w, z.tran_w, z.bearing_sigma) == len(dead), what    # an integer: the same on every run
            rows = p.resection_weights()
            assert not rows[dead].any() and np.isfinite(rows).all(), what
            assert (np.abs(rows[live]).max(axis=1) > 0).all(), what
            assert wr.row_error(rows[live], M) <= _row_bound(), what
            got = p.eval_resection_weighted(z.rot, z.tran, opt)
            _check(got, ref, _rel(store), f"zero weight {what}")
            assert np.isfinite(got.H).all() and np.isfinite(got.g).all() and np.isfinite(got.cost), what
            cv = p.resection_covariance(z.rot, z.tran, opt)
            assert (cv.n_zero_weight, cv.n_used, cv.dof) == (len(dead), n - len(dead), 2 * (n - len(dead)) - 6), what


# ---- the production caps ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_eval_and_moments_at_the_production_caps(store):
    """2 * CUs blocks and a ragged second step in the reduce pass, CUs blocks and three steps in the moments pass."""
    n = gc.cap_n(_cus(), _f32(store))
    with api.Problem(0) as p:
        _check_eval(p, n, store, (gc.EVAL_DELTA,), "caps")
        s = gc.eval_scene(n, False)
        p.upload_landmarks(s.X, s.y, store=store)
        _check_moments(p, n, store, "caps")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_weighted_freeze_and_eval_at_the_production_caps(store):
    """The weighted reduce pass at 2 * CUs blocks (f64 planes) and at CUs blocks and three steps (f32 planes)."""
    n = gc.cap_n(_cus(), _f32(store))
    with api.Problem(0) as p:
        _check_weighted(p, n, store, (wr.DELTA,), "caps")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_consensus_refit_at_the_production_caps(store):
    """The inlier moments pass at CUs blocks and three steps, between score passes over 128 trials."""
    n = gc.cap_n(_cus(), _f32(store))
    with api.Problem(0) as p:
        _check_refit(p, n, store, "caps")


@pytest.mark.parametrize("store", STORES, ids=IDS)
def test_scores_at_the_production_caps(store):
    """Every resident block of the score pass and at least one more step, four candidates."""
    n = gc.score_cap_n(_cus(), _f32(store))
    with api.Problem(0) as p:
        _check_scores(p, n, store, gc.CAP_SCORE_COUNT, "caps")
