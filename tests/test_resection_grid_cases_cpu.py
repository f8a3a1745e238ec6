"""CPU: the conditions tests/test_gpu_resection_grids.py rests on, over every case of tests/resection_grid_cases.py, with the CU
counts 1, 8, 64, 256 and 304 standing in for the device.

The shapes: at the small capped grids every block takes two full steps and the third has G - 2 full blocks, one block of one
full wave plus six lanes and an idle block; at the production caps the grid is full and a second, ragged step follows; the last
vector holds one match.  The planted rows of zero weight fall on the lanes the GPU test names.  The scenes: no match within
AMBIGUITY tau^2 of tau^2 at any scored candidate, none on the Huber threshold (float64 and long double count the same outliers;
the weighted chi^2 keeps MARGIN delta^2 from delta^2), and float64 numpy in the product's formulation and its own summation order
meets the GPU test's bounds against long double: REL_TOL_F64 block-relative for the sums, the moments and the depths, and 8 times
tests/test_resection_weighted_host_cpu.py's measured_row_error() for the M rows.  The noise-free consensus scene: a trial of the
128 whose inliers are exactly the rows that are not planted."""
from functools import lru_cache

import numpy as np
import pytest

import resection_consensus_reference as cr
import resection_grid_cases as gc
import resection_reference as rr
import resection_weighted_reference as wr
import test_resection_weighted_host_cpu as wh
from helpers import REL_TOL_F64, assert_normal_eq_close

F32 = [False, True]
IDS = ["f64", "f32"]
REFIT_SEED, REFIT_TRIALS = 7, 128              # tests/test_gpu_resection_consensus.py: SEED, TRIALS


@lru_cache(maxsize=None)
def _row_bound():
    return 8.0 * wh.measured_row_error()


# ---- shapes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f32", F32, ids=IDS)
@pytest.mark.parametrize("grid", gc.GRIDS)
def test_small_grids_take_three_steps_with_an_idle_block_and_a_partial_wave(grid, f32):
    ppt, n = gc.PPT[f32], gc.small_n(grid, f32)
    assert n == ppt * gc.small_nvec(grid) - (ppt - 1) and (n - 1) % ppt == 0         # one match in the last vector
    steps, last = gc.steps_and_blocks(n, ppt, grid)
    assert len(steps) == grid and max(steps) == 3 and min(steps) == 2
    assert steps == [3] * (grid - 1) + [2]                                            # the idle block of step 3 is the last one
    assert gc.last_step_blocks(n, ppt, grid) == (grid - 2, 70, 1)                     # 70 lanes: one full wave plus six
    # one block alone walks every vector; the default grid of the device gives each block one step
    assert gc.steps_and_blocks(n, ppt, 1) == ([-(-gc.small_nvec(grid) // 256)], gc.small_nvec(grid) % 256)
    assert set(gc.steps_and_blocks(n, ppt, 1 << 30)[0]) == {1}
    assert max(gc.small_n(g, f) for g in gc.GRIDS for f in F32) == 13589


def test_steps_and_blocks_on_hand_counted_sizes():
    assert gc.steps_and_blocks(0, 2, 4) == ([], 0)
    assert gc.steps_and_blocks(1, 2, 4) == ([1], 1)
    assert gc.steps_and_blocks(512, 2, 4) == ([1], 256)
    assert gc.steps_and_blocks(513, 2, 4) == ([1, 1], 257)
    assert gc.steps_and_blocks(1537, 2, 1) == ([4], 1)          # 769 vectors: 256 + 256 + 256 + 1
    assert gc.steps_and_blocks(3073, 4, 1) == ([4], 1)
    assert gc.steps_and_blocks(4 * 1024 + 1, 4, 2) == ([3, 2], 1)
    assert gc.where(2 * (512 + 256 + 65) + 1, 2, 2) == (1, 1, 1, 1, 1)


@pytest.mark.parametrize("f32", F32, ids=IDS)
@pytest.mark.parametrize("cus", gc.CU_COUNTS)
def test_cap_sizes_fill_the_production_grids_and_go_on(cus, f32):
    ppt = gc.PPT[f32]
    n = gc.cap_n(cus, f32)
    assert (n - 1) % ppt == 0
    # reduce passes at two blocks per CU: full grid, then one full block and one of 70 lanes
    steps, last = gc.steps_and_blocks(n, ppt, 2 * cus)
    assert len(steps) == 2 * cus and steps == [2, 2] + [1] * (2 * cus - 2) and last == 326
    assert gc.last_step_blocks(n, ppt, 2 * cus) == (1, 70, 2 * cus - 2)
    # moments passes (and the weighted reduce pass with f32 planes) at one block per CU: three steps
    steps, last = gc.steps_and_blocks(n, ppt, cus)
    assert len(steps) == cus and max(steps) == (3 if cus > 1 else 4) and last % 256 == 70
    # the passes without a reduction stay below their cap of eight blocks per CU
    assert (n + ppt - 1) // ppt <= 256 * 8 * cus
    # the score pass at 2, 3 or 4 blocks per CU
    n = gc.score_cap_n(cus, f32)
    assert (n - 1) % ppt == 0
    for occ in (2, 3, 4):
        steps, last = gc.steps_and_blocks(n, ppt, occ * cus)
        assert len(steps) == occ * cus and max(steps) >= 2 and min(steps) >= 1 and last % 256 == 70
    if cus == 256:
        assert (gc.cap_n(cus, False), gc.cap_n(cus, True)) == (262795, 525589)


@pytest.mark.parametrize("f32", F32, ids=IDS)
def test_planted_rows_fall_where_the_gpu_test_says(f32):
    ppt, g = gc.PPT[f32], gc.ZERO_GRID
    z = gc.zero_case(f32)
    assert z.n == gc.small_n(g, f32) and len(z.rows) == 14 and set(z.kinds) == set(range(len(gc.ZERO_KINDS)))
    at = {name: [gc.where(m, ppt, g) for m in rows] for name, rows in z.where.items()}
    first_last = at["first and last lane of every wave of block 0 in step 1"]
    assert [(s, b, w, l) for s, b, w, l, _ in first_last] == [(0, 0, w, l) for w in range(4) for l in (0, 63)]
    assert len({h for *_, h in first_last}) == ppt                                   # every slot of a vector among them
    assert [(s, b) for s, b, *_ in at["a lane of the last block"]] == [(0, g - 1)]
    (s1, b1, w1, l1, h1), (s2, b2, w2, l2, h2) = at["both matches of one vector"]
    assert (s1, b1, w1, l1) == (s2, b2, w2, l2) and (h1, h2) == (0, ppt - 1) and b1 == 1
    # step 3: block g - 2 holds one full wave and six lanes of the next
    assert gc.last_step_blocks(z.n, ppt, g) == (g - 2, 70, 1)
    assert [(s, b, w) for s, b, w, *_ in at["the partial wave of the ragged step"]] == [(2, g - 2, 1)] * 2
    assert all(l < 6 for _, _, _, l, _ in at["the partial wave of the ragged step"])
    assert z.where["the very last match"] == [z.n - 1] and at["the very last match"] == [(2, g - 2, 1, 5, 0)]
    # the long-double reference and float64 in the product's formulation call exactly these rows weightless
    X, y = gc.zero_planes(z, f32)
    with np.errstate(all="ignore"):
        _, zero = wr.info_matrices(X, y, z.cov, z.rot_w, z.tran_w, wr.COV_SCALE, z.bearing_sigma)
        _, _, zero64 = wr.basis_factor(X, y, z.cov, z.rot_w, z.tran_w, wr.COV_SCALE, z.bearing_sigma)
    assert np.array_equal(np.flatnonzero(zero), z.rows) and np.array_equal(zero, zero64)


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def _qualify_eval(n, f32, deltas):
    for delta in deltas:
        X, y = rr.planes(gc.eval_scene(n, delta > 0), f32)
        ref = gc.eval_reference(n, f32, delta)
        f64 = rr.sums(X, y, *gc.eval_pose(n), delta, np.float64)
        assert_normal_eq_close(f64, ref, REL_TOL_F64, f"eval n={n} delta={delta}")
        # no match on the Huber threshold: either precision counts the same outliers
        assert (f64.n_outlier, f64.n_behind) == (ref.n_outlier, ref.n_behind) and abs(f64.sum_w - ref.sum_w) <= REL_TOL_F64 * ref.sum_w
        if delta > 0:
            assert ref.n_outlier >= len(rr.planted(n)) and 0 < ref.sum_w < n
        else:
            assert ref.sum_w == n and ref.n_outlier == 0


def _qualify_moments(n, f32):
    X, y = rr.planes(gc.eval_scene(n, False), f32)
    ref = gc.moments_reference(n, f32)
    assert np.abs(rr.moments(X, y, np.float64) - ref).max() <= REL_TOL_F64 * float(np.abs(ref).max()), n


def _qualify_depths(n, f32):
    X, y = rr.planes(gc.eval_scene(n, False), f32)
    d = rr.per_match(X, y, *gc.eval_pose(n), np.float64)[1]
    assert np.abs(d - gc.depths_reference(n, f32)).max() <= REL_TOL_F64 * np.abs(X).max(), n


def _qualify_weighted(n, f32, deltas):
    for delta in deltas:
        err = wh._qualify(gc.weighted_case(n, delta), f32)          # the bound, no zero weight, the margin to delta^2
        assert 0 < err <= _row_bound(), (n, delta, err, _row_bound())


def _qualify_scores(n, f32, count):
    ref, amb = gc.score_reference(n, f32, count)
    assert amb.max() == 0 and len(ref) == count, (n, amb)
    assert ref[0] > 0.5 * n and ref.min() < 0.1 * n                 # the counts run from most matches down to nearly none


def _qualify_refit(n, f32):
    """Among the 128 trials one that draws no wrong match and whose pose makes exactly the rows that are not planted inliers, with
    none of the n near the threshold: the device's pick then has len(good) inliers and its refit is the DLT of those rows."""
    s = cr.exact_scene(n)
    X, y = rr.planes(s, f32)
    good = cr.inlier_rows(n)
    st, rot, tran, cond, idx = cr.harness_trials(n, f32, seed=REFIT_SEED, trials=REFIT_TRIALS, noisy=False)
    clean = np.flatnonzero((st == 0) & np.isin(idx, good).all(axis=1))
    assert len(clean) >= 4
    is_good = np.zeros(n, dtype=bool)
    is_good[good] = True
    for t in clean[np.argsort(-cond[clean])]:                       # the best-conditioned first
        sq = cr.sq_residuals(X, y, rot[t], tran[t])
        t2 = cr.LD(gc.REFIT_TAU) ** 2
        if np.array_equal(sq <= t2, is_good) and not (np.abs(sq - t2) <= cr.LD(cr.AMBIGUITY) * t2).any():
            break
    else:
        raise AssertionError(f"n={n} f32={f32}: no trial whose inliers are the {len(good)} rows that are not planted")
    lam = gc.refit_reference(n, f32).lam
    assert lam[1] / lam[11] >= 1e-5


@pytest.mark.parametrize("f32", F32, ids=IDS)
@pytest.mark.parametrize("grid", gc.GRIDS)
def test_scenes_at_the_small_grids(grid, f32):
    n = gc.small_n(grid, f32)
    _qualify_eval(n, f32, (0.0, gc.EVAL_DELTA))
    _qualify_moments(n, f32)
    _qualify_depths(n, f32)
    _qualify_weighted(n, f32, (0.0, wr.DELTA))
    _qualify_scores(n, f32, gc.SCORE_COUNT)
    _qualify_refit(n, f32)


@pytest.mark.parametrize("f32", F32, ids=IDS)
def test_zero_weight_scene(f32):
    z = gc.zero_case(f32)
    X, y = gc.zero_planes(z, f32)
    live = z.live
    ref, M = gc.zero_reference(f32)
    W, _, zero64 = wr.basis_factor(X[live], y[live], z.cov[live], z.rot_w, z.tran_w, wr.COV_SCALE, z.bearing_sigma)
    assert not zero64.any()
    got = wr.basis_sums(X[live], y[live], W, zero64, z.rot, z.tran, z.delta)
    assert_normal_eq_close(got, ref, REL_TOL_F64, "zero weight")
    assert (got.n_outlier, got.n_behind) == (ref.n_outlier, ref.n_behind) and ref.n_outlier >= 1
    assert np.abs(ref.s - z.delta ** 2).min() > wr.MARGIN * z.delta ** 2
    assert 0 < wr.row_error(wr.basis_rows(W), M) <= _row_bound()


@pytest.mark.parametrize("f32", F32, ids=IDS)
@pytest.mark.parametrize("cus", gc.CU_COUNTS)
def test_scenes_at_the_production_caps(cus, f32):
    n = gc.cap_n(cus, f32)
    _qualify_eval(n, f32, (gc.EVAL_DELTA,))
    _qualify_moments(n, f32)
    _qualify_weighted(n, f32, (wr.DELTA,))
    _qualify_refit(n, f32)
    _qualify_scores(gc.score_cap_n(cus, f32), f32, gc.CAP_SCORE_COUNT)
