"""Shared by tests/test_resection_grid_cases_cpu.py and tests/test_gpu_resection_grids.py (tests/ only): the sizes at which the
nine resection kernels take several grid-stride steps on several blocks, and the scenes run at them.  No algebra of its own:
scenes, candidates, covariances and long-double references are those of tests/resection_reference.py,
tests/resection_consensus_reference.py and tests/resection_weighted_reference.py.

All nine kernels run 256-thread blocks over 16-byte vectors, PPT matches per lane (2 with f64 planes, 4 with f32), a grid of
min(blocks, cap) blocks and a stride of 256 * grid vectors.

SMALL CAPPED GRIDS (SBA_RESECT_GRID = G in GRIDS): nvec = 2 * 256 G + 256 max(G - 2, 0) + 70 vectors, so that two full steps
are followed by a third with G - 2 full blocks, one block of one full wave plus six lanes, and at least one idle block;
n = PPT nvec - (PPT - 1) leaves a single match in the last vector.

PRODUCTION CAPS (no switch; sizes from the device's CU count): nvec = 256 * 2 CUs + 326 fills the 2-per-CU grid of the reduce
passes and adds a second step of one full block and one of 70 lanes (three steps at the one block per CU of the moments passes
and of the weighted reduce pass with f32 planes); nvec = 256 * 4 CUs + 326 gives the score pass at least two steps at 2, 3 or 4
blocks per CU.  The 8-per-CU cap of the three passes without a reduction is not reached: the small capped grids show all it
could."""
from dataclasses import dataclass
from functools import lru_cache

import numpy as np

import resection_consensus_reference as cr
import resection_reference as rr
import resection_weighted_reference as wr

GRIDS = (2, 3, 5)
PPT = {False: 2, True: 4}                      # matches per lane, by f32
CU_COUNTS = (1, 8, 64, 256, 304)               # what the CPU qualification lets stand in for the device
EVAL_DELTA = 0.02                              # the Huber delta of the unweighted cases (tests/test_resection_host_cpu.py: LM_DELTA)
SCORE_COUNT = 65                               # candidates at the small grids: more than one counter register of a lane
CAP_SCORE_COUNT = 4                            # at the caps
REFIT_TAU = 1e-3                               # the consensus call on the noise-free scene (tests/test_gpu_resection_consensus.py)
ZERO_GRID = 3                                  # the zero-weight cases run at the size of this grid


def matches_of(nvec, f32):
    return PPT[f32] * nvec - (PPT[f32] - 1)


def small_nvec(grid):
    return 2 * 256 * grid + 256 * max(grid - 2, 0) + 70


def small_n(grid, f32):
    return matches_of(small_nvec(grid), f32)


def cap_n(cus, f32):
    """Reduce, weighted reduce, moments and inlier moments at their production grids."""
    return matches_of(256 * 2 * cus + 326, f32)


def score_cap_n(cus, f32):
    return matches_of(256 * 4 * cus + 326, f32)


def steps_and_blocks(n, ppt, grid):
    """-> (steps, last): steps[b] is the number of grid-stride steps block b of a grid capped at `grid` blocks takes over n
    matches at ppt per lane, and last the number of lanes (vectors) the last step of the longest-running blocks fills."""
    nvec = (n + ppt - 1) // ppt
    g = min((nvec + 255) // 256, grid)
    if g == 0:
        return [], 0
    stride = 256 * g
    steps = [max(0, -(-(nvec - 256 * b) // stride)) for b in range(g)]
    return steps, nvec - (max(steps) - 1) * stride


def last_step_blocks(n, ppt, grid):
    """-> (full, partial, idle): in the last step, the number of blocks with 256 lanes, the lane count of the one partly filled
    block (0: none) and the number of blocks with nothing to do."""
    steps, last = steps_and_blocks(n, ppt, grid)
    full, partial = divmod(last, 256)
    return full, partial, len(steps) - full - (1 if partial else 0)


def where(match, ppt, grid):
    """-> (step, block, wave, lane in wave, slot in vector) of a match under a grid of `grid` blocks."""
    v, h = divmod(match, ppt)
    step, rest = divmod(v, 256 * grid)
    block, lane = divmod(rest, 256)
    return step, block, lane // 64, lane % 64, h


# ---- scenes -------------------------------------------------------------------------------------------------------------------
def eval_scene(n, with_outliers):
    """The unweighted evaluation: tests/test_gpu_resection.py's scenes, 8 % wrong matches where the loss is on."""
    return rr.make_scene(n, 500 + n, noise=1e-3, outliers=rr.planted(n) if with_outliers else ())


def eval_pose(n):
    return rr.start_near(eval_scene(n, False), n)


@lru_cache(maxsize=None)
def eval_reference(n, f32, delta):
    """Long-double sums of eval_scene(n, delta > 0) on what the planes hold at eval_pose(n); computed once, shared."""
    X, y = rr.planes(eval_scene(n, delta > 0), f32)
    return rr.sums(X, y, *eval_pose(n), delta)


@lru_cache(maxsize=None)
def moments_reference(n, f32):
    ref = rr.moments(*rr.planes(eval_scene(n, False), f32))
    ref.setflags(write=False)
    return ref


@lru_cache(maxsize=None)
def depths_reference(n, f32):
    d = rr.per_match(*rr.planes(eval_scene(n, False), f32), *eval_pose(n))[1]
    d.setflags(write=False)
    return d


@lru_cache(maxsize=None)
def weighted_case(n, delta):
    """tests/resection_weighted_reference.py's case at n: reference pose 0.004 and evaluation pose 0.002 from the truth, 8 % wrong
    matches where the loss is on, bearing noise 1e-3."""
    return wr._case(f"grid n={n} delta={delta}", wr.eval_scene(n, delta > 0), n, delta, 1e-3)


@lru_cache(maxsize=None)
def weighted_reference(n, f32, delta):
    """-> (long-double sums, M (n, 3, 3), zero mask) of weighted_case(n, delta); computed once, shared."""
    return wr.case_reference(weighted_case(n, delta), f32)


def score_reference(n, f32, count):
    """Long-double (inliers, ambiguous) of the first `count` candidates of tests/resection_consensus_reference.py on its scene."""
    return cr.score_reference(n, f32, count)


@lru_cache(maxsize=None)
def refit_reference(n, f32):
    """The numpy DLT over the rows of cr.exact_scene(n) that are not planted, on what the planes hold."""
    X, y = rr.planes(cr.exact_scene(n), f32)
    good = cr.inlier_rows(n)
    return rr.dlt(rr.moments(X[good], y[good]).astype(np.float64))


# ---- planted zero weights -----------------------------------------------------------------------------------------------------
ZERO_KINDS = ("infinite variances", "a NaN entry", "a zero covariance, no bearing noise", "a negative variance", "a zero bearing")


@dataclass(frozen=True)
class ZeroCase:
    n: int
    y: np.ndarray              # bearings with the zero bearings planted
    cov: np.ndarray            # (n, 6) with the bad rows planted
    rows: np.ndarray           # the planted matches, ascending
    kinds: tuple               # kinds[k]: index into ZERO_KINDS of rows[k]
    where: dict                # name of the position -> the matches planted there
    rot_w: np.ndarray
    tran_w: np.ndarray
    rot: np.ndarray
    tran: np.ndarray
    delta: float
    bearing_sigma: float

    @property
    def scene(self):
        return wr.eval_scene(self.n, True)

    @property
    def live(self):
        return np.setdiff1d(np.arange(self.n), self.rows)


def zero_positions(f32):
    """Where the rows of zero weight go at the size of ZERO_GRID, by name (positions under SBA_RESECT_GRID = ZERO_GRID)."""
    ppt, g = PPT[f32], ZERO_GRID
    nvec = small_nvec(g)
    stride = 256 * g
    ragged = 2 * stride + 256 * (g - 2)                    # the first vector of the partly filled block in step 3
    return {
        "first and last lane of every wave of block 0 in step 1": [ppt * (64 * w + l) + (2 * w + (l > 0)) % ppt for w in range(4) for l in (0, 63)],
        "a lane of the last block": [ppt * (256 * (g - 1) + 100) + 1],
        "both matches of one vector": [ppt * 300, ppt * 300 + ppt - 1],
        "the partial wave of the ragged step": [ppt * (ragged + 64), ppt * (ragged + 68) + 1],
        "the very last match": [ppt * (nvec - 1)],
    }


@lru_cache(maxsize=None)
def zero_case(f32):
    """tests/test_gpu_resection_weighted.py's zero-weight rows (test_zero_weight), each kind in turn over zero_positions(f32);
    bearing_sigma = 0, so that every kind is without weight."""
    n = small_n(ZERO_GRID, f32)
    s = wr.eval_scene(n, True)
    pos = zero_positions(f32)
    rows = np.array(sorted(m for v in pos.values() for m in v))
    assert len(set(rows.tolist())) == len(rows) and rows[-1] == n - 1
    cov, _ = wr.landmark_cov(s.X, n)
    cov, y = cov.copy(), s.y.copy()
    kinds = []
    for k, m in enumerate(rows):
        kind = k % len(ZERO_KINDS)
        kinds.append(kind)
        if kind == 0:
            cov[m] = [np.inf, np.inf, np.inf, 0, 0, 0]
        elif kind == 1:
            cov[m, 4] = np.nan
        elif kind == 2:
            cov[m] = 0.0
        elif kind == 3:
            cov[m, :3] = -cov[m, :3]
        else:
            y[m] = 0.0
    rw, tw = rr.start_near(s, n + 1000, 0.004, 0.004)
    re, te = rr.start_near(s, n, 0.002, 0.002)
    for a in (cov, y, rows):
        a.setflags(write=False)
    return ZeroCase(n, y, cov, rows, tuple(kinds), pos, rw, tw, re, te, wr.DELTA, 0.0)


def zero_planes(z, f32):
    """What the planes hold of a zero case: (X, y), f32-rounded with f32 planes."""
    X, _ = rr.planes(z.scene, f32)
    return X, (z.y.astype(np.float32).astype(np.float64) if f32 else z.y)


@lru_cache(maxsize=None)
def zero_reference(f32):
    """-> (long-double sums over the live rows, M of the live rows) of zero_case(f32), as test_zero_weight takes them."""
    z = zero_case(f32)
    X, y = zero_planes(z, f32)
    live = z.live
    M, zero = wr.info_matrices(X[live], y[live], z.cov[live], z.rot_w, z.tran_w, wr.COV_SCALE, z.bearing_sigma)
    assert not zero.any()
    return wr.sums(X[live], y[live], M, zero, z.rot, z.tran, z.delta), M
