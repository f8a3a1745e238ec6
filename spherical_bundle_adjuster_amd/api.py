"""Host-side Python mirror of the C-ABI (thin; the C++ mirror of the reference class lives in
``csrc/spherical_bundle_adjuster.hpp``).  Names follow the reference's domain: a *problem* holds
one shard of *correspondences* (matched key-points as unit vectors), a *sweep* is one residual +
Jacobian evaluation over them, the *solve stage* is the LM loop of ``solve_problem``
(reference spherical_bundle_adjuster.cpp:183-217)."""
from __future__ import annotations

import ctypes as C
import time
from dataclasses import dataclass
from typing import NamedTuple

import numpy as np

from . import _cabi as cabi
from ._cabi import (DEPTH_PER_MATCH, DEPTH_UNIFORM, KERNEL_EXPLICIT, KERNEL_FACTORED, MODE_ROT, MODE_RT, MODE_TRAN, STORE_F32,  # noqa: F401
                    STORE_F64, TRAN_FREE, TRAN_SPHERE, SbaError)


@dataclass
class NormalEquations:
    H: np.ndarray          # (6, 6) sum rho' J^T J over [rot | tran]
    g: np.ndarray          # (6,)   sum rho' J^T e
    cost: float            # 1/2 sum rho
    sum_w: float
    n_outlier: float


@dataclass
class JointEquations:
    """One reduce pass of the joint solve (Problem.eval_joint), parameter order [rot | tran], unscaled camera side."""
    S: np.ndarray          # (6, 6) reduced camera system sum (w F^T F - W^T U^-1 W) at the given depth damping
    gs: np.ndarray         # (6,)   reduced gradient
    V: np.ndarray          # (6, 6) unreduced camera block = eval(MODE_RT, DEPTH_PER_MATCH).H
    gc: np.ndarray         # (6,)
    cost: float
    sum_w: float
    n_outlier: float
    gd_max: float          # max-norm of the depth gradient


@dataclass
class JointCovariance:
    """Covariance of the joint problem at a point (Problem.covariance_joint): the robustified, undamped problem in the
    tangent space of the gauge.  Multiply by sigma2 for residuals of unknown variance."""
    cov: np.ndarray                # (6, 6) over [rot | tran], rank dim
    depth_cov: np.ndarray | None   # (n, 3) var d1, var d2, cov(d1, d2) per match; (inf, inf, 0) for a degenerate match
    cost: float                    # over the used matches
    sum_w: float
    n_used: int
    n_degenerate: int
    dim: int                       # 5 with TRAN_SPHERE, 6 with TRAN_FREE
    dof: int                       # n_used - dim

    @property
    def sigma2(self) -> float:
        """2 cost / dof: the residual variance the fit itself suggests (nan without a degree of freedom)."""
        return 2.0 * self.cost / self.dof if self.dof != 0 else float("nan")


@dataclass
class JointStructure:
    """Triangulated landmarks at a point (Problem.structure_joint), in camera 2's frame: per match the midpoint of the two
    ray ends, its 3 x 3 covariance under the joint covariance (depth-camera cross blocks included) and the dimensionless score
    trace(cov) / |xyz|^2.  Unscaled like JointCovariance: multiply cov and score by sigma2.  A degenerate match keeps its xyz,
    has the cov row (inf, inf, inf, 0, 0, 0) and score inf."""
    xyz: np.ndarray                # (n, 3)
    cov: np.ndarray | None         # (n, 6): xx, yy, zz, xy, xz, yz
    score: np.ndarray | None       # (n,)
    pose: JointCovariance          # what covariance_joint(depths=False) returns at the same arguments, bit for bit

    def __getattr__(self, name):
        """cost, sum_w, n_used, n_degenerate, dim, dof and sigma2 read through to `pose`."""
        if name in ("cost", "sum_w", "n_used", "n_degenerate", "dim", "dof", "sigma2"):
            return getattr(self.pose, name)
        raise AttributeError(name)


@dataclass
class ResectionEquations:
    """One reduce pass of the resection (Problem.eval_resection): the six-parameter problem over [rot | tran] with the
    bearing's depth eliminated per match."""
    H: np.ndarray          # (6, 6) sum w [A | I]^T P [A | I]
    g: np.ndarray          # (6,)   sum w [A | I]^T r
    cost: float            # 1/2 sum rho(|r|^2)
    sum_w: float
    n_outlier: float
    n_behind: float        # matches whose eliminated depth is <= 0 (counted, otherwise treated like any other)


@dataclass
class ResectionCovariance:
    """The covariance of a resected pose (Problem.resection_covariance): the inverse of the weighted normal matrix at the point,
    with the weights as frozen.  Not scaled: sigma2 = 2 cost / dof is reported for the caller to judge (near 1 when the landmark
    covariances and the bearing sigma are honest) or to apply."""
    cov: np.ndarray        # (6, 6) over [rot | tran]
    cost: float
    sum_w: float
    n_used: int            # n - n_zero_weight
    n_zero_weight: int     # matches the freeze gave no weight
    n_outlier: float
    dof: int               # 2 n_used - 6
    sigma2: float


@dataclass
class LandmarkFusion:
    """What one Landmarks.fuse pass did: every observation falls into exactly one class, n_obs = n_skipped + n_behind + n_gated +
    n_fused.  skipped: a non-finite landmark or covariance, a covariance that is not positive definite across the bearing, a zero
    bearing, a non-finite result (chi2 is NaN there); behind: the eliminated depth is <= 0; gated: chi2 > chi2_gate."""
    n_obs: int
    n_skipped: int
    n_behind: int
    n_gated: int
    n_fused: int
    chi2: np.ndarray | None    # (m,) per observation, or None when not asked for


@dataclass
class LandmarkRegisterEquations:
    """One evaluation of the joint registration (Landmarks.eval_register): the six-parameter problem over [rot | tran] that is
    left when every observed landmark has been eliminated exactly at the pose."""
    H: np.ndarray          # (6, 6) sum J_w^T J_w, the Schur complement of the full Gauss-Newton matrix
    g: np.ndarray          # (6,)   sum J_w^T u, the exact gradient of the reduced cost
    cost: float            # 1/2 sum chi2
    n_used: int            # observations that entered the sums
    n_behind: int          # of which: the eliminated depth is <= 0 at the evaluation pose


@dataclass
class LandmarkRegistration:
    """What one Landmarks.register did: the frame's pose and its covariance from the joint solve, and the class of every
    observation as in LandmarkFusion (gated: chi2 at the SOLUTION > chi2_gate; such observations did take part in the solve)."""
    rot: np.ndarray        # (3,)
    tran: np.ndarray       # (3,)
    cov: np.ndarray        # (6, 6) over [rot | tran]
    summary: "SolveSummary"
    n_obs: int
    n_skipped: int
    n_behind: int
    n_gated: int
    n_fused: int
    n_used: int            # observations that entered the sums at the solution
    chi2: np.ndarray | None    # (m,) per observation at the solution, NaN where skipped, or None when not asked for


@dataclass
class LandmarkRobustRegisterEquations(LandmarkRegisterEquations):
    """One evaluation of the robust joint registration (Landmarks.eval_register_robust): H = sum w J_w^T J_w, g = sum w J_w^T u,
    cost = 1/2 sum rho(chi2) with the Huber loss on every landmark's chi2 and w = rho'."""
    n_outlier: int         # of the used observations: chi2 > huber_delta^2


@dataclass
class LandmarkRobustRegistration(LandmarkRegistration):
    """What one Landmarks.register_robust did: LandmarkRegistration under the Huber loss; cov = H_rho^-1.  With bearings on the
    device and chi2 asked for, chi2 is what the caller passed as chi2_device (the address), not an array."""
    n_outlier: int         # observations with chi2 > huber_delta^2 at the solution: all of them are gated


@dataclass
class LandmarkHampelRegisterEquations(LandmarkRobustRegisterEquations):
    """One evaluation of the joint registration under Hampel's redescending loss (Landmarks.eval_register_hampel) with the
    thresholds a = huber_delta < b < c on sqrt(chi2): weight 1 up to a, a / r up to b, falling to exactly 0 at c."""
    n_rejected: int        # of the used observations: chi2 > c^2, weight 0


@dataclass
class LandmarkHampelRegistration(LandmarkRobustRegistration):
    """What one Landmarks.register_hampel did: LandmarkRobustRegistration under Hampel's loss; cov = H_rho^-1, in which a rejected
    observation does not count at all."""
    n_rejected: int        # observations with chi2 > c^2 at the solution
    rot_huber: np.ndarray  # (3,) the Huber stage's minimiser (huber_first), else the start pose
    tran_huber: np.ndarray # (3,)
    huber_iterations: int  # LM iterations of the Huber stage, 0 without it


@dataclass
class LandmarkPrune:
    """What one Landmarks.prune did: every landmark falls into exactly one class, tested in this order, n_before = n_invalid +
    n_uncertain + n_unobserved + n_masked + n_kept.  invalid: a non-finite entry of X or Sigma or a negative variance; uncertain:
    not (score <= max_score); unobserved: count < min_count; masked: the caller's mask is 0 there."""
    n_before: int
    n_invalid: int
    n_uncertain: int
    n_unobserved: int
    n_masked: int
    n_kept: int
    kept: np.ndarray | None    # (n_kept,) int64, the old indices of the kept landmarks, ascending, or None when not asked for


@dataclass
class LandmarkAssociation:
    """What one Landmarks.associate found.  Frame row j is accepted iff the matcher gives it two neighbours, d0 < ratio * d1 in
    float32 and d0 <= max_distance in float32; a landmark's winner is its claimant smallest in (bits of d0, j); the outputs list
    the claimed landmarks in ascending order.  n_accepted = n_contested + n_associated."""
    n_frame: int
    n_accepted: int
    n_contested: int
    n_associated: int
    idx: np.ndarray                # (n_associated,) int64, strictly increasing: what register* takes as idx
    rows: np.ndarray               # (n_associated,) int32: the winning frame row per landmark, no repeats
    distance: np.ndarray           # (n_associated,) float32: the winner's d0
    bearings: np.ndarray | None    # (n_associated, 3) float64 = frame_bearings[rows] bit for bit; None without frame bearings or
    #                                when they went to device memory


@dataclass
class ResectionGuess:
    """The linear starting point of the resection (Problem.resection_guess) and what its moment matrix says about it."""
    rot: np.ndarray        # (3,)
    tran: np.ndarray       # (3,)
    lambda1: float         # smallest eigenvalue of the 12 x 12 moment matrix (0 on exact data)
    lambda2: float         # the next: lambda2 / lambda12 near rounding level = a scene that does not fix the pose
    lambda12: float        # the largest
    sv: np.ndarray         # (3,) singular values of the rotation part over their mean: (1, 1, 1) on exact data
    scale: float
    n: int
    n_behind: float        # at (rot, tran)
    moments: np.ndarray | None   # (60,) the sums, if asked for


@dataclass
class ResectionConsensus:
    """The robust starting point of the resection (Problem.resection_guess_consensus): the best of the sampled DLT trials by
    its inlier count over all matches, or the linear refit over that trial's inliers."""
    rot: np.ndarray        # (3,)
    tran: np.ndarray       # (3,)
    n: int
    n_inlier: int          # matches within the threshold at (rot, tran)
    best_trial: int
    best_trial_inliers: int
    n_valid_trials: int    # trials whose DLT finish did not refuse
    refit_used: bool       # (rot, tran) is the refit, not the best trial itself
    refit: ResectionGuess | None   # the refit's finish (rot, tran, n_behind and moments not filled: zeros / None); None if not asked for
    n_behind: float        # at (rot, tran)
    trial_inliers: np.ndarray | None   # (trials,) int64, -1 = the trial refused; with per_trial
    trial_rot: np.ndarray | None       # (trials, 3)
    trial_tran: np.ndarray | None      # (trials, 3)


@dataclass
class BatchJointCovariance:
    """Covariance of every pair's joint problem (Batch.covariance_joint).  A pair with status != 0 has no covariance: its cov
    and its depth_cov rows are NaN.  Multiply a pair's blocks by its sigma2 for residuals of unknown variance."""
    cov: np.ndarray                # (B, 6, 6) over [rot | tran], rank dim
    depth_cov: np.ndarray | None   # (offsets[-1], 3) indexed like the uploaded d12; (inf, inf, 0) for a degenerate match
    cost: np.ndarray               # (B,) over the used matches
    sum_w: np.ndarray              # (B,)
    n_used: np.ndarray             # (B,) int64
    n_degenerate: np.ndarray       # (B,) int64
    dim: np.ndarray                # (B,) int32
    dof: np.ndarray                # (B,) int32: n_used - dim
    status: np.ndarray             # (B,) int32: 0 or SBA_ERR_NUMERIC
    offsets: np.ndarray            # (B + 1,) first depth_cov row of every pair

    @property
    def sigma2(self) -> np.ndarray:
        """(B,) 2 cost / dof per pair (nan without a degree of freedom)."""
        dof = np.asarray(self.dof, dtype=np.float64)
        out = np.full(dof.shape, np.nan)
        np.divide(2.0 * np.asarray(self.cost, dtype=np.float64), dof, out=out, where=dof != 0)
        return out

    def pair(self, g: int) -> JointCovariance:
        """Pair g's slice as the single-problem result type."""
        g = int(g)
        lo, hi = int(self.offsets[g]), int(self.offsets[g + 1])
        return JointCovariance(self.cov[g], None if self.depth_cov is None else self.depth_cov[lo:hi], float(self.cost[g]),
                               float(self.sum_w[g]), int(self.n_used[g]), int(self.n_degenerate[g]), int(self.dim[g]), int(self.dof[g]))


@dataclass
class BatchJointStructure:
    """Triangulated landmarks of every pair (Batch.structure_joint): JointStructure's arrays for all pairs, rows indexed like
    the uploaded d12 (pair g's rows are offsets[g] .. offsets[g + 1]).  A pair with status != 0 has no covariance: its rows are
    NaN in every output, xyz included.  Unscaled: multiply a pair's cov and score by its sigma2."""
    xyz: np.ndarray | None         # (offsets[-1], 3)
    cov: np.ndarray | None         # (offsets[-1], 6): xx, yy, zz, xy, xz, yz
    score: np.ndarray | None       # (offsets[-1],)
    pose: BatchJointCovariance     # what covariance_joint(depths=False, check=False) returns at the same arguments, bit for bit

    def __getattr__(self, name):
        """offsets, status, cost, sum_w, n_used, n_degenerate, dim, dof and sigma2 read through to `pose`."""
        if name in ("offsets", "status", "cost", "sum_w", "n_used", "n_degenerate", "dim", "dof", "sigma2"):
            return getattr(self.pose, name)
        raise AttributeError(name)

    def pair(self, g: int) -> JointStructure:
        """Pair g's slice as the single-problem result type."""
        g = int(g)
        lo, hi = int(self.pose.offsets[g]), int(self.pose.offsets[g + 1])
        cut = lambda a: None if a is None else a[lo:hi]
        return JointStructure(cut(self.xyz), cut(self.cov), cut(self.score), self.pose.pair(g))


@dataclass
class SolveSummary:
    termination: str
    num_iterations: int
    num_successful_steps: int
    num_evaluations: int
    initial_cost: float
    final_cost: float
    final_gradient_max_norm: float
    final_radius: float
    seconds_total: float
    seconds_eval: float
    num_line_search_steps: int = 0


class Residuals(NamedTuple):
    """Per-match residuals of a problem (Problem.residuals); a field that was not requested is None."""
    e: np.ndarray | None          # (n, 3) e = d2 x2 - d1 R x1 + t
    sq_norm: np.ndarray | None    # (n,)   e.e
    inlier: np.ndarray | None     # (n,)   bool: inside Huber's quadratic region (NaN residuals count as inliers)
    n_inlier: int


class BatchResiduals(NamedTuple):
    """Per-match residuals of a batch (Batch.residuals), rows in the order of Batch.offsets; a field that was not requested
    is None."""
    e: np.ndarray | None          # (rows, 3)
    sq_norm: np.ndarray | None    # (rows,)
    inlier: np.ndarray | None     # (rows,) bool
    n_inlier: np.ndarray          # (num_pairs,) int64: inliers per pair


def _f64(a, shape=None) -> np.ndarray:
    a = np.ascontiguousarray(a, dtype=np.float64)
    if shape is not None and a.shape != shape:
        raise ValueError(f"expected shape {shape}, got {a.shape}")
    return a


def _dptr(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_double))


class Matches(NamedTuple):
    """Result of match_descriptors: exact L2 2-NN of every query row and the reference's ratio test."""
    nn_index: np.ndarray      # (n_query, 2) int32: nearest, second nearest train row; -1 = none
    nn_distance: np.ndarray   # (n_query, 2) float32: their Euclidean distances (DMatch::distance); +inf = none
    query_idx: np.ndarray     # (n_matched,) int32: accepted queries, ascending (queryIdx)
    train_idx: np.ndarray     # (n_matched,) int32: their nearest train row (trainIdx)
    distance: np.ndarray      # (n_matched,) float32


class BatchMatches(NamedTuple):
    """Result of batch_match_descriptors; indices are local to the pair, pair g's matches are rows
    match_offsets[g] .. match_offsets[g + 1] of query_idx / train_idx / distance."""
    nn_index: np.ndarray      # (total queries, 2) int32
    nn_distance: np.ndarray   # (total queries, 2) float32
    n_matched: np.ndarray     # (num_pairs,) int64
    match_offsets: np.ndarray  # (num_pairs + 1,) int64: exclusive scan of n_matched
    query_idx: np.ndarray
    train_idx: np.ndarray
    distance: np.ndarray


def _descriptors(*arrays):
    """f32 (n, dim) descriptor arrays -> (arrays, row stride in bytes).  Rows may be padded (a view of a wider array, like a
    cv::Mat with a larger step) as long as every array has the same row stride; otherwise they are made contiguous."""
    out = []
    for a in arrays:
        a = np.asarray(a)
        if a.ndim != 2:
            raise ValueError("descriptors must be 2-D (n, dim)")
        if a.dtype != np.float32 or a.strides[1] != 4 or a.strides[0] % 4 or a.strides[0] < 4 * a.shape[1]:
            a = np.ascontiguousarray(a, dtype=np.float32)
        out.append(a)
    dims = {a.shape[1] for a in out}
    if len(dims) != 1:
        raise ValueError("descriptor dimensions differ")
    dim = dims.pop()
    strides = {a.strides[0] for a in out if a.shape[0] > 1}
    if len(strides) > 1:
        out = [np.ascontiguousarray(a) for a in out]
        strides = {4 * dim}
    stride = strides.pop() if strides else 4 * dim
    return out, dim, max(stride, 4 * dim)


def _vptr(a: np.ndarray):
    return C.c_void_p(a.ctypes.data) if a.size else None


def _offsets(o, name):
    off = np.ascontiguousarray(o, dtype=np.uint64)
    if off.ndim != 1 or off.size < 1:
        raise ValueError(f"{name} offsets must be 1-D with num_pairs + 1 entries")
    return off


def quantile_rank(probs, n: int) -> np.ndarray:
    """The 0-based rank floor(p * (n - 1)) of each probability 0 <= p <= 1 among n > 0 values, formed in float64: p = 0 is
    the minimum, p = 1 the maximum, and no interpolation between neighbours takes place."""
    p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
    if n < 1:
        raise ValueError("quantiles of an empty set")
    if not np.all((p >= 0.0) & (p <= 1.0)):
        raise ValueError("probabilities must lie in [0, 1]")
    return np.floor(p * np.float64(n - 1)).astype(np.uintp)


def _ranks(r) -> np.ndarray:
    a = np.asarray(r)
    if a.size and (not np.issubdtype(a.dtype, np.integer) or a.min() < 0):
        raise ValueError("ranks must be non-negative integers")
    return np.ascontiguousarray(np.atleast_1d(a), dtype=np.uintp)


def device_count() -> int:
    lib = cabi.load_library()
    n = C.c_int(0)
    cabi.check(lib, lib.sba_device_count(C.byref(n)))
    return n.value


def default_lm_options(**overrides) -> cabi.LmOptions:
    lib = cabi.load_library()
    o = cabi.LmOptions()
    lib.sba_lm_options_default(C.byref(o))
    for k, v in overrides.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def expand_pack(mode: int, pack) -> NormalEquations:
    lib = cabi.load_library()
    pack = _f64(pack, (cabi.PACK_SIZE,))
    ne = cabi.NormalEq()
    cabi.check(lib, lib.sba_expand_pack(mode, _dptr(pack), C.byref(ne)))
    return _to_ne(ne)


def _to_ne(ne: cabi.NormalEq) -> NormalEquations:
    return NormalEquations(np.array(ne.H, dtype=np.float64).reshape(6, 6), np.array(ne.g, dtype=np.float64),
                           float(ne.cost), float(ne.sum_w), float(ne.n_outlier))


def _summary(s: cabi.LmSummary) -> SolveSummary:
    return SolveSummary(cabi.TERMINATION.get(s.termination, str(s.termination)), s.num_iterations,
                        s.num_successful_steps, s.num_evaluations, s.initial_cost, s.final_cost,
                        s.final_gradient_max_norm, s.final_radius, s.seconds_total, s.seconds_eval,
                        s.num_line_search_steps)


class Problem:
    """One shard of correspondences resident on one GPU (``sba_problem``)."""

    def __init__(self, device: int = 0, stream: int | None = None, lib=None):
        self._lib = lib if lib is not None else cabi.load_library()
        self._h = C.c_void_p()
        cabi.check(self._lib, self._lib.sba_problem_create(C.byref(self._h), device, C.c_void_p(stream or 0)))
        self._hook_keepalive = None
        self.device = device

    # -- life cycle ---------------------------------------------------------------------------
    def close(self) -> None:
        """Destroy the handle.  `destroy_status` keeps the library's answer: non-zero means the handle was POISONED (a
        device wait timed out or the device faulted) and its device resources were leaked instead of freed -- the
        process should then exit non-zero; never raise from here, close() runs inside `with` blocks that are unwinding."""
        if getattr(self, "_h", None) is not None and self._h:
            self.destroy_status = int(self._lib.sba_problem_destroy(self._h))
            self._h = C.c_void_p()
            if self.destroy_status != 0:
                import warnings
                warnings.warn("sba_problem_destroy: " + cabi.last_error(self._lib), ResourceWarning, stacklevel=2)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data ------------------------------------------------------------------------------------
    def upload(self, left_xyz, right_xyz, d12=None, store: int = STORE_F64) -> None:
        """left_xyz/right_xyz: (n,3) f64 unit vectors (cv::Point3d layout); d12: (n,2) or None."""
        x1 = _f64(left_xyz).reshape(-1, 3)
        x2 = _f64(right_xyz).reshape(-1, 3)
        if x1.shape != x2.shape:
            raise ValueError("left/right shapes differ")
        n = x1.shape[0]
        dp = None
        if d12 is not None:
            d = _f64(d12).reshape(-1, 2)
            if d.shape[0] != n:
                raise ValueError("d12 length differs")
            dp = d.ctypes.data_as(C.c_void_p)
        cabi.check(self._lib, self._lib.sba_problem_upload(
            self._h, x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), dp, n, store))

    def upload_landmarks(self, xyz, bearings, store: int = STORE_F64) -> None:
        """The resection's data: landmarks xyz (n, 3) in the frame the pose maps from and the new frame's bearings (n, 3).
        Plain `upload` with left = xyz as given and d12 = (1, 1), so the landmark d1 * left is xyz exactly (with STORE_F32 the
        planes hold xyz rounded to f32).  For landmarks already on the device (structure_joint_into) use upload_device with
        the rows matched in the new frame as `left` and the caller's own d12, for example ones."""
        x = _f64(xyz).reshape(-1, 3)
        self.upload(x, bearings, np.ones((x.shape[0], 2)), store=store)

    def upload_keypoints(self, left_kp: np.ndarray, right_kp: np.ndarray, im_width: int, im_height: int, d12=None,
                         store: int = STORE_F64) -> None:
        """Matched cv::KeyPoint-like records (first two float32 = pt.x, pt.y) of both images -> device planes,
        pixel -> unit sphere computed on the device (reference .cpp:271-298)."""
        kl, kr = np.ascontiguousarray(left_kp), np.ascontiguousarray(right_kp)
        if kl.shape != kr.shape:
            raise ValueError("left/right key-point arrays differ")
        n = kl.shape[0]
        stride = kl.strides[0] if n > 0 else 28
        dp = None
        if d12 is not None:
            d = _f64(d12).reshape(-1, 2)
            if d.shape[0] != n:
                raise ValueError("d12 length differs")
            dp = d.ctypes.data_as(C.c_void_p)
        cabi.check(self._lib, self._lib.sba_problem_upload_keypoints(
            self._h, kl.ctypes.data_as(C.c_void_p), kr.ctypes.data_as(C.c_void_p), n, stride, im_width, im_height, dp,
            store))

    def upload_matches(self, left_kp: np.ndarray, right_kp: np.ndarray, left_desc, right_desc, im_width: int, im_height: int,
                       ratio: float = 0.3, init_depth: float | None = None, store: int = STORE_F64):
        """Match the descriptors of both images on the device (match_descriptors: left = query, right = train), then upload
        the matched key-point records as upload_keypoints would, with d12 = (init_depth, init_depth) per match if given.
        Key-point records and descriptor rows are one per key-point.  Returns (match_left, match_right): int32 indices."""
        kl, kr = np.ascontiguousarray(left_kp), np.ascontiguousarray(right_kp)
        if kl.ndim != 2 or kr.ndim != 2 or kl.dtype != kr.dtype or kl.shape[1] != kr.shape[1]:
            raise ValueError("left/right key-point records differ in layout")
        (dl, dr), dim, dstride = _descriptors(left_desc, right_desc)
        if dl.shape[0] != kl.shape[0] or dr.shape[0] != kr.shape[0]:
            raise ValueError("one descriptor row per key-point")
        stride = kl.strides[0] if kl.shape[0] > 0 else (kr.strides[0] if kr.shape[0] > 0 else 28)
        ml = np.zeros(max(kl.shape[0], 1), dtype=np.int32)
        mr = np.zeros(max(kl.shape[0], 1), dtype=np.int32)
        d = None if init_depth is None else (C.c_double * 1)(float(init_depth))
        n = C.c_size_t()
        cabi.check(self._lib, self._lib.sba_problem_upload_matches(
            self._h, _vptr(kl), kl.shape[0], _vptr(kr), kr.shape[0], stride, im_width, im_height, _vptr(dl), _vptr(dr), dim,
            dstride, ratio, d, store, C.byref(n), ml.ctypes.data_as(C.c_void_p), mr.ctypes.data_as(C.c_void_p)))
        return ml[:n.value].copy(), mr[:n.value].copy()

    def upload_device(self, left_ptr: int, right_ptr: int, d12_ptr: int | None, n: int,
                      store: int = STORE_F64) -> None:
        cabi.check(self._lib, self._lib.sba_problem_upload_device(
            self._h, C.c_void_p(left_ptr), C.c_void_p(right_ptr), C.c_void_p(d12_ptr or 0), n, store))

    def set_depths(self, d12) -> None:
        """(Re)upload only the per-match depths (n, 2) of the resident correspondences."""
        d = _f64(d12).reshape(-1, 2)
        if d.shape[0] != self.size:
            raise ValueError("d12 length differs from the uploaded correspondences")
        cabi.check(self._lib, self._lib.sba_problem_set_depths(self._h, d.ctypes.data_as(C.c_void_p)))

    def set_kernel(self, kind: int) -> None:
        """KERNEL_FACTORED (default) or KERNEL_EXPLICIT."""
        cabi.check(self._lib, self._lib.sba_problem_set_kernel(self._h, kind))

    def set_folding(self, on: bool) -> None:
        """Per-match-depth sweeps over f64 planes stream the depth-folded planes d1 x1, d2 x2 (True, default) or the
        raw planes (False).  Same results either way."""
        cabi.check(self._lib, self._lib.sba_problem_set_folding(self._h, 1 if on else 0))

    @property
    def size(self) -> int:
        n = C.c_size_t(0)
        cabi.check(self._lib, self._lib.sba_problem_size(self._h, C.byref(n)))
        return n.value

    # -- sweeps -----------------------------------------------------------------------------------
    def eval(self, mode, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM) -> NormalEquations:
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        ne = cabi.NormalEq()
        cabi.check(self._lib, self._lib.sba_problem_eval(self._h, mode, depth_mode, _dptr(rot), _dptr(tran),
                                                         d1, d2, huber_delta, C.byref(ne)))
        return _to_ne(ne)

    def eval_pack(self, mode, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        pack = np.zeros(cabi.PACK_SIZE)
        cabi.check(self._lib, self._lib.sba_problem_eval_pack(self._h, mode, depth_mode, _dptr(rot), _dptr(tran),
                                                              d1, d2, huber_delta, _dptr(pack)))
        return pack

    def eval_timed(self, mode, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM,
                   repeat: int = 10):
        """`repeat` back-to-back sweeps timed with HIP events on the problem's stream.
        Returns (pack, mean ms per step [sweep+finalize(+all-reduce)], mean ms of the sweep kernel alone)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        pack = np.zeros(cabi.PACK_SIZE)
        step_ms, sweep_ms = C.c_double(0), C.c_double(0)
        cabi.check(self._lib, self._lib.sba_problem_eval_timed(self._h, mode, depth_mode, _dptr(rot), _dptr(tran),
                                                               d1, d2, huber_delta, repeat, _dptr(pack),
                                                               C.byref(step_ms), C.byref(sweep_ms)))
        return pack, step_ms.value, sweep_ms.value

    def eval_launch_times(self, mode, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM,
                          repeat: int = 20) -> np.ndarray:
        """Device time (ms) of each of `repeat` back-to-back sweep-kernel launches (HIP event between every two)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        ms = np.zeros(repeat, dtype=np.float32)
        cabi.check(self._lib, self._lib.sba_problem_eval_launch_times(
            self._h, mode, depth_mode, _dptr(rot), _dptr(tran), d1, d2, huber_delta, repeat,
            ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms.astype(np.float64)

    def eval_steps(self, mode, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM, steps: int = 1):
        """`steps` host-synchronous sweeps in a row inside the library; returns (last pack, seconds of the loop)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        pack = np.zeros(cabi.PACK_SIZE)
        sec = C.c_double(0)
        cabi.check(self._lib, self._lib.sba_problem_eval_steps(self._h, mode, depth_mode, _dptr(rot), _dptr(tran),
                                                               d1, d2, huber_delta, steps, _dptr(pack), C.byref(sec)))
        return pack, sec.value

    # -- single matches ---------------------------------------------------------------------------------
    def residuals(self, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM,
                  fields=("e", "sq_norm", "inlier")) -> Residuals:
        """Per-match residuals at (rot, tran), formed on the device exactly as the sweep forms them.  `fields` picks the
        arrays copied back (any of "e", "sq_norm", "inlier"; empty = the inlier count only).  n - n_inlier equals the
        sweep's n_outlier at the same arguments."""
        unknown = set(fields) - {"e", "sq_norm", "inlier"}
        if unknown:
            raise ValueError(f"unknown residual fields {sorted(unknown)}")
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        n = self.size
        e = np.empty((n, 3)) if "e" in fields else None
        sq = np.empty(n) if "sq_norm" in fields else None
        inl = np.empty(n, dtype=np.uint8) if "inlier" in fields else None
        cnt = C.c_size_t(0)
        cabi.check(self._lib, self._lib.sba_problem_residuals(
            self._h, depth_mode, _dptr(rot), _dptr(tran), d1, d2, huber_delta,
            None if e is None else _dptr(e), None if sq is None else _dptr(sq),
            None if inl is None else inl.ctypes.data_as(C.c_void_p), C.byref(cnt)))
        return Residuals(e, sq, None if inl is None else inl.view(np.bool_), cnt.value)

    def compact(self, keep) -> np.ndarray:
        """Keep the matches where `keep` (length = size) is true, in order; the handle then equals a fresh upload of the
        kept matches.  Returns their original indices (np.int64)."""
        k = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint8)
        n = self.size
        if k.shape[0] != n:
            raise ValueError(f"keep has {k.shape[0]} entries, the problem holds {n} matches")
        idx = np.empty(n, dtype=np.int64)
        kept = C.c_size_t(0)
        cabi.check(self._lib, self._lib.sba_problem_compact(self._h, k.ctypes.data_as(C.c_void_p), C.byref(kept),
                                                            idx.ctypes.data_as(C.c_void_p)))
        return idx[:kept.value].copy()

    def keep_inliers(self, rot, tran, d1=1.0, d2=1.0, huber_delta=1.0, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        """Drop the matches in Huber's outlier region at (rot, tran): residuals() then compact().  Returns the original
        indices of the matches kept."""
        r = self.residuals(rot, tran, d1, d2, huber_delta, depth_mode, fields=("inlier",))
        return self.compact(r.inlier)

    def residual_order_stats(self, rot, tran, ranks, d1=1.0, d2=1.0, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        """The ranks[j]-th smallest (0-based) of the per-match squared residual norms at (rot, tran), selected on the device:
        each value is, bit for bit, an element of ``residuals(...).sq_norm``; nothing is interpolated.  Up to 8 ranks per
        call, each below `size`.  A NaN sorts above +inf."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        r = _ranks(ranks).reshape(-1)
        vals = np.empty(r.shape[0])
        cabi.check(self._lib, self._lib.sba_problem_residual_order_stats(
            self._h, depth_mode, _dptr(rot), _dptr(tran), d1, d2, r.ctypes.data_as(C.POINTER(C.c_size_t)), r.shape[0],
            _dptr(vals)))
        return vals

    def residual_quantiles(self, rot, tran, probs, d1=1.0, d2=1.0, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        """residual_order_stats at the ranks floor(p * (n - 1)) of the probabilities 0 <= p <= 1 (`quantile_rank`): the
        lower of the two neighbours where numpy's default quantile would interpolate."""
        return self.residual_order_stats(rot, tran, quantile_rank(probs, self.size), d1, d2, depth_mode)

    def keep_below(self, rot, tran, prob, scale, d1=1.0, d2=1.0, depth_mode=DEPTH_UNIFORM):
        """Keep the matches with sq_norm <= scale * (the `prob` quantile of sq_norm, as residual_quantiles), selected,
        flagged and compacted on the device; the handle then equals a fresh upload of the kept matches.  A NaN residual is
        dropped.  Returns (original indices of the kept matches (np.int64), the threshold).
        `scale` has no default on purpose: which multiple of which quantile separates outliers depends on the stage -- after
        the joint solve a residual keeps one effective degree of freedom, before it three -- so the choice is the caller's."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        n = self.size
        rank = int(quantile_rank(prob, n).reshape(-1)[0])
        idx = np.empty(max(n, 1), dtype=np.int64)
        kept, thr = C.c_size_t(0), C.c_double(0.0)
        cabi.check(self._lib, self._lib.sba_problem_keep_below(
            self._h, depth_mode, _dptr(rot), _dptr(tran), d1, d2, rank, float(scale), C.byref(thr), C.byref(kept),
            idx.ctypes.data_as(C.c_void_p)))
        return idx[:kept.value].copy(), thr.value

    # -- solve stage --------------------------------------------------------------------------------
    def solve(self, mode, rot, tran, d1=1.0, d2=1.0, depth_mode=DEPTH_UNIFORM, options: cabi.LmOptions | None = None):
        """LM solve; returns (rot, tran, SolveSummary).  Inputs are not modified."""
        rot = _f64(rot, (3,)).copy()
        tran = _f64(tran, (3,)).copy()
        opt = options if options is not None else default_lm_options()
        s = cabi.LmSummary()
        cabi.check(self._lib, self._lib.sba_problem_solve(self._h, mode, depth_mode, _dptr(rot), _dptr(tran),
                                                          d1, d2, C.byref(opt), C.byref(s)))
        return rot, tran, _summary(s)

    def solve_depths(self, rot, tran, lam=1.0, c=1.0, options: cabi.LmOptions | None = None):
        """d-only stage: refines the uploaded per-match depths in place; returns (d12 (n,2), SolveSummary)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        out = np.zeros((self.size, 2))
        opt = options if options is not None else default_lm_options()
        s = cabi.LmSummary()
        cabi.check(self._lib, self._lib.sba_problem_solve_depths(self._h, _dptr(rot), _dptr(tran), lam, c,
                                                                 C.byref(opt), out.ctypes.data_as(C.c_void_p),
                                                                 C.byref(s)))
        return out, _summary(s)

    # -- joint solve: depths, rotation and translation together ---------------------------------------
    def eval_joint(self, rot, tran, radius=float("inf"), options: cabi.LmOptions | None = None) -> JointEquations:
        """One reduce pass of the joint solve at (rot, tran) and the handle's depths; `radius` sets the depth damping
        (inf: none).  options None = the defaults with tran_param = TRAN_SPHERE."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        eq = cabi.JointEq()
        cabi.check(self._lib, self._lib.sba_problem_eval_joint(self._h, _dptr(rot), _dptr(tran), float(radius),
                                                               None if options is None else C.byref(options), C.byref(eq)))
        a = lambda v, shape: np.array(v, dtype=np.float64).reshape(shape)
        return JointEquations(a(eq.S, (6, 6)), a(eq.gs, (6,)), a(eq.V, (6, 6)), a(eq.gc, (6,)), float(eq.cost), float(eq.sum_w),
                              float(eq.n_outlier), float(eq.gd_max))

    def solve_joint(self, rot, tran, options: cabi.LmOptions | None = None, return_depths: bool = True):
        """Joint LM over the handle's per-match depths and the camera from (rot, tran): the reference's joint functor.  The
        refined depths stay in the handle.  options None = the defaults with tran_param = TRAN_SPHERE (|tran| pinned: the
        gauge of the problem).  Returns (rot, tran, d12 (n, 2) or None, SolveSummary); inputs are not modified."""
        rot = _f64(rot, (3,)).copy()
        tran = _f64(tran, (3,)).copy()
        out = np.zeros((self.size, 2)) if return_depths else None
        s = cabi.LmSummary()
        cabi.check(self._lib, self._lib.sba_problem_solve_joint(self._h, _dptr(rot), _dptr(tran),
                                                                None if options is None else C.byref(options), C.byref(s),
                                                                None if out is None else out.ctypes.data_as(C.c_void_p)))
        return rot, tran, out, _summary(s)

    def covariance_joint(self, rot, tran, options: cabi.LmOptions | None = None, min_sin2_parallax: float = 0.0,
                         depths: bool = True) -> JointCovariance:
        """Covariance of the joint problem at (rot, tran) and the handle's depths: the pose's 6 x 6 block and (depths=True)
        every match's own 2 x 2 depth block.  A match whose rays R x1 and x2 enclose an angle with sin^2 <=
        min_sin2_parallax is left out and reported as (inf, inf, 0).  options None = the defaults with tran_param =
        TRAN_SPHERE.  The handle's state is not touched."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        res = cabi.JointCov()
        dd = np.zeros((self.size, 3)) if depths else None
        cabi.check(self._lib, self._lib.sba_problem_covariance_joint(self._h, _dptr(rot), _dptr(tran),
                                                                     None if options is None else C.byref(options),
                                                                     float(min_sin2_parallax), C.byref(res),
                                                                     None if dd is None else _dptr(dd)))
        return JointCovariance(np.array(res.cov, dtype=np.float64).reshape(6, 6), dd, float(res.cost), float(res.sum_w),
                               int(res.n_used), int(res.n_degenerate), int(res.dim), int(res.dof))

    @staticmethod
    def _joint_cov(res) -> JointCovariance:
        return JointCovariance(np.array(res.cov, dtype=np.float64).reshape(6, 6), None, float(res.cost), float(res.sum_w),
                               int(res.n_used), int(res.n_degenerate), int(res.dim), int(res.dof))

    def structure_joint(self, rot, tran, options: cabi.LmOptions | None = None, min_sin2_parallax: float = 0.0,
                        cov: bool = True, score: bool = True, xyz: bool = True) -> JointStructure:
        """One 3-D point per match at (rot, tran) and the handle's depths, with its covariance and score (JointStructure).
        cov / score / xyz = False skips that output (it is then None).  Degeneracy rule, options and errors as
        covariance_joint.  The handle's state is not touched."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        n = self.size
        res = cabi.JointCov()
        X = np.zeros((n, 3)) if xyz else None
        Cv = np.zeros((n, 6)) if cov else None
        q = np.zeros(n) if score else None
        ptr = lambda a: None if a is None else _dptr(a)
        cabi.check(self._lib, self._lib.sba_problem_structure_joint(self._h, _dptr(rot), _dptr(tran),
                                                                    None if options is None else C.byref(options),
                                                                    float(min_sin2_parallax), C.byref(res), ptr(X), ptr(Cv), ptr(q)))
        return JointStructure(X, Cv, q, self._joint_cov(res))

    def structure_joint_into(self, xyz_ptr, cov_ptr, score_ptr, rot, tran, options: cabi.LmOptions | None = None,
                             min_sin2_parallax: float = 0.0) -> JointCovariance:
        """structure_joint with the outputs stored straight into DEVICE memory: xyz_ptr / cov_ptr / score_ptr are device
        addresses (for example ``tensor.data_ptr()`` of float64 tensors of n * 3, n * 6 and n elements on the handle's
        device), 16-byte aligned, 0 or None to skip an output.  Returns the pose record; nothing else crosses to the host."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        res = cabi.JointCov()
        vp = lambda a: C.c_void_p(int(a)) if a else None
        cabi.check(self._lib, self._lib.sba_problem_structure_joint_device(self._h, _dptr(rot), _dptr(tran),
                                                                           None if options is None else C.byref(options),
                                                                           float(min_sin2_parallax), C.byref(res), vp(xyz_ptr),
                                                                           vp(cov_ptr), vp(score_ptr)))
        return self._joint_cov(res)

    def structure_order_stats(self, rot, tran, ranks, options: cabi.LmOptions | None = None,
                              min_sin2_parallax: float = 0.0) -> np.ndarray:
        """The ranks[j]-th smallest (0-based) of structure_joint's scores, selected on the device: bit for bit elements of
        that array; inf (degenerate matches) sorts above every finite score, NaN above inf.  Up to 8 ranks."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        r = _ranks(ranks).reshape(-1)
        vals = np.empty(r.shape[0])
        cabi.check(self._lib, self._lib.sba_problem_structure_order_stats(
            self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options), float(min_sin2_parallax),
            r.ctypes.data_as(C.POINTER(C.c_size_t)), r.shape[0], _dptr(vals)))
        return vals

    def structure_keep_below(self, rot, tran, prob, scale, options: cabi.LmOptions | None = None,
                             min_sin2_parallax: float = 0.0):
        """Keep the matches with score <= scale * (the `prob` quantile of the scores, rank `quantile_rank`), selected,
        flagged and compacted on the device as keep_below does; the handle then equals a fresh upload of the kept matches.
        Degenerate matches (score inf) go unless the threshold itself is inf; a NaN score is dropped.  Returns (original
        indices of the kept matches (np.int64), the threshold).  `scale` has no default: how much worse than the typical
        landmark a landmark may be is the caller's choice."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        n = self.size
        rank = int(quantile_rank(prob, n).reshape(-1)[0]) if n > 0 else 0      # an empty handle: the library's refusal answers
        idx = np.empty(max(n, 1), dtype=np.int64)
        kept, thr = C.c_size_t(0), C.c_double(0.0)
        cabi.check(self._lib, self._lib.sba_problem_structure_keep_below(
            self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options), float(min_sin2_parallax), rank,
            float(scale), C.byref(thr), C.byref(kept), idx.ctypes.data_as(C.c_void_p)))
        return idx[:kept.value].copy(), thr.value

    # -- spherical resection: a further frame's pose from landmarks ------------------------------------
    def eval_resection(self, rot, tran, options: cabi.LmOptions | None = None) -> ResectionEquations:
        """The resection's normal equations at (rot, tran): landmarks d1 * left, bearings right, the d2 column never read.
        options is read for huber_delta only (None: the default, 1)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        eq = cabi.ResectionEq()
        cabi.check(self._lib, self._lib.sba_problem_eval_resection(self._h, _dptr(rot), _dptr(tran),
                                                                   None if options is None else C.byref(options), C.byref(eq)))
        ne = _to_ne(eq.eq)
        return ResectionEquations(ne.H, ne.g, ne.cost, ne.sum_w, ne.n_outlier, float(eq.n_behind))

    def solve_resection(self, rot, tran, options: cabi.LmOptions | None = None, store_depths: bool = True):
        """LM over all six pose parameters from (rot, tran), in the scale the landmarks define.  options None = the defaults
        (tran_param = TRAN_FREE: there is no gauge; TRAN_SPHERE keeps |tran| if asked).  store_depths: the eliminated depths
        at the result go into the handle's d2 column (resection_depths), after which residuals / keep_below / eval with
        DEPTH_PER_MATCH see this problem.  Returns (rot, tran, SolveSummary, n_behind); inputs are not modified."""
        rot = _f64(rot, (3,)).copy()
        tran = _f64(tran, (3,)).copy()
        s = cabi.LmSummary()
        nb = C.c_double(0.0)
        cabi.check(self._lib, self._lib.sba_problem_solve_resection(self._h, _dptr(rot), _dptr(tran),
                                                                    None if options is None else C.byref(options), C.byref(s),
                                                                    C.byref(nb), 1 if store_depths else 0))
        return rot, tran, _summary(s), float(nb.value)

    def resection_depths(self, rot, tran, return_depths: bool = True):
        """The eliminated bearing depths d* at (rot, tran) into the handle's d2 column; returns them (n,) or None."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        out = np.zeros(self.size) if return_depths else None
        cabi.check(self._lib, self._lib.sba_problem_resection_depths(self._h, _dptr(rot), _dptr(tran),
                                                                     None if out is None else _dptr(out)))
        return out

    def resection_guess(self, moments: bool = False) -> ResectionGuess:
        """The linear (DLT) pose from the landmarks and bearings: exact on noise-free data from 6 matches in general position,
        not robust to outliers.  Raises SbaError(SBA_ERR_NUMERIC) for fewer than 6 matches or a scene that does not fix the
        pose at rounding level (a planar landmark set); anything less degenerate is the caller's call from lambda2 / lambda12."""
        rot, tran = np.zeros(3), np.zeros(3)
        info = cabi.ResectionGuessInfo()
        mom = np.zeros(60) if moments else None
        cabi.check(self._lib, self._lib.sba_problem_resection_guess(self._h, _dptr(rot), _dptr(tran), C.byref(info),
                                                                    None if mom is None else _dptr(mom)))
        return ResectionGuess(rot, tran, float(info.lambda1), float(info.lambda2), float(info.lambda12),
                              np.array(info.sv, dtype=np.float64), float(info.scale), int(info.n), float(info.n_behind), mom)

    def score_resection(self, rots, trans, threshold: float) -> np.ndarray:
        """For every candidate pose (rots[k], trans[k]), k < count <= 1024, the number of matches whose resection residual has
        |r| <= threshold: (count,) int64, all candidates in one streaming pass, the same on every run."""
        rots, trans = np.ascontiguousarray(rots, dtype=np.float64), np.ascontiguousarray(trans, dtype=np.float64)
        if rots.ndim != 2 or rots.shape[1] != 3 or trans.shape != rots.shape:
            raise ValueError("rots and trans must both be (count, 3)")
        out = np.zeros(len(rots), dtype=np.int64)
        cabi.check(self._lib, self._lib.sba_problem_score_resection(self._h, _dptr(rots), _dptr(trans), len(rots), float(threshold),
                                                                    out.ctypes.data_as(C.POINTER(C.c_longlong))))
        return out

    def resection_guess_consensus(self, threshold: float, trials: int = 128, sample_size: int = 6, seed: int = 0,
                                  refit: bool = True, per_trial: bool = False) -> ResectionConsensus:
        """A starting pose that survives wrong matches: `trials` DLT trials of `sample_size` sampled matches each, every trial's
        pose scored against all matches on the device (inliers: |r| <= threshold, landmark units), the best one kept and, with
        refit, replaced by the DLT over its inliers if that has no fewer.  Raises SbaError(SBA_ERR_NUMERIC) for fewer matches
        than sample_size or when no trial finishes (every sample degenerate: a planar landmark set)."""
        opt = cabi.ResectionConsensusOptions(int(trials), int(sample_size), int(seed), float(threshold), 1 if refit else 0)
        nt = int(trials) if int(trials) > 0 else 128
        rot, tran = np.zeros(3), np.zeros(3)
        info = cabi.ResectionConsensusInfo()
        ti = np.full(max(nt, 1), -1, dtype=np.int64) if per_trial else None
        tr = np.zeros((max(nt, 1), 3)) if per_trial else None
        tt = np.zeros((max(nt, 1), 3)) if per_trial else None
        cabi.check(self._lib, self._lib.sba_problem_resection_guess_consensus(
            self._h, C.byref(opt), _dptr(rot), _dptr(tran), C.byref(info),
            None if ti is None else ti.ctypes.data_as(C.POINTER(C.c_longlong)), None if tr is None else _dptr(tr),
            None if tt is None else _dptr(tt)))
        g = info.refit
        fit = ResectionGuess(np.zeros(3), np.zeros(3), float(g.lambda1), float(g.lambda2), float(g.lambda12),
                             np.array(g.sv, dtype=np.float64), float(g.scale), int(g.n), 0.0, None) if refit else None
        return ResectionConsensus(rot, tran, int(info.n), int(info.n_inlier), int(info.best_trial), int(info.best_trial_inliers),
                                  int(info.n_valid_trials), bool(info.refit_used), fit, float(info.n_behind), ti, tr, tt)

    # -- the resection weighted by the landmarks' covariances ------------------------------------------
    def set_landmark_covariances(self, cov, scale: float = 1.0) -> None:
        """One 3 x 3 covariance per landmark, in the landmark frame: (n, 6) rows (xx, yy, zz, xy, xz, yz) as structure_joint
        returns them; `scale` multiplies every row (the pair's sigma2).  Every upload and compaction drops them again; setting
        them discards frozen weights."""
        c = _f64(cov).reshape(-1, 6)
        if c.shape[0] != self.size:
            raise ValueError("one covariance row per match")
        cabi.check(self._lib, self._lib.sba_problem_resection_set_landmark_cov(self._h, _dptr(c), float(scale)))

    def set_landmark_covariances_device(self, ptr, scale: float = 1.0) -> None:
        """set_landmark_covariances from DEVICE memory: the address of n * 6 float64 on the handle's device (for example
        ``tensor.data_ptr()``), 16-byte aligned, copied on the handle's stream."""
        cabi.check(self._lib, self._lib.sba_problem_resection_set_landmark_cov_device(self._h, C.c_void_p(int(ptr) if ptr else 0),
                                                                                      float(scale)))

    def freeze_resection_weights(self, rot, tran, bearing_sigma: float = 0.0) -> int:
        """Freeze every match's weight at the reference pose (rot, tran): the landmark covariance rotated into the new frame plus
        the bearing's noise (bearing_sigma, radians) at the eliminated depth, projected across the bearing.  Returns the number
        of matches left without weight (non-finite or indefinite covariance, non-finite depth)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        nz = C.c_longlong(0)
        cabi.check(self._lib, self._lib.sba_problem_resection_freeze_weights(self._h, _dptr(rot), _dptr(tran), float(bearing_sigma),
                                                                             C.byref(nz)))
        return int(nz.value)

    def resection_weights(self) -> np.ndarray:
        """(n, 6): the frozen information matrix of every match, rows (xx, yy, zz, xy, xz, yz); zeros where the weight is zero."""
        out = np.zeros((self.size, 6))
        cabi.check(self._lib, self._lib.sba_problem_resection_weights(self._h, _dptr(out)))
        return out

    def eval_resection_weighted(self, rot, tran, options: cabi.LmOptions | None = None) -> ResectionEquations:
        """eval_resection with the frozen weights: cost 1/2 sum rho(r^T M r), huber_delta in sigma units."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        eq = cabi.ResectionEq()
        cabi.check(self._lib, self._lib.sba_problem_eval_resection_weighted(self._h, _dptr(rot), _dptr(tran),
                                                                            None if options is None else C.byref(options), C.byref(eq)))
        ne = _to_ne(eq.eq)
        return ResectionEquations(ne.H, ne.g, ne.cost, ne.sum_w, ne.n_outlier, float(eq.n_behind))

    def solve_resection_weighted(self, rot, tran, options: cabi.LmOptions | None = None, bearing_sigma: float = 0.0,
                                 reweight_rounds: int = 1, store_depths: bool = True):
        """solve_resection with the landmark covariances: `reweight_rounds` (1 .. 8) times freeze the weights at the current pose,
        then LM from there.  Returns (rot, tran, SolveSummary of the last round, n_behind); the weights stay frozen where the
        last round froze them, so resection_covariance may follow."""
        rot = _f64(rot, (3,)).copy()
        tran = _f64(tran, (3,)).copy()
        s = cabi.LmSummary()
        nb = C.c_double(0.0)
        cabi.check(self._lib, self._lib.sba_problem_solve_resection_weighted(
            self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options), float(bearing_sigma),
            int(reweight_rounds), C.byref(s), C.byref(nb), 1 if store_depths else 0))
        return rot, tran, _summary(s), float(nb.value)

    def resection_covariance(self, rot, tran, options: cabi.LmOptions | None = None) -> ResectionCovariance:
        """The 6 x 6 covariance of the pose at (rot, tran) under the frozen weights (ResectionCovariance)."""
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        res = cabi.ResectionCov()
        cabi.check(self._lib, self._lib.sba_problem_resection_covariance(self._h, _dptr(rot), _dptr(tran),
                                                                         None if options is None else C.byref(options), C.byref(res)))
        return ResectionCovariance(np.array(res.cov, dtype=np.float64).reshape(6, 6), float(res.cost), float(res.sum_w),
                                   int(res.n_used), int(res.n_zero_weight), float(res.n_outlier), int(res.dof), float(res.sigma2))

    # -- 8-point initial guess ----------------------------------------------------------------------
    def epipolar_moments(self) -> np.ndarray:
        """(64, 45): upper triangle of A^T A of the kron(left, right) rows per interleaved group (i//2) % 64."""
        g = np.zeros((64, 45))
        cabi.check(self._lib, self._lib.sba_problem_epipolar_moments(self._h, _dptr(g)))
        return g

    def initial_guess(self, trials: int = 80, subset_fraction: float = 0.25, seed: int = 0):
        """Returns (euler (3,), tran (3,), number of candidates): R_vec_out / T_vec_out of the reference."""
        e, t, n = np.zeros(3), np.zeros(3), C.c_int(0)
        cabi.check(self._lib, self._lib.sba_problem_initial_guess(self._h, trials, subset_fraction, seed, _dptr(e),
                                                                  _dptr(t), C.byref(n)))
        return e, t, n.value

    def epipolar_subset_moments(self, indices) -> np.ndarray:
        """indices: (trials, m) int32 match indices -> (trials, 45): A^T A of the kron(left, right) rows of each list."""
        idx = np.ascontiguousarray(indices, dtype=np.int32)
        if idx.ndim != 2:
            raise ValueError("indices must be (trials, m)")
        out = np.zeros((idx.shape[0], 45))
        cabi.check(self._lib, self._lib.sba_problem_epipolar_subset_moments(self._h, idx.ctypes.data_as(C.c_void_p), idx.shape[0],
                                                                            idx.shape[1], _dptr(out)))
        return out

    def initial_guess_reference(self, trials: int = 80, subset_fraction: float = 0.25):
        """The initial guess from the subsets the reference itself would draw (std::random_shuffle on this process's
        rand() stream, reference .hpp:182-211 / .cpp:130-141).  Returns (euler, tran, number of candidates)."""
        e, t, n = np.zeros(3), np.zeros(3), C.c_int(0)
        cabi.check(self._lib, self._lib.sba_problem_initial_guess_reference(self._h, trials, subset_fraction, _dptr(e), _dptr(t),
                                                                            C.byref(n)))
        return e, t, n.value

    # -- multi-GPU ------------------------------------------------------------------------------------
    def comm_init_rank(self, nranks: int, rank: int, unique_id: bytes) -> None:
        if len(unique_id) != cabi.COMM_ID_BYTES:
            raise ValueError("unique_id must be 128 bytes")
        cabi.check(self._lib, self._lib.sba_problem_comm_init_rank(self._h, nranks, rank, unique_id))

    def comm_destroy(self) -> None:
        cabi.check(self._lib, self._lib.sba_problem_comm_destroy(self._h))

    def peer_export(self, nranks: int, rank: int) -> bytes:
        """Allocate this rank's inbox for the direct peer exchange; returns its 64-byte IPC handle."""
        buf = C.create_string_buffer(cabi.PEER_HANDLE_BYTES)
        cabi.check(self._lib, self._lib.sba_problem_peer_export(self._h, nranks, rank, buf))
        return buf.raw

    def peer_connect(self, handles: bytes) -> None:
        """handles: the nranks 64-byte IPC handles in rank order, concatenated."""
        cabi.check(self._lib, self._lib.sba_problem_peer_connect(self._h, handles))

    def peer_selftest(self, rounds: int = 8) -> bool:
        ok = C.c_int(0)
        cabi.check(self._lib, self._lib.sba_problem_peer_selftest(self._h, rounds, C.byref(ok)))
        return bool(ok.value)

    def peer_disable(self) -> None:
        cabi.check(self._lib, self._lib.sba_problem_peer_disable(self._h))

    def set_shard(self, rank: int, nranks: int) -> None:
        """Which shard of the correspondences this problem holds (needed by the d-only stage over the user hook)."""
        cabi.check(self._lib, self._lib.sba_problem_set_shard(self._h, rank, nranks))

    def set_allreduce(self, fn) -> None:
        """fn(device_ptr: int, count: int, stream: int) -> int (0 = ok), or None to clear."""
        if fn is None:
            cb = C.cast(None, cabi.ALLREDUCE_FN)
        else:
            def _tramp(buf, count, stream, _user):
                try:
                    return int(fn(buf or 0, count, stream or 0) or 0)
                except Exception:  # never let an exception cross the C boundary
                    import traceback
                    traceback.print_exc()
                    return -1
            cb = cabi.ALLREDUCE_FN(_tramp)
        self._hook_keepalive = cb
        cabi.check(self._lib, self._lib.sba_problem_set_allreduce(self._h, cb, None))

    @property
    def pack_device_ptr(self) -> int:
        p = C.c_void_p()
        cabi.check(self._lib, self._lib.sba_problem_pack_device_ptr(self._h, C.byref(p)))
        return p.value or 0


class Landmarks:
    """A landmark map resident on one GPU (``sba_landmarks``): n landmarks with their 3 x 3 covariances and a count of accepted
    observations each, kept across frames.  `fuse` folds one registered frame's bearings into them: per landmark the exact
    linear-Gaussian update of position and covariance from one bearing at a known pose with a known pose covariance."""

    def __init__(self, device: int = 0, stream: int | None = None, lib=None):
        self._lib = lib if lib is not None else cabi.load_library()
        self._h = C.c_void_p()
        cabi.check(self._lib, self._lib.sba_landmarks_create(C.byref(self._h), device, C.c_void_p(stream or 0)))
        self.device = device

    # -- life cycle ---------------------------------------------------------------------------
    def close(self) -> None:
        """Destroy the handle; `destroy_status` keeps the library's answer as Problem.close does (non-zero: POISONED, device
        resources leaked, the process should exit non-zero)."""
        if getattr(self, "_h", None) is not None and self._h:
            self.destroy_status = int(self._lib.sba_landmarks_destroy(self._h))
            self._h = C.c_void_p()
            if self.destroy_status != 0:
                import warnings
                warnings.warn("sba_landmarks_destroy: " + cabi.last_error(self._lib), ResourceWarning, stacklevel=2)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- data ------------------------------------------------------------------------------------
    def set(self, xyz, cov, cov_scale: float = 1.0) -> None:
        """Replace the map: xyz (n, 3) and cov (n, 6) rows (xx, yy, zz, xy, xz, yz) as structure_joint returns them; cov_scale
        multiplies every covariance row (the pair's sigma2).  Every observation count becomes 0."""
        x, c = _f64(xyz).reshape(-1, 3), _f64(cov).reshape(-1, 6)
        if x.shape[0] != c.shape[0]:
            raise ValueError("one covariance row per landmark")
        cabi.check(self._lib, self._lib.sba_landmarks_set(self._h, _dptr(x), _dptr(c), x.shape[0], float(cov_scale)))

    def set_device(self, xyz_ptr, cov_ptr, n: int, cov_scale: float = 1.0) -> None:
        """set from DEVICE rows on the handle's device (for example what Problem.structure_joint_into wrote), 16-byte aligned."""
        cabi.check(self._lib, self._lib.sba_landmarks_set_device(self._h, C.c_void_p(int(xyz_ptr) if xyz_ptr else 0),
                                                                 C.c_void_p(int(cov_ptr) if cov_ptr else 0), int(n), float(cov_scale)))

    @property
    def size(self) -> int:
        n = C.c_size_t(0)
        cabi.check(self._lib, self._lib.sba_landmarks_size(self._h, C.byref(n)))
        return n.value

    def get(self):
        """(xyz (n, 3), cov (n, 6)): the map as host rows."""
        n = self.size
        x, c = np.zeros((n, 3)), np.zeros((n, 6))
        cabi.check(self._lib, self._lib.sba_landmarks_get(self._h, _dptr(x), _dptr(c)))
        return x, c

    def get_device(self, xyz_ptr, cov_ptr) -> None:
        """The map as rows in the caller's DEVICE memory (n * 3 and n * 6 float64, 16-byte aligned, 0 or None to skip one): the
        layout Problem.upload_device reads as `left` and Problem.set_landmark_covariances_device reads.  Complete on return."""
        cabi.check(self._lib, self._lib.sba_landmarks_get_device(self._h, C.c_void_p(int(xyz_ptr) if xyz_ptr else 0),
                                                                 C.c_void_p(int(cov_ptr) if cov_ptr else 0)))

    def counts(self) -> np.ndarray:
        """(n,) uint32: accepted observations per landmark since the last set."""
        out = np.zeros(self.size, dtype=np.uint32)
        cabi.check(self._lib, self._lib.sba_landmarks_counts(self._h, out.ctypes.data_as(C.POINTER(C.c_uint32))))
        return out

    def fuse(self, bearings, rot, tran, bearing_sigma: float = 0.0, chi2_gate: float = float("inf"), pose_cov=None, idx=None,
             apply: bool = True, want_chi2: bool = True) -> LandmarkFusion:
        """Fuse one frame's bearings (m, 3), of any length > 0, seen from the pose (rot, tran) with covariance pose_cov (6, 6) over
        [rot | tran] or None.  idx None: the dense form, one bearing per landmark, a zero bearing = not seen; otherwise observation
        j is landmark idx[j], strictly increasing.  apply False: a dry run, chi2 and counts only."""
        y = _f64(bearings).reshape(-1, 3)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        m = y.shape[0]
        opt = cabi.LandmarkFuseOptions()
        opt.bearing_sigma, opt.chi2_gate, opt.apply = float(bearing_sigma), float(chi2_gate), 1 if apply else 0
        pc = None
        if pose_cov is not None:
            pc = _f64(pose_cov, (6, 6))
            opt.pose_cov = _dptr(pc)
        ip = None
        if idx is not None:
            ii = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
            if ii.shape[0] != m:
                raise ValueError("one index per bearing")
            ip = ii.ctypes.data_as(C.POINTER(C.c_int64))
        chi2 = np.full(m, np.nan) if want_chi2 else None
        res = cabi.LandmarkFuseResult()
        cabi.check(self._lib, self._lib.sba_landmarks_fuse(self._h, ip, _dptr(y), m, _dptr(rot), _dptr(tran), C.byref(opt), C.byref(res),
                                                           None if chi2 is None else _dptr(chi2)))
        return LandmarkFusion(int(res.n_obs), int(res.n_skipped), int(res.n_behind), int(res.n_gated), int(res.n_fused), chi2)

    def _register_args(self, bearings, idx, bearing_sigma, chi2_gate, apply, options):
        y = _f64(bearings).reshape(-1, 3)
        m = y.shape[0]
        ii = None
        if idx is not None:
            ii = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
            if ii.shape[0] != m:
                raise ValueError("one index per bearing")
        opt = cabi.LandmarkRegisterOptions()
        opt.bearing_sigma, opt.chi2_gate, opt.apply = float(bearing_sigma), float(chi2_gate), 1 if apply else 0
        opt.lm = options if options is not None else default_lm_options(huber_delta=0.0)
        return y, m, ii, opt

    def eval_register(self, bearings, rot, tran, rot_ref=None, tran_ref=None, bearing_sigma: float = 0.0,
                      idx=None) -> LandmarkRegisterEquations:
        """One evaluation of the joint registration at (rot, tran) with the bearing noise frozen at (rot_ref, tran_ref), by
        default the same pose.  bearings and idx as for `fuse`.  The map is not written."""
        y, m, ii, opt = self._register_args(bearings, idx, bearing_sigma, float("inf"), False, None)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        rot_ref = rot if rot_ref is None else _f64(rot_ref, (3,))
        tran_ref = tran if tran_ref is None else _f64(tran_ref, (3,))
        ev = cabi.LandmarkRegisterEval()
        cabi.check(self._lib, self._lib.sba_landmarks_eval_register(
            self._h, None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(y), m, _dptr(rot), _dptr(tran), _dptr(rot_ref),
            _dptr(tran_ref), C.byref(opt), C.byref(ev)))
        return LandmarkRegisterEquations(np.array(ev.H, dtype=np.float64).reshape(6, 6), np.array(ev.g, dtype=np.float64), float(ev.cost),
                                         int(ev.n_used), int(ev.n_behind))

    def register(self, bearings, rot, tran, bearing_sigma: float = 0.0, chi2_gate: float = float("inf"), idx=None, apply: bool = True,
                 options: cabi.LmOptions | None = None, return_chi2: bool = False) -> LandmarkRegistration:
        """Solve the frame's pose and every observed landmark jointly from the start (rot, tran), and with `apply` write the
        landmarks' posteriors back.  bearings and idx as for `fuse`.  options: LM options with huber_delta = 0 (the default here);
        max_num_iterations = 0 registers at the given pose.  apply False: a dry run."""
        y, m, ii, opt = self._register_args(bearings, idx, bearing_sigma, chi2_gate, apply, options)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        chi2 = np.full(m, np.nan) if return_chi2 else None
        res = cabi.LandmarkRegisterResult()
        cabi.check(self._lib, self._lib.sba_landmarks_register(
            self._h, None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64)), _dptr(y), m, _dptr(rot), _dptr(tran), C.byref(opt),
            C.byref(res), None if chi2 is None else _dptr(chi2)))
        return LandmarkRegistration(np.array(res.rot, dtype=np.float64), np.array(res.tran, dtype=np.float64),
                                    np.array(res.cov, dtype=np.float64).reshape(6, 6), _summary(res.summary), int(res.n_obs),
                                    int(res.n_skipped), int(res.n_behind), int(res.n_gated), int(res.n_fused), int(res.n_used), chi2)

    def _robust_args(self, bearings, bearings_device, m, idx, huber_delta, bearing_sigma, chi2_gate, apply, options):
        """(bearings pointer, m, idx array, options, the host bearings to keep alive) of the two robust methods."""
        if (bearings is None) == (bearings_device is None):
            raise ValueError("give either bearings or bearings_device")
        ii = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        if bearings_device is None:
            y = _f64(bearings).reshape(-1, 3)
            m, ptr = y.shape[0], _dptr(y)
        else:
            if m is None:
                if ii is None:
                    m = self.size
                else:
                    m = ii.shape[0]
            y, ptr = None, C.c_void_p(int(bearings_device))
        if ii is not None and ii.shape[0] != m:
            raise ValueError("one index per bearing")
        opt = cabi.LandmarkRegisterOptions()
        gate = float(huber_delta) ** 2 if chi2_gate is None else float(chi2_gate)
        opt.bearing_sigma, opt.chi2_gate, opt.apply = float(bearing_sigma), gate, 1 if apply else 0
        opt.lm = options if options is not None else default_lm_options()
        opt.lm.huber_delta = float(huber_delta)
        return ptr, int(m), ii, opt, y

    def eval_register_robust(self, bearings, rot, tran, huber_delta: float, rot_ref=None, tran_ref=None, bearing_sigma: float = 0.0,
                             idx=None, bearings_device=None, m: int | None = None) -> LandmarkRobustRegisterEquations:
        """eval_register under the Huber loss on every landmark's chi2 (huber_delta > 0, in units of the whitened residual).
        bearings_device: instead of `bearings` (then None), the address of m * 3 float64 on the handle's device, for example
        ``tensor.data_ptr()``; m defaults to len(idx), or to the map's size in the dense form."""
        ptr, m, ii, opt, keep = self._robust_args(bearings, bearings_device, m, idx, huber_delta, bearing_sigma, None, False, None)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        rot_ref = rot if rot_ref is None else _f64(rot_ref, (3,))
        tran_ref = tran if tran_ref is None else _f64(tran_ref, (3,))
        ev = cabi.LandmarkRegisterRobustEval()
        fn = self._lib.sba_landmarks_eval_register_robust if bearings_device is None else self._lib.sba_landmarks_eval_register_robust_device
        cabi.check(self._lib, fn(self._h, None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64)), ptr, m, _dptr(rot), _dptr(tran),
                                 _dptr(rot_ref), _dptr(tran_ref), C.byref(opt), C.byref(ev)))
        return LandmarkRobustRegisterEquations(np.array(ev.H, dtype=np.float64).reshape(6, 6), np.array(ev.g, dtype=np.float64), float(ev.cost),
                                               int(ev.n_used), int(ev.n_behind), int(ev.n_outlier))

    def register_robust(self, bearings, rot, tran, huber_delta: float, bearing_sigma: float = 0.0, chi2_gate: float | None = None, idx=None,
                        apply: bool = True, options: cabi.LmOptions | None = None, return_chi2: bool = False, bearings_device=None,
                        m: int | None = None, chi2_device=None) -> LandmarkRobustRegistration:
        """`register` under the Huber loss on every landmark's chi2: wrong matches are downweighted in the solve and gated in
        the write-back.  chi2_gate defaults to huber_delta^2, the largest value accepted: a downweighted observation must not
        be fused (its conditional covariance would be inflated by 1 / w).  options: LM options whose huber_delta is replaced by
        `huber_delta`.  bearings_device as for eval_register_robust; with it chi2 goes to chi2_device (the address of m float64
        on the device, or None) instead of return_chi2's host array."""
        ptr, m, ii, opt, keep = self._robust_args(bearings, bearings_device, m, idx, huber_delta, bearing_sigma, chi2_gate, apply, options)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        res = cabi.LandmarkRegisterRobustResult()
        ip = None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64))
        if bearings_device is None:
            if chi2_device is not None:
                raise ValueError("chi2_device goes with bearings_device")
            chi2 = np.full(m, np.nan) if return_chi2 else None
            cabi.check(self._lib, self._lib.sba_landmarks_register_robust(
                self._h, ip, ptr, m, _dptr(rot), _dptr(tran), C.byref(opt), C.byref(res), None if chi2 is None else _dptr(chi2)))
        else:
            if return_chi2:
                raise ValueError("with bearings_device chi2 is written to chi2_device")
            chi2 = chi2_device
            cabi.check(self._lib, self._lib.sba_landmarks_register_robust_device(
                self._h, ip, ptr, m, _dptr(rot), _dptr(tran), C.byref(opt), C.byref(res), C.c_void_p(int(chi2_device) if chi2_device else 0)))
        return LandmarkRobustRegistration(np.array(res.rot, dtype=np.float64), np.array(res.tran, dtype=np.float64),
                                          np.array(res.cov, dtype=np.float64).reshape(6, 6), _summary(res.summary), int(res.n_obs),
                                          int(res.n_skipped), int(res.n_behind), int(res.n_gated), int(res.n_fused), int(res.n_used), chi2,
                                          int(res.n_outlier))

    def _hampel_options(self, opt, huber_delta, b, c, huber_first):
        """The Hampel options record around the robust one: b and c default to 2 a and 4 a."""
        ho = cabi.LandmarkRegisterHampelOptions()
        ho.base = opt
        ho.b = 2.0 * float(huber_delta) if b is None else float(b)
        ho.c = 4.0 * float(huber_delta) if c is None else float(c)
        ho.huber_first = 1 if huber_first else 0
        return ho

    def eval_register_hampel(self, bearings, rot, tran, huber_delta: float, b: float | None = None, c: float | None = None, rot_ref=None,
                             tran_ref=None, bearing_sigma: float = 0.0, idx=None, bearings_device=None,
                             m: int | None = None) -> LandmarkHampelRegisterEquations:
        """eval_register under Hampel's three-part loss on every landmark's chi2: a = huber_delta < b < c in units of the whitened
        residual, by default b = 2 a and c = 4 a; b = c = inf is the Huber loss.  Everything else as for eval_register_robust."""
        ptr, m, ii, opt, keep = self._robust_args(bearings, bearings_device, m, idx, huber_delta, bearing_sigma, None, False, None)
        ho = self._hampel_options(opt, huber_delta, b, c, True)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        rot_ref = rot if rot_ref is None else _f64(rot_ref, (3,))
        tran_ref = tran if tran_ref is None else _f64(tran_ref, (3,))
        ev = cabi.LandmarkRegisterHampelEval()
        fn = self._lib.sba_landmarks_eval_register_hampel if bearings_device is None else self._lib.sba_landmarks_eval_register_hampel_device
        cabi.check(self._lib, fn(self._h, None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64)), ptr, m, _dptr(rot), _dptr(tran),
                                 _dptr(rot_ref), _dptr(tran_ref), C.byref(ho), C.byref(ev)))
        return LandmarkHampelRegisterEquations(np.array(ev.H, dtype=np.float64).reshape(6, 6), np.array(ev.g, dtype=np.float64), float(ev.cost),
                                               int(ev.n_used), int(ev.n_behind), int(ev.n_outlier), int(ev.n_rejected))

    def register_hampel(self, bearings, rot, tran, huber_delta: float, b: float | None = None, c: float | None = None,
                        huber_first: bool = True, bearing_sigma: float = 0.0, chi2_gate: float | None = None, idx=None, apply: bool = True,
                        options: cabi.LmOptions | None = None, return_chi2: bool = False, bearings_device=None, m: int | None = None,
                        chi2_device=None) -> LandmarkHampelRegistration:
        """`register_robust` under Hampel's redescending loss: a wrong match beyond c has weight exactly 0, in the solve and in
        cov = H_rho^-1, which Huber's bounded but non-zero influence leaves optimistic.  a = huber_delta, b and c default to 2 a
        and 4 a.  The objective is not convex: with huber_first the Huber solve runs first, from (rot, tran), and the Hampel solve
        starts at its minimiser (rot_huber, tran_huber, huber_iterations report that stage).  chi2_gate defaults to a^2, the
        largest value accepted.  Raises SbaError(SBA_ERR_NUMERIC), the map untouched, when fewer than 3 observations keep a
        weight at the solution.  Everything else as for register_robust."""
        ptr, m, ii, opt, keep = self._robust_args(bearings, bearings_device, m, idx, huber_delta, bearing_sigma, chi2_gate, apply, options)
        ho = self._hampel_options(opt, huber_delta, b, c, huber_first)
        rot, tran = _f64(rot, (3,)), _f64(tran, (3,))
        res = cabi.LandmarkRegisterHampelResult()
        ip = None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64))
        if bearings_device is None:
            if chi2_device is not None:
                raise ValueError("chi2_device goes with bearings_device")
            chi2 = np.full(m, np.nan) if return_chi2 else None
            cabi.check(self._lib, self._lib.sba_landmarks_register_hampel(
                self._h, ip, ptr, m, _dptr(rot), _dptr(tran), C.byref(ho), C.byref(res), None if chi2 is None else _dptr(chi2)))
        else:
            if return_chi2:
                raise ValueError("with bearings_device chi2 is written to chi2_device")
            chi2 = chi2_device
            cabi.check(self._lib, self._lib.sba_landmarks_register_hampel_device(
                self._h, ip, ptr, m, _dptr(rot), _dptr(tran), C.byref(ho), C.byref(res), C.c_void_p(int(chi2_device) if chi2_device else 0)))
        return LandmarkHampelRegistration(np.array(res.rot, dtype=np.float64), np.array(res.tran, dtype=np.float64),
                                          np.array(res.cov, dtype=np.float64).reshape(6, 6), _summary(res.summary), int(res.n_obs),
                                          int(res.n_skipped), int(res.n_behind), int(res.n_gated), int(res.n_fused), int(res.n_used), chi2,
                                          int(res.n_outlier), int(res.n_rejected), np.array(res.rot_huber, dtype=np.float64),
                                          np.array(res.tran_huber, dtype=np.float64), int(res.huber_iterations))

    # -- edits: the counts survive all of them -------------------------------------------------------
    def scores(self) -> np.ndarray:
        """(n,) trace Sigma / X . X per landmark, ((xx + yy) + zz) / ((x x + y y) + z z) in float64 in exactly that order."""
        out = np.zeros(self.size)
        cabi.check(self._lib, self._lib.sba_landmarks_scores(self._h, _dptr(out)))
        return out

    def prune(self, max_score: float = float("inf"), min_count: int = 0, mask=None, apply: bool = True,
              want_kept: bool = True) -> LandmarkPrune:
        """Drop the landmarks that are invalid, whose score exceeds max_score, that have fewer than min_count accepted observations
        or whose mask entry (n,) is 0; the kept ones close up in their old order with their counts.  apply False: a dry run."""
        n = self.size
        opt = cabi.LandmarkPruneOptions()
        opt.max_score, opt.min_count, opt.apply = float(max_score), int(min_count), 1 if apply else 0
        mk = None
        if mask is not None:
            mk = np.ascontiguousarray(np.asarray(mask).reshape(-1) != 0, dtype=np.uint8)
            if mk.shape[0] != n:
                raise ValueError("one mask entry per landmark")
            opt.mask = mk.ctypes.data_as(C.POINTER(C.c_uint8))
        kept = np.zeros(n, dtype=np.int64) if want_kept else None
        res = cabi.LandmarkPruneResult()
        cabi.check(self._lib, self._lib.sba_landmarks_prune(self._h, C.byref(opt), C.byref(res),
                                                            None if kept is None else kept.ctypes.data_as(C.POINTER(C.c_int64))))
        return LandmarkPrune(int(res.n_before), int(res.n_invalid), int(res.n_uncertain), int(res.n_unobserved), int(res.n_masked),
                             int(res.n_kept), None if kept is None else kept[:int(res.n_kept)].copy())

    def append(self, xyz, cov, cov_scale: float = 1.0) -> None:
        """Add rows as `set` takes them behind the map's own: the old landmarks and counts stay, the new ones start at count 0."""
        x, c = _f64(xyz).reshape(-1, 3), _f64(cov).reshape(-1, 6)
        if x.shape[0] != c.shape[0]:
            raise ValueError("one covariance row per landmark")
        cabi.check(self._lib, self._lib.sba_landmarks_append(self._h, _dptr(x), _dptr(c), x.shape[0], float(cov_scale)))

    def append_device(self, xyz_ptr, cov_ptr, n_add: int, cov_scale: float = 1.0) -> None:
        """append from DEVICE rows on the handle's device (for example what Problem.structure_joint_into wrote), 16-byte aligned."""
        cabi.check(self._lib, self._lib.sba_landmarks_append_device(self._h, C.c_void_p(int(xyz_ptr) if xyz_ptr else 0),
                                                                    C.c_void_p(int(cov_ptr) if cov_ptr else 0), int(n_add), float(cov_scale)))

    def gather(self, idx):
        """(xyz (m, 3), cov (m, 6), counts (m,)): rows idx of the map; any order, repeats allowed."""
        ii = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        m = ii.shape[0]
        x, c, k = np.zeros((m, 3)), np.zeros((m, 6)), np.zeros(m, dtype=np.uint32)
        cabi.check(self._lib, self._lib.sba_landmarks_gather(self._h, ii.ctypes.data_as(C.POINTER(C.c_int64)), m, _dptr(x), _dptr(c),
                                                             k.ctypes.data_as(C.POINTER(C.c_uint32))))
        return x, c, k

    def gather_device(self, idx, xyz_ptr, cov_ptr) -> None:
        """Rows idx (host indices) of the map as rows in the caller's DEVICE memory (m * 3 and m * 6 float64, 16-byte aligned, 0 or
        None to skip one): what Problem.upload_device reads as `left` and Problem.set_landmark_covariances_device reads."""
        ii = np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        cabi.check(self._lib, self._lib.sba_landmarks_gather_device(self._h, ii.ctypes.data_as(C.POINTER(C.c_int64)), ii.shape[0],
                                                                    C.c_void_p(int(xyz_ptr) if xyz_ptr else 0),
                                                                    C.c_void_p(int(cov_ptr) if cov_ptr else 0)))

    # -- descriptors: a row per landmark, kept in step with the map by set, prune and append ------------
    def set_descriptors(self, desc) -> None:
        """One float32 descriptor row (n, dim) per landmark, 1 <= dim <= 256; padded rows (a view of a wider array) pass as they
        are.  A second call replaces the rows; None or dim 0 drops them."""
        if desc is None or np.asarray(desc).ndim == 2 and np.asarray(desc).shape[1] == 0:
            cabi.check(self._lib, self._lib.sba_landmarks_set_descriptors(self._h, None, 0, 0, 0))
            return
        (d,), dim, stride = _descriptors(desc)
        cabi.check(self._lib, self._lib.sba_landmarks_set_descriptors(self._h, C.c_void_p(d.ctypes.data), d.shape[0], dim, stride))

    def set_descriptors_device(self, desc_ptr, n_rows: int, dim: int, row_stride_bytes: int | None = None) -> None:
        """set_descriptors from DEVICE rows on the handle's device, 4-byte aligned; complete on return."""
        cabi.check(self._lib, self._lib.sba_landmarks_set_descriptors_device(
            self._h, C.c_void_p(int(desc_ptr) if desc_ptr else 0), int(n_rows), int(dim), int(4 * dim if row_stride_bytes is None else row_stride_bytes)))

    @property
    def descriptor_dim(self) -> int:
        """The dimension of the map's descriptor rows; 0: the map keeps none."""
        dim = C.c_int(0)
        cabi.check(self._lib, self._lib.sba_landmarks_descriptor_dim(self._h, C.byref(dim)))
        return dim.value

    def get_descriptors(self, idx=None) -> np.ndarray:
        """(n, dim) float32, or rows idx (any order, repeats allowed) as (m, dim)."""
        dim = self.descriptor_dim
        ii = None if idx is None else np.ascontiguousarray(idx, dtype=np.int64).reshape(-1)
        rows = self.size if ii is None else ii.shape[0]
        out = np.zeros((rows, dim), dtype=np.float32)
        cabi.check(self._lib, self._lib.sba_landmarks_get_descriptors(
            self._h, None if ii is None else ii.ctypes.data_as(C.POINTER(C.c_int64)), rows, C.c_void_p(out.ctypes.data), 4 * max(dim, 1)))
        return out

    def append_described(self, xyz, cov, desc, cov_scale: float = 1.0) -> None:
        """append plus the new rows' descriptors (n_add, dim): the map keeps descriptors of this dim, or is empty."""
        x, c = _f64(xyz).reshape(-1, 3), _f64(cov).reshape(-1, 6)
        (d,), dim, stride = _descriptors(desc)
        if x.shape[0] != c.shape[0] or x.shape[0] != d.shape[0]:
            raise ValueError("one covariance row and one descriptor row per landmark")
        cabi.check(self._lib, self._lib.sba_landmarks_append_described(self._h, _dptr(x), _dptr(c), C.c_void_p(d.ctypes.data), x.shape[0], dim,
                                                                       stride, float(cov_scale)))

    def append_described_device(self, xyz_ptr, cov_ptr, desc_ptr, n_add: int, dim: int, cov_scale: float = 1.0,
                                row_stride_bytes: int | None = None) -> None:
        """append_described from DEVICE arrays on the handle's device: xyz and cov 16-byte aligned, the descriptors 4-byte."""
        cabi.check(self._lib, self._lib.sba_landmarks_append_described_device(
            self._h, C.c_void_p(int(xyz_ptr) if xyz_ptr else 0), C.c_void_p(int(cov_ptr) if cov_ptr else 0),
            C.c_void_p(int(desc_ptr) if desc_ptr else 0), int(n_add), int(dim), int(4 * dim if row_stride_bytes is None else row_stride_bytes),
            float(cov_scale)))

    def _associate_out(self, m, ratio, max_distance):
        cap = min(self.size, int(m))
        opt = cabi.LandmarkAssociateOptions(float(ratio), float(max_distance))
        return opt, cabi.LandmarkAssociateResult(), np.zeros(cap, dtype=np.int64), np.zeros(cap, dtype=np.int32), np.zeros(cap, dtype=np.float32)

    @staticmethod
    def _association(res, idx, rows, dist, bearings) -> LandmarkAssociation:
        k = int(res.n_associated)
        return LandmarkAssociation(int(res.n_frame), int(res.n_accepted), int(res.n_contested), k, idx[:k].copy(), rows[:k].copy(),
                                   dist[:k].copy(), None if bearings is None else bearings[:k].copy())

    def associate(self, frame_desc, frame_bearings=None, ratio: float = 0.3, max_distance: float = float("inf")) -> LandmarkAssociation:
        """A frame's descriptors (m, dim) against the map's: per claimed landmark its index, the winning frame row, its distance
        and, with frame_bearings (m, 3), that row's bearing -- what register* takes as idx and bearings (LandmarkAssociation)."""
        (d,), dim, stride = _descriptors(frame_desc)
        m = d.shape[0]
        b = None if frame_bearings is None else _f64(frame_bearings).reshape(-1, 3)
        if b is not None and b.shape[0] != m:
            raise ValueError("one bearing per frame row")
        opt, res, idx, rows, dist = self._associate_out(m, ratio, max_distance)
        out = None if b is None else np.zeros((idx.shape[0], 3))
        cabi.check(self._lib, self._lib.sba_landmarks_associate(
            self._h, C.c_void_p(d.ctypes.data), m, dim, stride, None if b is None else _dptr(b), C.byref(opt), C.byref(res),
            idx.ctypes.data_as(C.POINTER(C.c_int64)), rows.ctypes.data_as(C.POINTER(C.c_int32)), dist.ctypes.data_as(C.POINTER(C.c_float)),
            None if out is None else _dptr(out)))
        return self._association(res, idx, rows, dist, out)

    def associate_device(self, frame_desc_ptr, m: int, dim: int, frame_bearings_ptr=None, bearings_out_ptr=None, ratio: float = 0.3,
                         max_distance: float = float("inf"), row_stride_bytes: int | None = None) -> LandmarkAssociation:
        """associate from DEVICE rows on the handle's device (descriptors 4-byte, bearings 8-byte aligned); the gathered bearings
        go to bearings_out_ptr (device, 16-byte aligned, min(n, m) rows of 3 float64), where register_robust / register_hampel read
        them in place.  idx, rows and distance come back on the host; `bearings` is None."""
        opt, res, idx, rows, dist = self._associate_out(m, ratio, max_distance)
        cabi.check(self._lib, self._lib.sba_landmarks_associate_device(
            self._h, C.c_void_p(int(frame_desc_ptr) if frame_desc_ptr else 0), int(m), int(dim),
            int(4 * dim if row_stride_bytes is None else row_stride_bytes), C.c_void_p(int(frame_bearings_ptr) if frame_bearings_ptr else 0),
            C.byref(opt), C.byref(res), idx.ctypes.data_as(C.POINTER(C.c_int64)), rows.ctypes.data_as(C.POINTER(C.c_int32)),
            dist.ctypes.data_as(C.POINTER(C.c_float)), C.c_void_p(int(bearings_out_ptr) if bearings_out_ptr else 0)))
        return self._association(res, idx, rows, dist, None)


class Batch:
    """Many independent two-view problems ("pairs") on one GPU (``sba_batch``; BASELINE config C5)."""

    def __init__(self, device: int = 0, stream: int | None = None, lib=None):
        self._lib = lib if lib is not None else cabi.load_library()
        self._h = C.c_void_p()
        cabi.check(self._lib, self._lib.sba_batch_create(C.byref(self._h), device, C.c_void_p(stream or 0)))
        self.num_pairs = 0
        self._total = 0
        self._offsets = np.zeros(1, dtype=np.uint64)

    def close(self) -> None:
        """As Problem.close(): `destroy_status` != 0 = the batch was poisoned and its device resources were leaked."""
        if getattr(self, "_h", None) is not None and self._h:
            self.destroy_status = int(self._lib.sba_batch_destroy(self._h))
            self._h = C.c_void_p()
            if self.destroy_status != 0:
                import warnings
                warnings.warn("sba_batch_destroy: " + cabi.last_error(self._lib), ResourceWarning, stacklevel=2)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_kernel(self, kind: int) -> None:
        cabi.check(self._lib, self._lib.sba_batch_set_kernel(self._h, kind))

    def upload(self, left_xyz, right_xyz, offsets, d12=None, store: int = STORE_F64) -> None:
        """left/right: (total, 3); offsets: (num_pairs+1,) row offsets of each pair; d12: (total, 2) or None."""
        x1 = _f64(left_xyz).reshape(-1, 3)
        x2 = _f64(right_xyz).reshape(-1, 3)
        off = np.ascontiguousarray(offsets, dtype=np.uint64)
        if off.ndim != 1 or off.size < 1 or int(off[-1]) > x1.shape[0] or x1.shape != x2.shape:
            raise ValueError("bad offsets / array shapes")
        dp = None
        if d12 is not None:
            d = _f64(d12).reshape(-1, 2)
            if d.shape[0] != x1.shape[0]:
                raise ValueError("d12 length differs")
            dp = d.ctypes.data_as(C.c_void_p)
        self.num_pairs = off.size - 1
        self._total = int(off[-1])
        cabi.check(self._lib, self._lib.sba_batch_upload(
            self._h, x1.ctypes.data_as(C.c_void_p), x2.ctypes.data_as(C.c_void_p), dp,
            off.ctypes.data_as(C.POINTER(C.c_size_t)), self.num_pairs, store))
        self._offsets = off.copy()

    def upload_matches(self, left_kp: np.ndarray, left_offsets, right_kp: np.ndarray, right_offsets, left_desc, right_desc,
                       im_width: int, im_height: int, ratio: float = 0.3, init_depth=None, store: int = STORE_F64):
        """Match every pair's descriptors on the device (batch_match_descriptors), then upload the matched key-points of all
        pairs as upload() of their sphere points would, with offsets = the exclusive scan of the per-pair counts and
        d12 = (init_depth[g], init_depth[g]) per match of pair g if init_depth (num_pairs,) or a scalar is given.  Offsets
        index key-point records and descriptor rows alike.  Returns (match_left, match_right, n_matched): pair-local int32
        indices concatenated in pair order, and the per-pair counts."""
        kl, kr = np.ascontiguousarray(left_kp), np.ascontiguousarray(right_kp)
        if kl.ndim != 2 or kr.ndim != 2 or kl.dtype != kr.dtype or kl.shape[1] != kr.shape[1]:
            raise ValueError("left/right key-point records differ in layout")
        lo, ro = _offsets(left_offsets, "left"), _offsets(right_offsets, "right")
        if lo.size != ro.size:
            raise ValueError("left/right offsets differ in length")
        B = lo.size - 1
        (dl, dr), dim, dstride = _descriptors(left_desc, right_desc)
        if dl.shape[0] != kl.shape[0] or dr.shape[0] != kr.shape[0]:
            raise ValueError("one descriptor row per key-point")
        if int(lo[-1]) > kl.shape[0] or int(ro[-1]) > kr.shape[0]:
            raise ValueError("offsets run past the arrays")
        stride = kl.strides[0] if kl.shape[0] > 0 else (kr.strides[0] if kr.shape[0] > 0 else 28)
        dp = None
        if init_depth is not None:
            dd = np.ascontiguousarray(np.broadcast_to(np.asarray(init_depth, dtype=np.float64), (B,)))
            dp = _dptr(dd)
        nl = max(int(lo[-1] - lo[0]) if B else 0, 1)
        ml, mr = np.zeros(nl, dtype=np.int32), np.zeros(nl, dtype=np.int32)
        cnt = np.zeros(max(B, 1), dtype=np.uint64)
        cabi.check(self._lib, self._lib.sba_batch_upload_matches(
            self._h, _vptr(kl), lo.ctypes.data_as(C.c_void_p), _vptr(kr), ro.ctypes.data_as(C.c_void_p), B, stride, im_width,
            im_height, _vptr(dl), _vptr(dr), dim, dstride, ratio, dp, store, cnt.ctypes.data_as(C.c_void_p),
            ml.ctypes.data_as(C.c_void_p), mr.ctypes.data_as(C.c_void_p)))
        n = cnt[:B].astype(np.int64)
        off = np.zeros(B + 1, dtype=np.uint64)
        off[1:] = np.cumsum(n)
        self.num_pairs = B
        self._total = int(off[-1])
        self._offsets = off
        m = int(off[-1])
        return ml[:m].copy(), mr[:m].copy(), n

    def set_depths(self, d12) -> None:
        """Re-send only the per-match depths (total, 2), laid out like the d12 of upload(); the coordinates stay resident."""
        d = _f64(d12).reshape(-1, 2)
        if self.num_pairs and d.shape[0] != self._total:
            raise ValueError("d12 length differs from the uploaded pairs")
        cabi.check(self._lib, self._lib.sba_batch_set_depths(self._h, _dptr(d)))

    @property
    def offsets(self) -> np.ndarray:
        """Row offsets (num_pairs + 1,) of the current layout: as uploaded, or the exclusive scan of the kept counts after a
        compaction.  A copy."""
        return self._offsets.copy()

    @property
    def blocks_per_pair(self) -> int:
        n, b = C.c_int(0), C.c_int(0)
        cabi.check(self._lib, self._lib.sba_batch_size(self._h, C.byref(n), C.byref(b)))
        return b.value

    def _pp(self, a, width):
        if a is None:
            return None, None
        arr = _f64(a).reshape(self.num_pairs, width) if width > 1 else _f64(a).reshape(self.num_pairs)
        return arr, _dptr(arr)

    def eval(self, mode, rot, tran, d1=None, d2=None, huber_delta=1.0, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        """rot, tran: (num_pairs, 3).  Returns packs (num_pairs, 24) in the SBA_PACK layout."""
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        packs = np.zeros((self.num_pairs, cabi.PACK_SIZE))
        cabi.check(self._lib, self._lib.sba_batch_eval(self._h, mode, depth_mode, rp, tp, d1p, d2p, huber_delta,
                                                       _dptr(packs)))
        return packs

    def eval_timed(self, mode, rot, tran, steps, d1=None, d2=None, huber_delta=1.0, depth_mode=DEPTH_UNIFORM):
        """`steps` host-synchronous batched steps in a C loop.  Returns (packs, dict of mean ms: step / prepare /
        device / convert)."""
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        packs = np.zeros((self.num_pairs, cabi.PACK_SIZE))
        ms = [C.c_double(0) for _ in range(4)]
        cabi.check(self._lib, self._lib.sba_batch_eval_timed(
            self._h, mode, depth_mode, rp, tp, d1p, d2p, huber_delta, steps, _dptr(packs),
            *[C.cast(C.byref(m), C.POINTER(C.c_double)) for m in ms]))
        return packs, dict(zip(("step_ms", "prepare_ms", "device_ms", "convert_ms"), (m.value for m in ms)))

    def _launch_times(self, fn, mode, rot, tran, d1, d2, huber_delta, depth_mode, repeat) -> np.ndarray:
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        ms = np.zeros(repeat, dtype=np.float32)
        cabi.check(self._lib, fn(self._h, mode, depth_mode, rp, tp, d1p, d2p, huber_delta, repeat,
                                 ms.ctypes.data_as(C.POINTER(C.c_float))))
        return ms.astype(np.float64)

    def sweep_launch_times(self, mode, rot, tran, d1=None, d2=None, huber_delta=1.0, depth_mode=DEPTH_UNIFORM,
                           repeat: int = 20) -> np.ndarray:
        """Device time (ms) of each of `repeat` back-to-back launches of the batched sweep kernel alone."""
        return self._launch_times(self._lib.sba_batch_sweep_launch_times, mode, rot, tran, d1, d2, huber_delta, depth_mode,
                                  repeat)

    def step_launch_times(self, mode, rot, tran, d1=None, d2=None, huber_delta=1.0, depth_mode=DEPTH_UNIFORM,
                          repeat: int = 20) -> np.ndarray:
        """The same for the dominant kernel of the step this batch really runs (`step_is_fused`: the one-launch
        batch_step_kernel, else the batched sweep kernel)."""
        return self._launch_times(self._lib.sba_batch_step_launch_times, mode, rot, tran, d1, d2, huber_delta, depth_mode,
                                  repeat)

    @property
    def step_is_fused(self) -> bool:
        rc = self._lib.sba_batch_step_is_fused(self._h)
        if rc < 0:
            cabi.check(self._lib, rc)
        return rc == 1

    # -- single matches ---------------------------------------------------------------------------------
    def _rows(self) -> int:
        return int(self._offsets[-1]) - int(self._offsets[0])

    def residuals(self, rot, tran, d1=None, d2=None, huber_delta=1.0, depth_mode=DEPTH_UNIFORM,
                  fields=("e", "sq_norm", "inlier")) -> BatchResiduals:
        """Every pair's per-match residuals at its own (rot, tran) (B, 3), formed on the device as the batched sweep forms
        them; rows as in `offsets`.  `fields` picks the arrays copied back (any of "e", "sq_norm", "inlier"; empty = the
        per-pair inlier counts only).  n[g] - n_inlier[g] equals the pack's n_outlier of eval() at the same arguments."""
        unknown = set(fields) - {"e", "sq_norm", "inlier"}
        if unknown:
            raise ValueError(f"unknown residual fields {sorted(unknown)}")
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        rows = self._rows()
        e = np.empty((rows, 3)) if "e" in fields else None
        sq = np.empty(rows) if "sq_norm" in fields else None
        inl = np.empty(rows, dtype=np.uint8) if "inlier" in fields else None
        cnt = np.zeros(max(self.num_pairs, 1), dtype=np.uintp)
        cabi.check(self._lib, self._lib.sba_batch_residuals(
            self._h, depth_mode, rp, tp, d1p, d2p, huber_delta, None if e is None else _dptr(e),
            None if sq is None else _dptr(sq), None if inl is None else inl.ctypes.data_as(C.c_void_p),
            cnt.ctypes.data_as(C.POINTER(C.c_size_t))))
        return BatchResiduals(e, sq, None if inl is None else inl.view(np.bool_), cnt[:self.num_pairs].astype(np.int64))

    def _compacted(self, idx, n_kept):
        off = np.zeros(self.num_pairs + 1, dtype=np.uint64)
        off[1:] = np.cumsum(n_kept[:self.num_pairs], dtype=np.uint64)
        self._offsets = off
        self._total = int(off[-1])
        return idx[:self._total].copy(), off.copy()

    def compact(self, keep):
        """Keep the rows where `keep` (one entry per row of `offsets`) is true, in order; every pair keeps its own rows.  The
        handle then equals a fresh upload of the kept rows with offsets from 0.  Returns (kept row numbers (np.int64),
        the new offsets)."""
        k = np.ascontiguousarray(np.asarray(keep).reshape(-1) != 0, dtype=np.uint8)
        rows = self._rows()
        if k.shape[0] != rows:
            raise ValueError(f"keep has {k.shape[0]} entries, the batch holds {rows} rows")
        idx = np.empty(max(rows, 1), dtype=np.int64)
        nk = np.zeros(max(self.num_pairs, 1), dtype=np.uintp)
        cabi.check(self._lib, self._lib.sba_batch_compact(self._h, k.ctypes.data_as(C.c_void_p),
                                                          nk.ctypes.data_as(C.POINTER(C.c_size_t)),
                                                          idx.ctypes.data_as(C.c_void_p)))
        return self._compacted(idx, nk)

    def keep_inliers(self, rot, tran, d1=None, d2=None, huber_delta=1.0, depth_mode=DEPTH_UNIFORM):
        """Drop every pair's matches in Huber's outlier region at its (rot, tran): residuals() then compact(), with the
        inlier mask kept on the device.  Returns what compact() returns."""
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        idx = np.empty(max(self._rows(), 1), dtype=np.int64)
        nk = np.zeros(max(self.num_pairs, 1), dtype=np.uintp)
        cabi.check(self._lib, self._lib.sba_batch_keep_inliers(self._h, depth_mode, rp, tp, d1p, d2p, huber_delta,
                                                               nk.ctypes.data_as(C.POINTER(C.c_size_t)),
                                                               idx.ctypes.data_as(C.c_void_p)))
        return self._compacted(idx, nk)

    def _pair_ranks(self, probs):
        """(num_pairs, k) ranks floor(p * (n[g] - 1)) of every pair's own size (0 for an empty pair, which takes no part)."""
        n = np.diff(self._offsets.astype(np.int64))
        p = np.atleast_1d(np.asarray(probs, dtype=np.float64))
        return np.stack([quantile_rank(p, int(m)) if m > 0 else np.zeros(p.shape[0], dtype=np.uintp) for m in n]) \
            if self.num_pairs else np.zeros((0, p.shape[0]), dtype=np.uintp)

    def residual_order_stats(self, rot, tran, ranks, d1=None, d2=None, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        """Every pair's ranks[g][j]-th smallest (0-based) squared residual norm among its own rows at its own (rot, tran),
        all pairs in the same launches; `ranks` (num_pairs, k), k <= 8, or (k,) for every pair alike.  Returns
        (num_pairs, k): elements of ``residuals(...).sq_norm`` bit for bit, NaN for an empty pair."""
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        r = _ranks(ranks)
        if r.ndim == 1:
            r = np.ascontiguousarray(np.broadcast_to(r, (self.num_pairs, r.shape[0])))
        if r.ndim != 2 or r.shape[0] != self.num_pairs:
            raise ValueError(f"ranks has shape {r.shape}, the batch holds {self.num_pairs} pairs")
        vals = np.full((max(self.num_pairs, 1), r.shape[1]), np.nan)
        cabi.check(self._lib, self._lib.sba_batch_residual_order_stats(
            self._h, depth_mode, rp, tp, d1p, d2p, r.ctypes.data_as(C.POINTER(C.c_size_t)), r.shape[1], _dptr(vals)))
        return vals[:self.num_pairs]

    def residual_quantiles(self, rot, tran, probs, d1=None, d2=None, depth_mode=DEPTH_UNIFORM) -> np.ndarray:
        """residual_order_stats at every pair's own ranks floor(p * (n[g] - 1)) (`quantile_rank` of the pair's size)."""
        return self.residual_order_stats(rot, tran, self._pair_ranks(probs), d1, d2, depth_mode)

    def keep_below(self, rot, tran, prob, scale, d1=None, d2=None, depth_mode=DEPTH_UNIFORM):
        """Every pair keeps its rows with sq_norm <= scale[g] * (its own `prob` quantile of sq_norm); thresholds and flags
        stay on the device, then compact()'s layout.  `prob` and `scale`: a number or one per pair.  Returns (kept row
        numbers, the new offsets, the per-pair thresholds (NaN for an empty pair)).  `scale` has no default on purpose: the
        right multiple of the right quantile depends on the stage (see Problem.keep_below)."""
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        B = self.num_pairs
        n = np.diff(self._offsets.astype(np.int64))
        prob = np.broadcast_to(np.asarray(prob, dtype=np.float64), (B,))
        rank = np.array([int(quantile_rank(prob[g], int(n[g]))[0]) if n[g] > 0 else 0 for g in range(B)] + [0] * (B == 0),
                        dtype=np.uintp)
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (max(B, 1),)))
        thr = np.full(max(B, 1), np.nan)
        idx = np.empty(max(self._rows(), 1), dtype=np.int64)
        nk = np.zeros(max(B, 1), dtype=np.uintp)
        cabi.check(self._lib, self._lib.sba_batch_keep_below(
            self._h, depth_mode, rp, tp, d1p, d2p, rank.ctypes.data_as(C.POINTER(C.c_size_t)), _dptr(sc), _dptr(thr),
            nk.ctypes.data_as(C.POINTER(C.c_size_t)), idx.ctypes.data_as(C.c_void_p)))
        return (*self._compacted(idx, nk), thr[:B].copy())

    def solve(self, mode, rot, tran, d1=None, d2=None, depth_mode=DEPTH_UNIFORM, options: cabi.LmOptions | None = None):
        """Per-pair LM in lock-step.  Returns (rot (B,3), tran (B,3), [SolveSummary], status (B,))."""
        rot = _f64(rot).reshape(self.num_pairs, 3).copy()
        tran = _f64(tran).reshape(self.num_pairs, 3).copy()
        d1a, d1p = self._pp(d1, 1)
        d2a, d2p = self._pp(d2, 1)
        opt = options if options is not None else default_lm_options()
        sums = (cabi.LmSummary * max(self.num_pairs, 1))()
        status = np.zeros(max(self.num_pairs, 1), dtype=np.int32)
        cabi.check(self._lib, self._lib.sba_batch_solve(self._h, mode, depth_mode, _dptr(rot), _dptr(tran), d1p, d2p,
                                                        C.byref(opt), sums, status.ctypes.data_as(C.POINTER(C.c_int))))
        return rot, tran, [_summary(sums[i]) for i in range(self.num_pairs)], status[:self.num_pairs]

    def solve_depths(self, rot, tran, lam: float = 1.0, c: float = 1.0, options: cabi.LmOptions | None = None,
                     total_matches: int | None = None, want_depths: bool = True):
        """The d-only stage for every pair (its own trust region / line search / convergence each), in lock-step.
        Returns (d12 (offsets[-1], 2) indexed like the uploaded depths, [SolveSummary], status (B,))."""
        rot = _f64(rot).reshape(self.num_pairs, 3)
        tran = _f64(tran).reshape(self.num_pairs, 3)
        opt = options if options is not None else default_lm_options()
        total = int(self._total) if total_matches is None else int(total_matches)
        d12 = np.zeros((total, 2)) if want_depths else None           # None: the refined depths stay on the device only
        sums = (cabi.LmSummary * max(self.num_pairs, 1))()
        status = np.zeros(max(self.num_pairs, 1), dtype=np.int32)
        cabi.check(self._lib, self._lib.sba_batch_solve_depths(self._h, _dptr(rot), _dptr(tran), lam, c, C.byref(opt),
                                                               d12.ctypes.data_as(C.c_void_p) if want_depths else None, sums,
                                                               status.ctypes.data_as(C.POINTER(C.c_int))))
        return d12, [_summary(sums[i]) for i in range(self.num_pairs)], status[:self.num_pairs]


    # -- joint solve: every pair's depths, rotation and translation together ----------------------------
    def eval_joint(self, rot, tran, radius=float("inf"), options: cabi.LmOptions | None = None):
        """One reduce pass of the joint solve per pair at (rot[g], tran[g]) and the batch's depths; `radius` sets the depth
        damping (inf: none).  options None = the defaults with tran_param = TRAN_SPHERE.  Returns a list of JointEquations."""
        rot, rp = self._pp(rot, 3)
        tran, tp = self._pp(tran, 3)
        eqs = (cabi.JointEq * max(self.num_pairs, 1))()
        cabi.check(self._lib, self._lib.sba_batch_eval_joint(self._h, rp, tp, float(radius),
                                                             None if options is None else C.byref(options), eqs))
        a = lambda v, shape: np.array(v, dtype=np.float64).reshape(shape)
        return [JointEquations(a(e.S, (6, 6)), a(e.gs, (6,)), a(e.V, (6, 6)), a(e.gc, (6,)), float(e.cost), float(e.sum_w),
                               float(e.n_outlier), float(e.gd_max)) for e in eqs[:self.num_pairs]]

    def solve_joint(self, rot, tran, options: cabi.LmOptions | None = None, return_depths: bool = True, check: bool = True):
        """Joint LM per pair over the batch's per-match depths and the pair's camera from (rot[g], tran[g]): the reference's
        joint functor for every pair.  The refined depths stay in the batch.  options None = the defaults with tran_param =
        TRAN_SPHERE (|tran| pinned per pair).  Returns (rot (B, 3), tran (B, 3), d12 (offsets[-1], 2) or None, [SolveSummary],
        status (B,)); inputs are not modified.  check=False: pairs that failed are reported in status only."""
        B = self.num_pairs
        rot = _f64(rot).reshape(B, 3).copy()
        tran = _f64(tran).reshape(B, 3).copy()
        d12 = np.zeros((int(self._total), 2)) if return_depths else None
        sums = (cabi.LmSummary * max(B, 1))()
        status = np.zeros(max(B, 1), dtype=np.int32)
        rc = self._lib.sba_batch_solve_joint(self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options), sums,
                                             status.ctypes.data_as(C.POINTER(C.c_int)),
                                             None if d12 is None else d12.ctypes.data_as(C.c_void_p))
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        return rot, tran, d12, [_summary(sums[i]) for i in range(B)], status[:B]

    def covariance_joint(self, rot, tran, options: cabi.LmOptions | None = None, min_sin2_parallax: float = 0.0,
                         depths: bool = True, check: bool = True) -> BatchJointCovariance:
        """Covariance of every pair's joint problem at (rot[g], tran[g]) and the batch's depths, in one launch: per pair what
        Problem.covariance_joint gives on that pair alone.  depths=False skips the per-match blocks.  options None = the
        defaults with tran_param = TRAN_SPHERE.  A pair without a covariance (non-finite point, too few used matches, a
        rank-deficient system) has status SBA_ERR_NUMERIC and NaN blocks; check=True raises SbaError then, check=False returns
        the result with status, as solve_joint does.  The batch's state is not touched."""
        B = self.num_pairs
        rot = _f64(rot).reshape(B, 3)
        tran = _f64(tran).reshape(B, 3)
        res = (cabi.JointCov * max(B, 1))()
        dd = np.zeros((int(self._total), 3)) if depths else None
        status = np.zeros(max(B, 1), dtype=np.int32)
        rc = self._lib.sba_batch_covariance_joint(self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options),
                                                  float(min_sin2_parallax), res, None if dd is None else _dptr(dd),
                                                  status.ctypes.data_as(C.POINTER(C.c_int)))
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        r = res[:B]
        return BatchJointCovariance(np.array([list(e.cov) for e in r], dtype=np.float64).reshape(B, 6, 6), dd,
                                    np.array([e.cost for e in r], dtype=np.float64), np.array([e.sum_w for e in r], dtype=np.float64),
                                    np.array([e.n_used for e in r], dtype=np.int64), np.array([e.n_degenerate for e in r], dtype=np.int64),
                                    np.array([e.dim for e in r], dtype=np.int32), np.array([e.dof for e in r], dtype=np.int32),
                                    status[:B].copy(), np.asarray(self.offsets, dtype=np.int64).copy())

    def _batch_joint_cov(self, res, status) -> BatchJointCovariance:
        B = self.num_pairs
        r = res[:B]
        return BatchJointCovariance(np.array([list(e.cov) for e in r], dtype=np.float64).reshape(B, 6, 6), None,
                                    np.array([e.cost for e in r], dtype=np.float64), np.array([e.sum_w for e in r], dtype=np.float64),
                                    np.array([e.n_used for e in r], dtype=np.int64), np.array([e.n_degenerate for e in r], dtype=np.int64),
                                    np.array([e.dim for e in r], dtype=np.int32), np.array([e.dof for e in r], dtype=np.int32),
                                    status[:B].copy(), np.asarray(self.offsets, dtype=np.int64).copy())

    def structure_joint(self, rot, tran, options: cabi.LmOptions | None = None, min_sin2_parallax: float = 0.0,
                        xyz: bool = True, cov: bool = True, score: bool = True, check: bool = True) -> BatchJointStructure:
        """One 3-D point per match of every pair at (rot[g], tran[g]) and the batch's depths, with its covariance and score
        (BatchJointStructure): per pair what Problem.structure_joint gives on that pair alone.  xyz / cov / score = False
        skips that output (it is then None).  A pair without a covariance has status SBA_ERR_NUMERIC and NaN rows; check=True
        raises SbaError then, check=False returns the result with status, as covariance_joint does.  The batch's state is
        not touched."""
        B = self.num_pairs
        rot = _f64(rot).reshape(B, 3)
        tran = _f64(tran).reshape(B, 3)
        res = (cabi.JointCov * max(B, 1))()
        rows = int(self._total)
        X = np.zeros((rows, 3)) if xyz else None
        Cv = np.zeros((rows, 6)) if cov else None
        q = np.zeros(rows) if score else None
        status = np.zeros(max(B, 1), dtype=np.int32)
        ptr = lambda a: None if a is None else _dptr(a)
        rc = self._lib.sba_batch_structure_joint(self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options),
                                                 float(min_sin2_parallax), res, ptr(X), ptr(Cv), ptr(q),
                                                 status.ctypes.data_as(C.POINTER(C.c_int)))
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        return BatchJointStructure(X, Cv, q, self._batch_joint_cov(res, status))

    def structure_joint_into(self, xyz_ptr, cov_ptr, score_ptr, rot, tran, options: cabi.LmOptions | None = None,
                             min_sin2_parallax: float = 0.0, check: bool = True) -> BatchJointCovariance:
        """structure_joint with the outputs stored straight into DEVICE memory: xyz_ptr / cov_ptr / score_ptr are device
        addresses (for example ``tensor.data_ptr()`` of float64 tensors of rows * 3, rows * 6 and rows elements on the
        batch's device, rows = offsets[-1] - offsets[0], the batch's own rows), 16-byte aligned, 0 or None to skip an output.
        Returns the pose record; nothing else crosses to the host."""
        B = self.num_pairs
        rot = _f64(rot).reshape(B, 3)
        tran = _f64(tran).reshape(B, 3)
        res = (cabi.JointCov * max(B, 1))()
        status = np.zeros(max(B, 1), dtype=np.int32)
        vp = lambda a: C.c_void_p(int(a)) if a else None
        rc = self._lib.sba_batch_structure_joint_device(self._h, _dptr(rot), _dptr(tran),
                                                        None if options is None else C.byref(options), float(min_sin2_parallax),
                                                        res, vp(xyz_ptr), vp(cov_ptr), vp(score_ptr),
                                                        status.ctypes.data_as(C.POINTER(C.c_int)))
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        return self._batch_joint_cov(res, status)

    def structure_order_stats(self, rot, tran, ranks, options: cabi.LmOptions | None = None, min_sin2_parallax: float = 0.0,
                              check: bool = True):
        """Every pair's ranks[g][j]-th smallest (0-based) of its own structure_joint scores, selected on the device: bit for
        bit elements of that pair's score rows; inf (degenerate matches) sorts above every finite score.  `ranks`
        (num_pairs, k), k <= 8, or (k,) for every pair alike.  Returns ((num_pairs, k) values, status (num_pairs,)): NaN
        values for an empty pair and for a pair without a covariance (status SBA_ERR_NUMERIC; check=True raises then)."""
        B = self.num_pairs
        rot = _f64(rot).reshape(B, 3)
        tran = _f64(tran).reshape(B, 3)
        r = _ranks(ranks)
        if r.ndim == 1:
            r = np.ascontiguousarray(np.broadcast_to(r, (B, r.shape[0])))
        if r.ndim != 2 or r.shape[0] != B:
            raise ValueError(f"ranks has shape {r.shape}, the batch holds {B} pairs")
        vals = np.full((max(B, 1), r.shape[1]), np.nan)
        status = np.zeros(max(B, 1), dtype=np.int32)
        rc = self._lib.sba_batch_structure_order_stats(
            self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options), float(min_sin2_parallax),
            r.ctypes.data_as(C.POINTER(C.c_size_t)), r.shape[1], _dptr(vals), status.ctypes.data_as(C.POINTER(C.c_int)))
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        return vals[:B], status[:B]

    def structure_keep_below(self, rot, tran, prob, scale, options: cabi.LmOptions | None = None,
                             min_sin2_parallax: float = 0.0, check: bool = True):
        """Every pair keeps its rows with score <= scale[g] * (its own `prob` quantile of the scores, rank `quantile_rank` of
        the pair's size), selected, flagged and compacted on the device as keep_below does; the batch then equals a fresh
        upload of the kept rows.  Degenerate matches (score inf) go unless the pair's threshold itself is inf.  A pair without
        a covariance is not cut: it keeps every row, its threshold is NaN and its status SBA_ERR_NUMERIC; check=True raises
        SbaError then -- AFTER the other pairs were cut, and `offsets` is up to date either way.  `prob` and `scale`: a number
        or one per pair.  Returns (kept row numbers, the new offsets, the per-pair thresholds, status (num_pairs,))."""
        B = self.num_pairs
        rot = _f64(rot).reshape(B, 3)
        tran = _f64(tran).reshape(B, 3)
        n = np.diff(self._offsets.astype(np.int64))
        prob = np.broadcast_to(np.asarray(prob, dtype=np.float64), (B,))
        rank = np.array([int(quantile_rank(prob[g], int(n[g]))[0]) if n[g] > 0 else 0 for g in range(B)] + [0] * (B == 0),
                        dtype=np.uintp)
        sc = np.ascontiguousarray(np.broadcast_to(np.asarray(scale, dtype=np.float64), (max(B, 1),)))
        thr = np.full(max(B, 1), np.nan)
        idx = np.empty(max(self._rows(), 1), dtype=np.int64)
        nk = np.zeros(max(B, 1), dtype=np.uintp)
        status = np.zeros(max(B, 1), dtype=np.int32)
        rc = self._lib.sba_batch_structure_keep_below(
            self._h, _dptr(rot), _dptr(tran), None if options is None else C.byref(options), float(min_sin2_parallax),
            rank.ctypes.data_as(C.POINTER(C.c_size_t)), _dptr(sc), _dptr(thr), nk.ctypes.data_as(C.POINTER(C.c_size_t)),
            idx.ctypes.data_as(C.c_void_p), status.ctypes.data_as(C.POINTER(C.c_int)))
        if rc not in (cabi.SBA_OK, cabi.SBA_ERR_NUMERIC):
            cabi.check(self._lib, rc)
        out = (*self._compacted(idx, nk), thr[:B].copy(), status[:B].copy())     # the cut took place: the offsets follow it
        if check:
            cabi.check(self._lib, rc)
        return out

    def solve_problem(self, rot=None, tran=None, use_initial_guess: bool = True, trials: int = 80, subset_fraction: float = 0.25,
                      seed: int = 0, options: cabi.LmOptions | None = None, want_depths: bool = False, check: bool = True,
                      joint: bool = False):
        """The reference's per-pair pipeline for every pair (initial guess -> d-only -> rot-only -> tran-only,
        reference .cpp:302-331, :183-217).  rot / tran: start values (B, 3) (needed when use_initial_guess is False; with the
        guess they only serve pairs that have no valid candidate).  Returns a dict: rot, tran (B, 3), d_uniform (B, 2),
        guess_candidates (B,), depth / rot / tran stage summaries, status (B,), d12 (if want_depths).
        joint=True: solve_joint() follows the tran-only stage, from that stage's rot / tran and the refined depths; the dict
        then also holds joint_rot, joint_tran (B, 3), joint_stage summaries, joint_status (B,) and joint_d12 (if want_depths)."""
        B = self.num_pairs
        r = np.zeros((max(B, 1), 3)) if rot is None else _f64(rot).reshape(B, 3).copy()
        t = np.zeros((max(B, 1), 3)) if tran is None else _f64(tran).reshape(B, 3).copy()
        opt = options if options is not None else default_lm_options()
        d12 = np.zeros((int(self._total), 2)) if want_depths else None
        du = np.zeros((max(B, 1), 2))
        nc, status = np.zeros(max(B, 1), dtype=np.int32), np.zeros(max(B, 1), dtype=np.int32)
        sums = [(cabi.LmSummary * max(B, 1))() for _ in range(3)]
        t0 = time.perf_counter()
        rc = self._lib.sba_batch_solve_problem(self._h, 1 if use_initial_guess else 0, trials, subset_fraction, seed, _dptr(r), _dptr(t),
                                               C.byref(opt), d12.ctypes.data_as(C.c_void_p) if want_depths else None, _dptr(du),
                                               nc.ctypes.data_as(C.POINTER(C.c_int)), sums[0], sums[1], sums[2],
                                               status.ctypes.data_as(C.POINTER(C.c_int)))
        seconds = time.perf_counter() - t0       # the library call alone (the summaries below are 3 B Python objects)
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        res = {"rot": r[:B], "tran": t[:B], "d_uniform": du[:B], "guess_candidates": nc[:B], "status": status[:B], "d12": d12,
                "seconds_inside_the_library": seconds,
                "depth_stage": [_summary(sums[0][i]) for i in range(B)], "rot_stage": [_summary(sums[1][i]) for i in range(B)],
                "tran_stage": [_summary(sums[2][i]) for i in range(B)]}
        if joint:
            jr, jt, jd, js, jst = self.solve_joint(r[:B], t[:B], return_depths=want_depths, check=check)
            res.update(joint_rot=jr, joint_tran=jt, joint_d12=jd, joint_stage=js, joint_status=jst)
        return res

    def epipolar_moments(self):
        """Group moments of every pair: (B, 64, 45)."""
        g = np.zeros((max(self.num_pairs, 1), 64, 45))
        cabi.check(self._lib, self._lib.sba_batch_epipolar_moments(self._h, _dptr(g)))
        return g[:self.num_pairs]

    def initial_guess(self, trials: int = 80, subset_fraction: float = 0.25, seed: int = 0, check: bool = True):
        """The 8-point initial guess of every pair (reference initial_guess, .cpp:47-181, once per pair).
        Returns (rot_euler (B, 3), tran (B, 3), num_candidates (B,), status (B,)); check=False: a pair without a valid
        candidate is reported in status only."""
        B = self.num_pairs
        e, t = np.zeros((max(B, 1), 3)), np.zeros((max(B, 1), 3))
        nc, status = np.zeros(max(B, 1), dtype=np.int32), np.zeros(max(B, 1), dtype=np.int32)
        rc = self._lib.sba_batch_initial_guess(self._h, trials, subset_fraction, seed, _dptr(e), _dptr(t),
                                               nc.ctypes.data_as(C.POINTER(C.c_int)), status.ctypes.data_as(C.POINTER(C.c_int)))
        if check or rc != cabi.SBA_ERR_NUMERIC:
            cabi.check(self._lib, rc)
        return e[:B], t[:B], nc[:B], status[:B]


def set_host_threads(n: int) -> None:
    """Host threads for the host-side trial loop of the initial guess (reference: set_omp).  0 = auto."""
    lib = cabi.load_library()
    cabi.check(lib, lib.sba_set_host_threads(n))


def initial_guess_from_moments(groups, trials: int = 80, subset_fraction: float = 0.25, seed: int = 0):
    """Host-only part of the initial guess (no device needed)."""
    lib = cabi.load_library()
    g = _f64(groups, (64, 45))
    e, t, n = np.zeros(3), np.zeros(3), C.c_int(0)
    cabi.check(lib, lib.sba_initial_guess_from_moments(_dptr(g), trials, subset_fraction, seed, _dptr(e), _dptr(t),
                                                       C.byref(n)))
    return e, t, n.value


def reference_rand_seed(seed: int = 1) -> None:
    """Reset the library's copy of the reference's rand() stream (1 = the never-seeded state a fresh process starts in)."""
    lib = cabi.load_library()
    cabi.check(lib, lib.sba_reference_rand_seed(seed))


def reference_rand_next() -> int:
    return int(cabi.load_library().sba_reference_rand_next())


def reference_trial_subsets(n: int, trials: int = 80, subset_fraction: float = 0.25) -> np.ndarray:
    """Host-only: (trials, int(n * subset_fraction)) match indices the reference's trials draw from the library's copy of
    the reference's rand() stream at this point (sba_reference_trial_subsets)."""
    lib = cabi.load_library()
    m = C.c_int(0)
    cabi.check(lib, lib.sba_reference_trial_subsets(n, trials, subset_fraction, None, C.byref(m)))
    out = np.zeros((trials, m.value), dtype=np.int32)
    cabi.check(lib, lib.sba_reference_trial_subsets(n, trials, subset_fraction, out.ctypes.data_as(C.c_void_p), C.byref(m)))
    return out


def rccl_available() -> bool:
    """librccl loadable and bound in this process (checked on every rank before anyone enters ncclCommInitRank)."""
    return bool(cabi.load_library().sba_rccl_available())


def comm_unique_id() -> bytes:
    lib = cabi.load_library()
    buf = C.create_string_buffer(cabi.COMM_ID_BYTES)
    cabi.check(lib, lib.sba_comm_unique_id(buf))
    return buf.raw

def match_descriptors(query, train, ratio: float = 0.3, device: int = 0) -> Matches:
    """feature_matcher::match_two_image on the device: exact L2 2-NN of every query row (n_query, dim) among the train rows
    (n_train, dim) (f32; 1 <= dim <= 256), then the ratio test d0 < ratio * d1 (reference: 0.3).  The accepted matches come
    in ascending query order, like the reference's good_matches."""
    lib = cabi.load_library()
    (q, t), dim, stride = _descriptors(query, train)
    nq = q.shape[0]
    nn_i, nn_d = np.zeros((max(nq, 1), 2), dtype=np.int32), np.zeros((max(nq, 1), 2), dtype=np.float32)
    mq, mt, md = (np.zeros(max(nq, 1), dtype=np.int32), np.zeros(max(nq, 1), dtype=np.int32),
                  np.zeros(max(nq, 1), dtype=np.float32))
    n = C.c_size_t()
    cabi.check(lib, lib.sba_match_descriptors(device, _vptr(q), nq, _vptr(t), t.shape[0], dim, stride, ratio,
                                              nn_i.ctypes.data_as(C.c_void_p), nn_d.ctypes.data_as(C.c_void_p), C.byref(n),
                                              mq.ctypes.data_as(C.c_void_p), mt.ctypes.data_as(C.c_void_p),
                                              md.ctypes.data_as(C.c_void_p)))
    m = n.value
    return Matches(nn_i[:nq], nn_d[:nq], mq[:m].copy(), mt[:m].copy(), md[:m].copy())


def batch_match_descriptors(query, query_offsets, train, train_offsets, ratio: float = 0.3, device: int = 0) -> BatchMatches:
    """match_descriptors for many pairs in one launch: pair g = query rows query_offsets[g] .. [g + 1] against train rows
    train_offsets[g] .. [g + 1].  nn_* are indexed by query row - query_offsets[0]."""
    lib = cabi.load_library()
    (q, t), dim, stride = _descriptors(query, train)
    qo, to = _offsets(query_offsets, "query"), _offsets(train_offsets, "train")
    if qo.size != to.size:
        raise ValueError("query/train offsets differ in length")
    B = qo.size - 1
    if B and (int(qo[-1]) > q.shape[0] or int(to[-1]) > t.shape[0]):
        raise ValueError("offsets run past the arrays")
    nq = int(qo[-1] - qo[0]) if B else 0
    nn_i, nn_d = np.zeros((max(nq, 1), 2), dtype=np.int32), np.zeros((max(nq, 1), 2), dtype=np.float32)
    mq, mt, md = (np.zeros(max(nq, 1), dtype=np.int32), np.zeros(max(nq, 1), dtype=np.int32),
                  np.zeros(max(nq, 1), dtype=np.float32))
    cnt = np.zeros(max(B, 1), dtype=np.uint64)
    cabi.check(lib, lib.sba_batch_match_descriptors(device, _vptr(q), qo.ctypes.data_as(C.c_void_p), _vptr(t),
                                                    to.ctypes.data_as(C.c_void_p), B, dim, stride, ratio,
                                                    nn_i.ctypes.data_as(C.c_void_p), nn_d.ctypes.data_as(C.c_void_p),
                                                    cnt.ctypes.data_as(C.c_void_p), mq.ctypes.data_as(C.c_void_p),
                                                    mt.ctypes.data_as(C.c_void_p), md.ctypes.data_as(C.c_void_p)))
    n = cnt[:B].astype(np.int64)
    off = np.zeros(B + 1, dtype=np.int64)
    off[1:] = np.cumsum(n)
    m = int(off[-1])
    return BatchMatches(nn_i[:nq], nn_d[:nq], n, off, mq[:m].copy(), mt[:m].copy(), md[:m].copy())



def keypoints_to_sphere(keypoints: np.ndarray, im_width: int, im_height: int, device: int = 0) -> np.ndarray:
    """keypoints: structured/2-D array whose rows start with float32 pt.x, pt.y (cv::KeyPoint: 28 B)."""
    lib = cabi.load_library()
    kp = np.ascontiguousarray(keypoints)
    n = kp.shape[0]
    stride = kp.strides[0] if n > 0 else 28
    out = np.zeros((n, 3))
    cabi.check(lib, lib.sba_keypoints_to_sphere(device, kp.ctypes.data_as(C.c_void_p), n, stride, im_width,
                                                im_height, out.ctypes.data_as(C.c_void_p)))
    return out


def equi2cube(erp: np.ndarray, cube_size: int, device: int = 0) -> np.ndarray:
    """erp: (H, W, 3) uint8 -> (S, 6S, 3) uint8 strip, faces left,front,right,back,top,bottom."""
    lib = cabi.load_library()
    im = np.ascontiguousarray(erp, dtype=np.uint8)
    if im.ndim != 3 or im.shape[2] != 3:
        raise ValueError("erp must be (H, W, 3) uint8")
    out = np.zeros((cube_size, 6 * cube_size, 3), dtype=np.uint8)
    cabi.check(lib, lib.sba_equi2cube(device, im.ctypes.data_as(C.c_void_p), im.shape[0], im.shape[1], cube_size,
                                      out.ctypes.data_as(C.c_void_p)))
    return out


def _kp_inplace(fn, keypoints: np.ndarray, *args, device: int = 0) -> np.ndarray:
    lib = cabi.load_library()
    kp = np.ascontiguousarray(keypoints).copy()
    n = kp.shape[0]
    stride = kp.strides[0] if n > 0 else 28
    cabi.check(lib, getattr(lib, fn)(device, kp.ctypes.data_as(C.c_void_p), n, stride, *args))
    return kp


def rotate_keypoints(keypoints: np.ndarray, pitch_deg: float, im_width: int, im_height: int, device: int = 0):
    """spherical_surf::rotate_keypoint on cv::KeyPoint-like records (first two float32 = pt.x, pt.y); returns a copy."""
    return _kp_inplace("sba_rotate_keypoints", keypoints, C.c_float(pitch_deg), im_width, im_height, device=device)


def cube2equi_keypoints(keypoints: np.ndarray, cube_size: int, im_width: int, im_height: int, device: int = 0):
    """equi2cube_surf::cube2equi_pixel on key-point records; returns a copy."""
    return _kp_inplace("sba_cube2equi_keypoints", keypoints, cube_size, im_width, im_height, device=device)


def crop_rotated_image(erp: np.ndarray, pitch_deg: float, device: int = 0) -> np.ndarray:
    """spherical_surf::crop_rotated_image: (H, W, 3) uint8 -> (H//4, W, 3) rotated equatorial band."""
    lib = cabi.load_library()
    im = np.ascontiguousarray(erp, dtype=np.uint8)
    if im.ndim != 3 or im.shape[2] != 3:
        raise ValueError("erp must be (H, W, 3) uint8")
    out = np.zeros((im.shape[0] // 4, im.shape[1], 3), dtype=np.uint8)
    cabi.check(lib, lib.sba_crop_rotated_image(device, im.ctypes.data_as(C.c_void_p), im.shape[0], im.shape[1],
                                               C.c_float(pitch_deg), out.ctypes.data_as(C.c_void_p)))
    return out
