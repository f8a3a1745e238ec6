"""ctypes binding of the C-ABI in ``include/sba_hip.h`` (``libsba_hip.so``).

This is plumbing only: every call lands in the HIP library.  There is no Python or CPU
implementation of the hot path in this package; if the shared library is missing the import
fails loudly (``LibraryNotBuilt``), and without a HIP device every compute call raises ``SbaError``.
"""
from __future__ import annotations

import ctypes as C
import os
from pathlib import Path

PKG_DIR = Path(__file__).resolve().parent
LIB_PATH = PKG_DIR / "libsba_hip.so"

# status codes / enums (mirror include/sba_hip.h)
SBA_OK = 0
SBA_ERR_INVALID_ARG, SBA_ERR_NO_DEVICE, SBA_ERR_HIP, SBA_ERR_NOT_UPLOADED = -1, -2, -3, -4
SBA_ERR_COMM, SBA_ERR_NUMERIC, SBA_ERR_UNSUPPORTED = -5, -6, -7
MODE_ROT, MODE_TRAN, MODE_RT = 0, 1, 2
DEPTH_UNIFORM, DEPTH_PER_MATCH = 0, 1
STORE_F64, STORE_F32 = 0, 1
TRAN_FREE, TRAN_SPHERE = 0, 1
KERNEL_FACTORED, KERNEL_EXPLICIT = 0, 1
PACK_SIZE = 24
ABI_VERSION = 2          # SBA_ABI_VERSION of include/sba_hip.h
COMM_ID_BYTES = 128
PEER_HANDLE_BYTES = 64
TERMINATION = {1: "CONVERGENCE_FUNCTION", 2: "CONVERGENCE_GRADIENT", 3: "CONVERGENCE_PARAMETER",
               4: "NO_CONVERGENCE", 5: "MIN_RADIUS", 6: "FAILURE"}


class LibraryNotBuilt(ImportError):
    pass


class SbaError(RuntimeError):
    def __init__(self, code: int, message: str):
        super().__init__(f"sba error {code}: {message}")
        self.code = code
        self.message = message


class NormalEq(C.Structure):
    _fields_ = [("H", C.c_double * 36), ("g", C.c_double * 6), ("cost", C.c_double),
                ("sum_w", C.c_double), ("n_outlier", C.c_double)]


class JointEq(C.Structure):
    _fields_ = [("S", C.c_double * 36), ("gs", C.c_double * 6), ("V", C.c_double * 36), ("gc", C.c_double * 6),
                ("cost", C.c_double), ("sum_w", C.c_double), ("n_outlier", C.c_double), ("gd_max", C.c_double)]


class JointCov(C.Structure):
    _fields_ = [("cov", C.c_double * 36), ("cost", C.c_double), ("sum_w", C.c_double), ("n_used", C.c_longlong),
                ("n_degenerate", C.c_longlong), ("dim", C.c_int), ("dof", C.c_int)]


class ResectionEq(C.Structure):
    _fields_ = [("eq", NormalEq), ("n_behind", C.c_double)]


class ResectionGuessInfo(C.Structure):
    _fields_ = [("lambda1", C.c_double), ("lambda2", C.c_double), ("lambda12", C.c_double), ("sv", C.c_double * 3),
                ("scale", C.c_double), ("n", C.c_longlong), ("n_behind", C.c_double)]


class ResectionConsensusOptions(C.Structure):
    _fields_ = [("trials", C.c_int), ("sample_size", C.c_int), ("seed", C.c_ulonglong), ("threshold", C.c_double),
                ("refit", C.c_int)]


class ResectionConsensusInfo(C.Structure):
    _fields_ = [("n", C.c_longlong), ("n_inlier", C.c_longlong), ("best_trial", C.c_longlong),
                ("best_trial_inliers", C.c_longlong), ("n_valid_trials", C.c_longlong), ("refit_used", C.c_int),
                ("refit", ResectionGuessInfo), ("n_behind", C.c_double)]


class ResectionCov(C.Structure):
    _fields_ = [("cov", C.c_double * 36), ("cost", C.c_double), ("sum_w", C.c_double), ("n_used", C.c_longlong),
                ("n_zero_weight", C.c_longlong), ("n_outlier", C.c_double), ("dof", C.c_longlong), ("sigma2", C.c_double)]


class LandmarkFuseOptions(C.Structure):
    _fields_ = [("bearing_sigma", C.c_double), ("chi2_gate", C.c_double), ("pose_cov", C.POINTER(C.c_double)), ("apply", C.c_int)]


class LandmarkFuseResult(C.Structure):
    _fields_ = [("n_obs", C.c_longlong), ("n_skipped", C.c_longlong), ("n_behind", C.c_longlong), ("n_gated", C.c_longlong),
                ("n_fused", C.c_longlong)]


class LandmarkPruneOptions(C.Structure):
    _fields_ = [("max_score", C.c_double), ("min_count", C.c_uint32), ("mask", C.POINTER(C.c_uint8)), ("apply", C.c_int)]


class LandmarkPruneResult(C.Structure):
    _fields_ = [("n_before", C.c_longlong), ("n_invalid", C.c_longlong), ("n_uncertain", C.c_longlong), ("n_unobserved", C.c_longlong),
                ("n_masked", C.c_longlong), ("n_kept", C.c_longlong)]


class LmOptions(C.Structure):
    _fields_ = [("max_num_iterations", C.c_int),
                ("initial_trust_region_radius", C.c_double),
                ("max_trust_region_radius", C.c_double),
                ("min_trust_region_radius", C.c_double),
                ("min_relative_decrease", C.c_double),
                ("min_lm_diagonal", C.c_double),
                ("max_lm_diagonal", C.c_double),
                ("function_tolerance", C.c_double),
                ("gradient_tolerance", C.c_double),
                ("parameter_tolerance", C.c_double),
                ("jacobi_scaling", C.c_int),
                ("huber_delta", C.c_double),
                ("tran_param", C.c_int),
                ("verbose", C.c_int),
                ("max_num_line_search_step_size_iterations", C.c_int),
                ("line_search_sufficient_function_decrease", C.c_double),
                ("max_line_search_step_contraction", C.c_double),
                ("min_line_search_step_contraction", C.c_double),
                ("min_line_search_step_size", C.c_double)]


class LmSummary(C.Structure):
    _fields_ = [("termination", C.c_int), ("num_iterations", C.c_int),
                ("num_successful_steps", C.c_int), ("num_evaluations", C.c_int),
                ("initial_cost", C.c_double), ("final_cost", C.c_double),
                ("final_gradient_max_norm", C.c_double), ("final_radius", C.c_double),
                ("seconds_total", C.c_double), ("seconds_eval", C.c_double),
                ("num_line_search_steps", C.c_int)]


class LandmarkAssociateOptions(C.Structure):
    _fields_ = [("ratio", C.c_float), ("max_distance", C.c_float)]


class LandmarkAssociateResult(C.Structure):
    _fields_ = [("n_frame", C.c_longlong), ("n_accepted", C.c_longlong), ("n_contested", C.c_longlong), ("n_associated", C.c_longlong)]


class LandmarkRegisterOptions(C.Structure):
    _fields_ = [("bearing_sigma", C.c_double), ("chi2_gate", C.c_double), ("apply", C.c_int), ("lm", LmOptions)]


class LandmarkRegisterResult(C.Structure):
    _fields_ = [("rot", C.c_double * 3), ("tran", C.c_double * 3), ("cov", C.c_double * 36), ("summary", LmSummary),
                ("n_obs", C.c_longlong), ("n_skipped", C.c_longlong), ("n_behind", C.c_longlong), ("n_gated", C.c_longlong),
                ("n_fused", C.c_longlong), ("n_used", C.c_longlong)]


class LandmarkRegisterEval(C.Structure):
    _fields_ = [("H", C.c_double * 36), ("g", C.c_double * 6), ("cost", C.c_double), ("n_used", C.c_longlong),
                ("n_behind", C.c_longlong)]


class LandmarkRegisterRobustResult(C.Structure):
    _fields_ = LandmarkRegisterResult._fields_ + [("n_outlier", C.c_longlong)]


class LandmarkRegisterRobustEval(C.Structure):
    _fields_ = LandmarkRegisterEval._fields_ + [("n_outlier", C.c_longlong)]


class LandmarkRegisterHampelOptions(C.Structure):
    _fields_ = [("base", LandmarkRegisterOptions), ("b", C.c_double), ("c", C.c_double), ("huber_first", C.c_int)]


class LandmarkRegisterHampelResult(C.Structure):
    _fields_ = LandmarkRegisterRobustResult._fields_ + [("n_rejected", C.c_longlong), ("rot_huber", C.c_double * 3),
                                                        ("tran_huber", C.c_double * 3), ("huber_iterations", C.c_int)]


class LandmarkRegisterHampelEval(C.Structure):
    _fields_ = LandmarkRegisterRobustEval._fields_ + [("n_rejected", C.c_longlong)]


ALLREDUCE_FN =C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p)

_dp = C.POINTER(C.c_double)
_vp = C.c_void_p

# name -> (restype, argtypes); must list every function include/sba_hip.h declares
SIGNATURES = {
    "sba_abi_version": (C.c_int, []),
    "sba_last_error": (C.c_char_p, []),
    "sba_device_count": (C.c_int, [C.POINTER(C.c_int)]),
    "sba_lm_options_default": (None, [C.POINTER(LmOptions)]),
    "sba_problem_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    "sba_problem_destroy": (C.c_int, [_vp]),
    "sba_problem_upload": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int]),
    "sba_problem_upload_keypoints": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _vp, C.c_int]),
    "sba_problem_upload_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int]),
    "sba_problem_size": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "sba_problem_set_kernel": (C.c_int, [_vp, C.c_int]),
    "sba_problem_set_folding": (C.c_int, [_vp, C.c_int]),
    "sba_problem_set_depths": (C.c_int, [_vp, _vp]),
    "sba_problem_residuals": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_double, _dp, _dp, _vp,
                                        C.POINTER(C.c_size_t)]),
    "sba_problem_compact": (C.c_int, [_vp, _vp, C.POINTER(C.c_size_t), _vp]),
    "sba_problem_residual_order_stats": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_double, C.c_double, C.POINTER(C.c_size_t),
                                                   C.c_int, _dp]),
    "sba_problem_keep_below": (C.c_int, [_vp, C.c_int, _dp, _dp, C.c_double, C.c_double, C.c_size_t, C.c_double, _dp,
                                         C.POINTER(C.c_size_t), _vp]),
    "sba_problem_eval": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                   C.c_double, C.POINTER(NormalEq)]),
    "sba_problem_eval_pack": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                        C.c_double, _dp]),
    "sba_problem_eval_timed": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                         C.c_double, C.c_int, _dp, _dp, _dp]),
    "sba_problem_eval_launch_times": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                                C.c_double, C.c_int, C.POINTER(C.c_float)]),
    "sba_problem_eval_steps": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                         C.c_double, C.c_int, _dp, _dp]),
    "sba_expand_pack": (C.c_int, [C.c_int, _dp, C.POINTER(NormalEq)]),
    "sba_problem_solve": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, C.c_double, C.c_double,
                                    C.POINTER(LmOptions), C.POINTER(LmSummary)]),
    "sba_problem_solve_depths": (C.c_int, [_vp, _dp, _dp, C.c_double, C.c_double, C.POINTER(LmOptions), _vp,
                                           C.POINTER(LmSummary)]),
    "sba_problem_eval_joint": (C.c_int, [_vp, _dp, _dp, C.c_double, C.POINTER(LmOptions), C.POINTER(JointEq)]),
    "sba_problem_solve_joint": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.POINTER(LmSummary), _vp]),
    "sba_problem_covariance_joint": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(JointCov), _dp]),
    "sba_problem_structure_joint": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(JointCov), _dp, _dp,
                                              _dp]),
    "sba_problem_structure_joint_device": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(JointCov), _vp,
                                                     _vp, _vp]),
    "sba_problem_structure_order_stats": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(C.c_size_t),
                                                    C.c_int, _dp]),
    "sba_problem_structure_keep_below": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.c_size_t, C.c_double,
                                                   _dp, C.POINTER(C.c_size_t), _vp]),
    "sba_problem_eval_resection": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.POINTER(ResectionEq)]),
    "sba_problem_solve_resection": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.POINTER(LmSummary), _dp, C.c_int]),
    "sba_problem_resection_depths": (C.c_int, [_vp, _dp, _dp, _dp]),
    "sba_problem_resection_guess": (C.c_int, [_vp, _dp, _dp, C.POINTER(ResectionGuessInfo), _dp]),
    "sba_problem_score_resection": (C.c_int, [_vp, _dp, _dp, C.c_int, C.c_double, C.POINTER(C.c_longlong)]),
    "sba_problem_resection_guess_consensus": (C.c_int, [_vp, C.POINTER(ResectionConsensusOptions), _dp, _dp,
                                                        C.POINTER(ResectionConsensusInfo), C.POINTER(C.c_longlong), _dp, _dp]),
    "sba_problem_resection_set_landmark_cov": (C.c_int, [_vp, _dp, C.c_double]),
    "sba_problem_resection_set_landmark_cov_device": (C.c_int, [_vp, C.c_void_p, C.c_double]),
    "sba_problem_resection_freeze_weights": (C.c_int, [_vp, _dp, _dp, C.c_double, C.POINTER(C.c_longlong)]),
    "sba_problem_resection_weights": (C.c_int, [_vp, _dp]),
    "sba_problem_eval_resection_weighted": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.POINTER(ResectionEq)]),
    "sba_problem_solve_resection_weighted": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.c_int,
                                                       C.POINTER(LmSummary), _dp, C.c_int]),
    "sba_problem_resection_covariance": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.POINTER(ResectionCov)]),
    "sba_landmarks_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    "sba_landmarks_destroy": (C.c_int, [_vp]),
    "sba_landmarks_size": (C.c_int, [_vp, C.POINTER(C.c_size_t)]),
    "sba_landmarks_set": (C.c_int, [_vp, _dp, _dp, C.c_size_t, C.c_double]),
    "sba_landmarks_set_device": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_double]),
    "sba_landmarks_get": (C.c_int, [_vp, _dp, _dp]),
    "sba_landmarks_get_device": (C.c_int, [_vp, _vp, _vp]),
    "sba_landmarks_counts": (C.c_int, [_vp, C.POINTER(C.c_uint32)]),
    "sba_landmarks_fuse": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp, C.POINTER(LandmarkFuseOptions),
                                     C.POINTER(LandmarkFuseResult), _dp]),
    "sba_landmarks_scores": (C.c_int, [_vp, _dp]),
    "sba_landmarks_prune": (C.c_int, [_vp, C.POINTER(LandmarkPruneOptions), C.POINTER(LandmarkPruneResult), C.POINTER(C.c_int64)]),
    "sba_landmarks_append": (C.c_int, [_vp, _dp, _dp, C.c_size_t, C.c_double]),
    "sba_landmarks_append_device": (C.c_int, [_vp, _vp, _vp, C.c_size_t, C.c_double]),
    "sba_landmarks_gather": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_size_t, _dp, _dp, C.POINTER(C.c_uint32)]),
    "sba_landmarks_gather_device": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_size_t, _vp, _vp]),
    "sba_landmarks_eval_register": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp, _dp, _dp,
                                              C.POINTER(LandmarkRegisterOptions), C.POINTER(LandmarkRegisterEval)]),
    "sba_landmarks_register": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp, C.POINTER(LandmarkRegisterOptions),
                                         C.POINTER(LandmarkRegisterResult), _dp]),
    "sba_landmarks_eval_register_robust": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp, _dp, _dp,
                                                     C.POINTER(LandmarkRegisterOptions), C.POINTER(LandmarkRegisterRobustEval)]),
    "sba_landmarks_register_robust": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp, C.POINTER(LandmarkRegisterOptions),
                                                C.POINTER(LandmarkRegisterRobustResult), _dp]),
    "sba_landmarks_eval_register_robust_device": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, C.c_size_t, _dp, _dp, _dp, _dp,
                                                            C.POINTER(LandmarkRegisterOptions), C.POINTER(LandmarkRegisterRobustEval)]),
    "sba_landmarks_register_robust_device": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, C.c_size_t, _dp, _dp,
                                                       C.POINTER(LandmarkRegisterOptions), C.POINTER(LandmarkRegisterRobustResult), _vp]),
    "sba_landmarks_eval_register_hampel": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp, _dp, _dp,
                                                     C.POINTER(LandmarkRegisterHampelOptions), C.POINTER(LandmarkRegisterHampelEval)]),
    "sba_landmarks_register_hampel": (C.c_int, [_vp, C.POINTER(C.c_int64), _dp, C.c_size_t, _dp, _dp,
                                                C.POINTER(LandmarkRegisterHampelOptions), C.POINTER(LandmarkRegisterHampelResult), _dp]),
    "sba_landmarks_eval_register_hampel_device": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, C.c_size_t, _dp, _dp, _dp, _dp,
                                                            C.POINTER(LandmarkRegisterHampelOptions), C.POINTER(LandmarkRegisterHampelEval)]),
    "sba_landmarks_register_hampel_device": (C.c_int, [_vp, C.POINTER(C.c_int64), _vp, C.c_size_t, _dp, _dp,
                                                       C.POINTER(LandmarkRegisterHampelOptions), C.POINTER(LandmarkRegisterHampelResult), _vp]),
    "sba_landmarks_set_descriptors": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t]),
    "sba_landmarks_set_descriptors_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t]),
    "sba_landmarks_descriptor_dim": (C.c_int, [_vp, C.POINTER(C.c_int)]),
    "sba_landmarks_get_descriptors": (C.c_int, [_vp, C.POINTER(C.c_int64), C.c_size_t, _vp, C.c_size_t]),
    "sba_landmarks_append_described": (C.c_int, [_vp, _dp, _dp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_double]),
    "sba_landmarks_append_described_device": (C.c_int, [_vp, _vp, _vp, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_double]),
    "sba_landmarks_associate": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t, _dp, C.POINTER(LandmarkAssociateOptions),
                                          C.POINTER(LandmarkAssociateResult), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_float), _dp]),
    "sba_landmarks_associate_device": (C.c_int, [_vp, _vp, C.c_size_t, C.c_int, C.c_size_t, _vp, C.POINTER(LandmarkAssociateOptions),
                                                 C.POINTER(LandmarkAssociateResult), C.POINTER(C.c_int64), C.POINTER(C.c_int32),
                                                 C.POINTER(C.c_float), _vp]),
    "sba_problem_epipolar_moments": (C.c_int, [_vp, _dp]),
    "sba_initial_guess_from_moments": (C.c_int, [_dp, C.c_int, C.c_double, C.c_ulonglong, _dp, _dp,
                                                 C.POINTER(C.c_int)]),
    "sba_problem_initial_guess": (C.c_int, [_vp, C.c_int, C.c_double, C.c_ulonglong, _dp, _dp, C.POINTER(C.c_int)]),
    "sba_reference_rand_seed": (C.c_int, [C.c_uint]),
    "sba_reference_rand_next": (C.c_int, []),
    "sba_reference_trial_subsets": (C.c_int, [C.c_int, C.c_int, C.c_double, _vp, C.POINTER(C.c_int)]),
    "sba_problem_epipolar_subset_moments": (C.c_int, [_vp, _vp, C.c_int, C.c_int, _dp]),
    "sba_problem_initial_guess_reference": (C.c_int, [_vp, C.c_int, C.c_double, _dp, _dp, C.POINTER(C.c_int)]),
    "sba_comm_unique_id": (C.c_int, [C.c_char_p]),
    "sba_problem_comm_init_rank": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "sba_rccl_available": (C.c_int, []),
    "sba_problem_comm_destroy": (C.c_int, [_vp]),
    "sba_problem_peer_export": (C.c_int, [_vp, C.c_int, C.c_int, C.c_char_p]),
    "sba_problem_peer_connect": (C.c_int, [_vp, C.c_char_p]),
    "sba_problem_peer_selftest": (C.c_int, [_vp, C.c_int, C.POINTER(C.c_int)]),
    "sba_problem_peer_disable": (C.c_int, [_vp]),
    "sba_set_host_threads": (C.c_int, [C.c_int]),
    "sba_problem_set_shard": (C.c_int, [_vp, C.c_int, C.c_int]),
    "sba_problem_set_allreduce": (C.c_int, [_vp, ALLREDUCE_FN, _vp]),
    "sba_problem_pack_device_ptr": (C.c_int, [_vp, C.POINTER(_vp)]),
    "sba_batch_create": (C.c_int, [C.POINTER(_vp), C.c_int, _vp]),
    "sba_batch_destroy": (C.c_int, [_vp]),
    "sba_batch_set_kernel": (C.c_int, [_vp, C.c_int]),
    "sba_batch_upload": (C.c_int, [_vp, _vp, _vp, _vp, C.POINTER(C.c_size_t), C.c_int, C.c_int]),
    "sba_batch_size": (C.c_int, [_vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sba_batch_eval": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, _dp]),
    "sba_batch_eval_timed": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_int, _dp,
                                       _dp, _dp, _dp, _dp]),
    "sba_batch_sweep_launch_times": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_int,
                                               C.POINTER(C.c_float)]),
    "sba_batch_step_launch_times": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.c_int,
                                              C.POINTER(C.c_float)]),
    "sba_batch_step_is_fused": (C.c_int, [_vp]),
    "sba_batch_solve": (C.c_int, [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(LmOptions),
                                  C.POINTER(LmSummary), C.POINTER(C.c_int)]),
    "sba_batch_solve_depths": (C.c_int, [_vp, _dp, _dp, C.c_double, C.c_double, C.POINTER(LmOptions), _vp,
                                         C.POINTER(LmSummary), C.POINTER(C.c_int)]),
    "sba_batch_eval_joint": (C.c_int, [_vp, _dp, _dp, C.c_double, C.POINTER(LmOptions), C.POINTER(JointEq)]),
    "sba_batch_solve_joint": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.POINTER(LmSummary), C.POINTER(C.c_int), _vp]),
    "sba_batch_covariance_joint": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(JointCov), _dp,
                                             C.POINTER(C.c_int)]),
    "sba_batch_structure_joint": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(JointCov), _dp, _dp, _dp,
                                            C.POINTER(C.c_int)]),
    "sba_batch_structure_joint_device": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(JointCov), _vp, _vp,
                                                   _vp, C.POINTER(C.c_int)]),
    "sba_batch_structure_order_stats": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(C.c_size_t), C.c_int,
                                                  _dp, C.POINTER(C.c_int)]),
    "sba_batch_structure_keep_below": (C.c_int, [_vp, _dp, _dp, C.POINTER(LmOptions), C.c_double, C.POINTER(C.c_size_t), _dp, _dp,
                                                 C.POINTER(C.c_size_t), _vp, C.POINTER(C.c_int)]),
    "sba_batch_residuals": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, C.c_double, _dp, _dp, _vp, C.POINTER(C.c_size_t)]),
    "sba_batch_compact": (C.c_int, [_vp, _vp, C.POINTER(C.c_size_t), _vp]),
    "sba_batch_keep_inliers": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, C.c_double, C.POINTER(C.c_size_t), _vp]),
    "sba_batch_residual_order_stats": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_size_t), C.c_int, _dp]),
    "sba_batch_keep_below": (C.c_int, [_vp, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(C.c_size_t), _dp, _dp, C.POINTER(C.c_size_t),
                                       _vp]),
    "sba_batch_solve_problem": (C.c_int, [_vp, C.c_int, C.c_int, C.c_double, C.c_ulonglong, _dp, _dp, C.POINTER(LmOptions), _vp, _dp,
                                          C.POINTER(C.c_int), C.POINTER(LmSummary), C.POINTER(LmSummary), C.POINTER(LmSummary),
                                          C.POINTER(C.c_int)]),
    "sba_batch_set_depths": (C.c_int, [_vp, _dp]),
    "sba_batch_epipolar_moments": (C.c_int, [_vp, _dp]),
    "sba_batch_initial_guess": (C.c_int, [_vp, C.c_int, C.c_double, C.c_ulonglong, _dp, _dp, C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    "sba_keypoints_to_sphere": (C.c_int, [C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _vp]),
    "sba_rotate_keypoints": (C.c_int, [C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_int]),
    "sba_cube2equi_keypoints": (C.c_int, [C.c_int, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "sba_crop_rotated_image": (C.c_int, [C.c_int, _vp, C.c_int, C.c_int, C.c_float, _vp]),
    "sba_rotate_keypoints_device": (C.c_int, [C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, C.c_float, C.c_int, C.c_int]),
    "sba_cube2equi_keypoints_device": (C.c_int, [C.c_int, _vp, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, C.c_int]),
    "sba_crop_rotated_image_device": (C.c_int, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_float, C.c_int, _vp]),
    "sba_map_table_host_decided": (C.c_long, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int]),
    "sba_map_table_tiles": (C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int),
                                      C.POINTER(C.c_int)]),
    "sba_equi2cube": (C.c_int, [C.c_int, _vp, C.c_int, C.c_int, C.c_int, _vp]),
    "sba_equi2cube_device": (C.c_int, [C.c_int, _vp, _vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp]),
    "sba_match_descriptors": (C.c_int, [C.c_int, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_float, _vp, _vp,
                                        C.POINTER(C.c_size_t), _vp, _vp, _vp]),
    "sba_match_descriptors_device": (C.c_int, [C.c_int, _vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_int, C.c_size_t, C.c_float,
                                               _vp, _vp, C.POINTER(C.c_size_t), _vp, _vp, _vp]),
    "sba_batch_match_descriptors": (C.c_int, [C.c_int, _vp, _vp, _vp, _vp, C.c_int, C.c_int, C.c_size_t, C.c_float, _vp, _vp,
                                              _vp, _vp, _vp, _vp]),
    "sba_problem_upload_matches": (C.c_int, [_vp, _vp, C.c_size_t, _vp, C.c_size_t, C.c_size_t, C.c_int, C.c_int, _vp, _vp,
                                             C.c_int, C.c_size_t, C.c_float, _dp, C.c_int, C.POINTER(C.c_size_t), _vp, _vp]),
    "sba_batch_upload_matches": (C.c_int, [_vp, _vp, _vp, _vp, _vp, C.c_int, C.c_size_t, C.c_int, C.c_int, _vp, _vp, C.c_int,
                                           C.c_size_t, C.c_float, _dp, C.c_int, _vp, _vp, _vp]),
}

_lib = None


def load_library(path: os.PathLike | None = None) -> C.CDLL:
    """Load libsba_hip.so (once).  Raises LibraryNotBuilt when it has not been compiled."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    # SBA_LIBRARY_PATH: a differently built libsba_hip.so (tools' A/B measurements of build variants only)
    p = Path(path) if path else Path(os.environ.get("SBA_LIBRARY_PATH", LIB_PATH))
    if not p.exists():
        raise LibraryNotBuilt(
            f"{p} not found: build it with `make -C {PKG_DIR / 'csrc'}` or "
            "`python -c 'import __graft_entry__ as g; g.build()'`. "
            "There is no Python/CPU fallback for the HIP hot path.")
    # One HIP runtime per process: torch bundles libamdhip64.so.7; if torch is going to be used in
    # this process, let it load its copy first so this library binds to the same one.
    try:
        import torch  # noqa: F401
    except Exception:
        pass
    lib = C.CDLL(str(p))
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)   # AttributeError here = header and library out of sync
        fn.restype = res
        fn.argtypes = args
    if lib.sba_abi_version() != ABI_VERSION:
        raise LibraryNotBuilt(f"{p}: ABI version {lib.sba_abi_version()} != {ABI_VERSION}, rebuild")
    if path is None:
        _lib = lib
    return lib


def last_error(lib: C.CDLL) -> str:
    msg = lib.sba_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(lib: C.CDLL, rc: int) -> None:
    if rc != SBA_OK:
        msg = lib.sba_last_error()
        raise SbaError(rc, msg.decode("utf-8", "replace") if msg else "")
