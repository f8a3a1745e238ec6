/*
 * sba_hip.h -- C-ABI drop-in boundary of the MI355X spherical bundle-adjustment hot path.
 *
 * What this replaces in the reference (whdlgp/spherical_bundle_adjuster, all citations
 * relative to the reference tree):
 *
 *   - the four `add_residual` loops that build one Ceres residual block per match
 *     (spherical_bundle_adjuster.cpp:870-889, :921-945, :978-1002, :1034-1063)
 *       -> sba_problem_upload()            (one flat upload instead of 3 heap objects per match)
 *   - one residual+Jacobian sweep of ceres::Solve over those blocks, i.e. the templated
 *     functors (spherical_bundle_adjuster.cpp:843-868, :891-919, :947-976) pushed through
 *     AutoDiffCostFunction + HuberLoss(1.0) and accumulated into J^T J / J^T r
 *       -> sba_problem_eval() / sba_problem_eval_pack()
 *   - `ceres::Solve(opt, &problem_rot|tran, &summary)` inside solve_problem()
 *     (spherical_bundle_adjuster.cpp:183-217, options :334-338)
 *       -> sba_problem_solve()             (Levenberg-Marquardt on the host, normal equations from the GPU)
 *   - the d-only stage (spherical_bundle_adjuster.cpp:1004-1063)
 *       -> sba_problem_solve_depths()
 *   - the joint functor over depths, rotation and translation (spherical_bundle_adjuster.cpp:843-889)
 *       -> sba_problem_solve_joint(), sba_problem_eval_joint()
 *   - (no counterpart in the reference) a further frame registered against the landmarks of a solved pair
 *       -> sba_problem_solve_resection(), sba_problem_resection_guess()
 *          weighted by the landmarks' covariances, with the covariance of the resected pose:
 *          sba_problem_solve_resection_weighted(), sba_problem_resection_covariance()
 *   - (no counterpart in the reference) the landmarks kept across frames and improved by each registered frame's bearings
 *       -> sba_landmarks_*()               (a handle of its own; sba_landmarks_fuse: one Kalman update per landmark;
 *                                           sba_landmarks_scores / _prune / _append / _gather: the map edited on the device;
 *                                           sba_landmarks_register: a frame's pose and its landmarks solved jointly;
 *                                           sba_landmarks_set_descriptors / _associate: a descriptor row per landmark and a
 *                                           frame's idx and bearings from its descriptors)
 *   - pixel -> unit sphere (spherical_bundle_adjuster.cpp:271-298)
 *       -> sba_keypoints_to_sphere()
 *   - equi2cube::get_all (equi2cube.cpp:12-302)
 *       -> sba_equi2cube(), sba_equi2cube_device()
 *   - initial_guess / eight_point_estimation (spherical_bundle_adjuster.cpp:47-181)
 *       -> sba_problem_initial_guess()
 *   - spherical_surf::rotate_keypoint / crop_rotated_image, equi2cube_surf::cube2equi_pixel
 *       -> sba_rotate_keypoints(), sba_crop_rotated_image(), sba_cube2equi_keypoints()
 *   - one run of main/main.cpp per image pair
 *       -> sba_batch_*()                   (many pairs per launch, one LM per pair)
 *   - feature_matcher::match_two_image (feature_matcher.cpp:42-59: FLANN 2-NN + ratio test)
 *       -> sba_match_descriptors(), sba_batch_match_descriptors(), sba_*_upload_matches()
 *
 * Conventions
 *   - every function returns an int status: 0 = SBA_OK, negative = error; the text of the
 *     last error on the calling thread is returned by sba_last_error().
 *   - no exceptions cross this boundary, no C++ or torch types appear in a signature.
 *   - the caller owns every host array it passes in; the library owns the device buffers
 *     inside the opaque handles.  Handles are not thread-safe.
 *   - residual convention (spherical_bundle_adjuster.cpp:897-916):
 *         e_i = d2 * x2_i - ( R(rot) * (d1 * x1_i) - tran )
 *     with R(rot) the angle-axis rotation (Ceres AngleAxisRotatePoint semantics, including
 *     its small-angle branch), robustified per 3-vector block by Huber(delta).
 *   - there is NO CPU fallback: without a usable HIP device every compute entry point fails
 *     with SBA_ERR_NO_DEVICE.
 */
#ifndef SBA_HIP_H_
#define SBA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SBA_ABI_VERSION 2

/* ---- status codes ------------------------------------------------------------------ */
enum {
  SBA_OK = 0,
  SBA_ERR_INVALID_ARG = -1,
  SBA_ERR_NO_DEVICE = -2,   /* no HIP device / HIP runtime unusable                     */
  SBA_ERR_HIP = -3,         /* a HIP call failed (text in sba_last_error)               */
  SBA_ERR_NOT_UPLOADED = -4,
  SBA_ERR_COMM = -5,        /* RCCL / user all-reduce hook failed                        */
  SBA_ERR_NUMERIC = -6,     /* non-finite normal equations, singular system             */
  SBA_ERR_UNSUPPORTED = -7
};

/* ---- which parameter block is free (= which reference functor is evaluated) ---------- */
enum {
  SBA_MODE_ROT = 0,  /* ba_spherical_costfunctor_rot_only  (.cpp:891-919): rot free, tran frozen */
  SBA_MODE_TRAN = 1, /* ba_spherical_costfunctor_tran_only (.cpp:947-976): tran free, rot frozen */
  SBA_MODE_RT = 2    /* ba_spherical_costfunctor (.cpp:843-868) with d held fixed: rot+tran free
                        (d free as well: sba_problem_solve_joint) */
};

/* ---- where d1,d2 come from ----------------------------------------------------------- */
enum {
  SBA_DEPTH_UNIFORM = 0,  /* two scalars for every match: what the reference actually does,
                             init_d[0][0] / init_d[1][0] (.cpp:941-942, :998-999)          */
  SBA_DEPTH_PER_MATCH = 1 /* d12[i][0], d12[i][1] per match (.cpp:887, the joint functor)  */
};

/* ---- storage type of the device-resident unit vectors -------------------------------- */
enum {
  SBA_STORE_F64 = 0, /* 48 B / correspondence (64 B with per-match depths): reference-faithful */
  SBA_STORE_F32 = 1  /* 24 B / correspondence (32 B): arithmetic stays f64                    */
};

/* ---- which sweep kernel evaluates the Jacobian terms (results agree to rounding) ---------------- */
enum {
  SBA_KERNEL_FACTORED = 0, /* default: d e/d rot = -[v]x J_l(rot), v = -d1 R x1; the device accumulates the
                              moments sum w v v^T, sum w v e^T, sum w v and the host applies J_l          */
  SBA_KERNEL_EXPLICIT = 1  /* the 3x3 Jacobian block d e/d rot is formed per match on the device          */
};

/* ---- translation parameterisation in SBA_MODE_RT / SBA_MODE_TRAN ---------------------- */
enum {
  SBA_TRAN_FREE = 0,   /* 3 free components, additive update (reference behaviour)            */
  SBA_TRAN_SPHERE = 1  /* 5-DoF: tran stays on the sphere |tran| = const, 2-dim tangent update */
};

/* Indices into the 24-double device pack (the thing that is all-reduced across GPUs).     */
enum {
  SBA_PACK_HAA = 0,   /* [0..5]  upper triangle of sum w A^T A : 00 01 02 11 12 22          */
  SBA_PACK_HAT = 6,   /* [6..14] sum w A^T  (3x3 row-major: row = rot index, col = tran idx) */
  SBA_PACK_SW = 15,   /* sum w            (H_tt = SW * I3)                                  */
  SBA_PACK_GA = 16,   /* [16..18] sum w A^T e                                               */
  SBA_PACK_GT = 19,   /* [19..21] sum w e                                                   */
  SBA_PACK_COST = 22, /* 1/2 sum rho(|e|^2)                                                 */
  SBA_PACK_NOUT = 23, /* number of blocks in Huber's outlier region (as a double)           */
  SBA_PACK_SIZE = 24
};

/* Expanded normal equations over the parameter order [rot0 rot1 rot2 tran0 tran1 tran2].  */
typedef struct sba_normal_eq {
  double H[36];      /* row-major symmetric 6x6 = sum rho' J^T J; unused blocks are zero     */
  double g[6];       /* sum rho' J^T e                                                       */
  double cost;       /* 1/2 sum rho(|e|^2)   (what Ceres reports as the cost)                */
  double sum_w;      /* sum rho'                                                             */
  double n_outlier;  /* blocks with |e|^2 > delta^2                                          */
} sba_normal_eq;

/* Levenberg-Marquardt options; defaults (sba_lm_options_default) restate the Ceres defaults
 * that govern the reference's solve (spherical_bundle_adjuster.cpp:334-338 sets only
 * max_num_iterations = 50, the linear solver, stdout logging and the thread count).       */
typedef struct sba_lm_options {
  int max_num_iterations;             /* 50  (.cpp:336)                                     */
  double initial_trust_region_radius; /* 1e4                                               */
  double max_trust_region_radius;     /* 1e16                                              */
  double min_trust_region_radius;     /* 1e-32                                             */
  double min_relative_decrease;       /* 1e-3                                              */
  double min_lm_diagonal;             /* 1e-6                                              */
  double max_lm_diagonal;             /* 1e32                                              */
  double function_tolerance;          /* 1e-6                                              */
  double gradient_tolerance;          /* 1e-10                                             */
  double parameter_tolerance;         /* 1e-8                                              */
  int jacobi_scaling;                 /* 1                                                 */
  double huber_delta;                 /* 1.0 (.cpp:887,:943,:1000); <= 0 disables the loss */
  int tran_param;                     /* SBA_TRAN_FREE (reference) or SBA_TRAN_SPHERE       */
  int verbose;                        /* 1 = per-iteration line on stdout (.cpp:337)        */
  /* Projected line search of a bounds-constrained problem -- only the d-only stage has bounds
   * (.cpp:1060-1061).  Ceres runs it on every trust-region step when the count below is > 0; the
   * reference leaves all five at Ceres' defaults.  ARMIJO, CUBIC interpolation.  0 = off.        */
  int max_num_line_search_step_size_iterations;    /* 20                                     */
  double line_search_sufficient_function_decrease; /* 1e-4                                   */
  double max_line_search_step_contraction;         /* 1e-3                                   */
  double min_line_search_step_contraction;         /* 0.6                                    */
  double min_line_search_step_size;                /* 1e-9                                   */
} sba_lm_options;

enum {
  SBA_TERM_CONVERGENCE_FUNCTION = 1,
  SBA_TERM_CONVERGENCE_GRADIENT = 2,
  SBA_TERM_CONVERGENCE_PARAMETER = 3,
  SBA_TERM_NO_CONVERGENCE = 4,     /* iteration limit                                       */
  SBA_TERM_MIN_RADIUS = 5,
  SBA_TERM_FAILURE = 6
};

typedef struct sba_lm_summary {
  int termination;            /* SBA_TERM_*                                                */
  int num_iterations;         /* LM iterations run (successful + unsuccessful)             */
  int num_successful_steps;
  int num_evaluations;        /* residual+Jacobian sweeps over the correspondences         */
  double initial_cost;
  double final_cost;
  double final_gradient_max_norm;
  double final_radius;
  double seconds_total;       /* wall clock of the whole solve                             */
  double seconds_eval;        /* of which: waiting for the device sweeps                   */
  int num_line_search_steps;  /* d-only stage: step-size contractions of the projected line search */
} sba_lm_summary;

typedef struct sba_problem sba_problem; /* opaque: one shard of correspondences on one GPU  */

/* User all-reduce hook (sum, in place) over `count` doubles at device address `device_buf`,
 * to be enqueued on HIP stream `stream`.  Lets a host that already owns a communicator
 * (e.g. torch.distributed) supply the exchange; see also sba_problem_comm_init_rank.        */
typedef int (*sba_allreduce_fn)(void* device_buf, size_t count, void* stream, void* user);

/* ---- library ------------------------------------------------------------------------- */
int sba_abi_version(void);
const char* sba_last_error(void);
int sba_device_count(int* count);
void sba_lm_options_default(sba_lm_options* opt);

/* ---- problem life cycle ---------------------------------------------------------------- */
/* device: HIP ordinal.  stream: an existing hipStream_t to launch on, or NULL to let the
 * problem create its own non-blocking stream.                                              */
int sba_problem_create(sba_problem** out, int device, void* stream);
int sba_problem_destroy(sba_problem* p);

/* Upload n correspondences.  left_xyz / right_xyz: packed double[3n], exactly
 * `std::vector<cv::Point3d>::data()` of key_point_left_rect / key_point_right_rect
 * (spherical_bundle_adjuster.cpp:286-298).  d12: NULL, or double[2n] =
 * `std::vector<std::array<double,2>>::data()` (init_d, .cpp:311-327) for per-match depths.
 * The arrays are copied (and re-laid-out as planes) once; they are not referenced afterwards.
 * n == 0 is legal (every eval then returns zeros).                                          */
int sba_problem_upload(sba_problem* p, const double* left_xyz, const double* right_xyz,
                       const double* d12, size_t n, int store);

/* Same, from arrays already resident on this problem's device (same AoS layouts).          */
int sba_problem_upload_device(sba_problem* p, const void* left_xyz_dev, const void* right_xyz_dev,
                              const void* d12_dev, size_t n, int store);

/* Same, straight from the matcher's output: `left_keypoints[i]` / `right_keypoints[i]` are the MATCHED
 * key-point records (cv::KeyPoint layout: the first two float32 of each record are pt.x, pt.y;
 * stride_bytes = sizeof(cv::KeyPoint) = 28) of the two equirectangular images.  The pixel -> unit-sphere
 * map of spherical_bundle_adjuster.cpp:271-298 runs on the device and writes the coordinate planes
 * directly, so the host never materialises the cv::Point3d arrays.       */
int sba_problem_upload_keypoints(sba_problem* p, const void* left_keypoints, const void* right_keypoints, size_t n,
                                 size_t stride_bytes, int im_width, int im_height, const double* d12, int store);

int sba_problem_size(const sba_problem* p, size_t* n);
/* (Re)upload only the per-match depths d12 (double[2n], init_d layout) of the resident correspondences.    */
int sba_problem_set_depths(sba_problem* p, const double* d12);
/* Select the sweep kernel (SBA_KERNEL_*); also settable with the environment variable
 * SBA_KERNEL=explicit at sba_problem_create time.                                                 */
int sba_problem_set_kernel(sba_problem* p, int kind);
/* on = 1 (default): sweeps with per-match depths over f64 planes stream X1 = d1 x1 and X2 = d2 x2, kept in six extra
 * planes of the handle (48 B per match instead of 64; formed at upload / set_depths, re-formed before the next such sweep
 * after the d-only stage).  on = 0: they stream the raw planes and the extra planes are released.  The results are the
 * same bits either way; only speed and device memory differ.                                                           */
int sba_problem_set_folding(sba_problem* p, int on);

/* ---- single matches: residuals, inlier set, compaction ---- */
/* e[i] = d2 x2 - d1 R(rot) x1 + tran, formed exactly as the sweep forms it (uniform depths d1, d2, or the per-match depths
 * with depth_mode = SBA_DEPTH_PER_MATCH), for every uploaded match.  Every output may be NULL:
 *   e_xyz   double[n][3]     the residual
 *   sq_norm double[n]        s = e.e, the argument of the Huber loss
 *   inlier  uint8[n]         !(s > huber_delta^2): 1 = inside Huber's quadratic region; all 1 when huber_delta <= 0
 *   n_inlier                 the number of inliers; n - n_inlier equals SBA_PACK_NOUT of a sweep at the same arguments
 * A match whose residual is NaN counts as an inlier here, as it does in the sweep's outlier count.  The residual does not
 * depend on the sweep mode.  A sharded handle answers for its own matches.                                             */
int sba_problem_residuals(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1, double d2,
                          double huber_delta, double* e_xyz, double* sq_norm, unsigned char* inlier, size_t* n_inlier);
/* Keep the matches with keep[i] != 0 (host array of the handle's size n), in their original order.  Afterwards the handle
 * is what a fresh upload of the kept matches (coordinates and, if present, depths) with the same store would be: same size,
 * same plane contents and padding, so every later sweep, solve, d-only stage, moment pass and initial guess gives the same
 * bits as on such a handle; sba_problem_set_depths then takes *n_kept rows.  kept_index (may be NULL; capacity n) receives
 * the *n_kept original indices in order.  Compacted on the device, deterministic; the count is the one synchronous step.
 * A sharded handle compacts only its own matches: every rank of a collective may keep a different subset and the packs
 * still sum over the union.  On an error the handle may be left without correspondences (SBA_ERR_NOT_UPLOADED after).  */
int sba_problem_compact(sba_problem* p, const unsigned char* keep, size_t* n_kept, long long* kept_index);

/* ---- order statistics of the squared residual norms, and an inlier cut taken from them ---- */
/* values[j] = the ranks[j]-th smallest (0-based: rank 0 is the minimum, n - 1 the maximum) of s_i = e_i.e_i, the sq_norm of
 * sba_problem_residuals at the same arguments, selected on the device: the s plane is written by the same kernel, so every
 * value is, bit for bit, an element of that array, and no interpolation happens.  1 <= num_ranks <= 8, every ranks[j] < n,
 * n > 0.  Order is that of the bit patterns read as unsigned 64-bit integers: numeric for s >= +0, and every NaN (either
 * sign) sorts above +inf.  Exact radix select with integer counts: the same bits on every run and for every grid size.
 * Replaces sba_problem_residuals(sq_norm) + a partition of the n doubles on the host.  A handle that is sharded, hooked or
 * connected to peers is refused with SBA_ERR_UNSUPPORTED (the shards' histograms are not summed).                        */
int sba_problem_residual_order_stats(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1,
                                     double d2, const size_t* ranks, int num_ranks, double* values);
/* *threshold = scale * s_(rank) (one IEEE f64 multiplication; scale finite and >= 0), then the matches with
 * s_i <= *threshold stay, through the compaction of sba_problem_compact: afterwards the handle is what a fresh upload of the
 * kept matches with the same store would be, *n_kept is their number and kept_index (may be NULL; capacity n) receives their
 * original indices in order.  A match whose s is NaN is dropped -- unlike `inlier` of sba_problem_residuals, where a NaN
 * counts as inside.  The flags stay on the device.  Replaces sba_problem_residuals(sq_norm) + a host partition +
 * sba_problem_compact with a host-built mask.  Arguments and refusals as for sba_problem_residual_order_stats.           */
int sba_problem_keep_below(sba_problem* p, int depth_mode, const double rot[3], const double tran[3], double d1, double d2,
                           size_t rank, double scale, double* threshold, size_t* n_kept, long long* kept_index);

/* ---- one residual + Jacobian sweep ------------------------------------------------------ */
/* Evaluates all local correspondences at (rot, tran), reduces on the device, all-reduces if a
 * communicator/hook is installed, and returns the expanded normal equations.  depth_mode
 * SBA_DEPTH_UNIFORM uses (d1, d2) for every match; SBA_DEPTH_PER_MATCH uses the uploaded d12
 * (d1, d2 ignored).  huber_delta <= 0 means no robustifier.  Synchronous.                  */
int sba_problem_eval(sba_problem* p, int mode, int depth_mode, const double rot[3],
                     const double tran[3], double d1, double d2, double huber_delta,
                     sba_normal_eq* out);

/* As above but returns the raw 24-double pack (SBA_PACK_* layout).                         */
int sba_problem_eval_pack(sba_problem* p, int mode, int depth_mode, const double rot[3],
                          const double tran[3], double d1, double d2, double huber_delta,
                          double pack[SBA_PACK_SIZE]);

/* Enqueue `repeat` back-to-back sweeps without host synchronisation in between and time them with
 * HIP events recorded on the problem's stream: *mean_step_ms = (sweep + finalize [+ all-reduce] +
 * publication) per repeat; *mean_sweep_ms = the sweep kernel alone, `repeat` launches back to back under
 * one event pair (kernel + the boundary between dependent launches).  Either output pointer may be NULL.
 * The last sweep's pack is returned.  This is bench.py's timing primitive.                          */
int sba_problem_eval_timed(sba_problem* p, int mode, int depth_mode, const double rot[3],
                           const double tran[3], double d1, double d2, double huber_delta,
                           int repeat, double pack[SBA_PACK_SIZE], double* mean_step_ms,
                           double* mean_sweep_ms);

/* The sweep kernel launched `repeat` times back to back with a HIP event recorded between every two launches on the
 * problem's stream: launch_ms[i] = device time from the event before launch i to the event after it (the kernel plus
 * one event boundary).  Shows the spread of the dominant kernel -- first launches after idle run at ramping clocks --
 * that the mean of sba_problem_eval_timed hides.  repeat <= 4096.                                            */
int sba_problem_eval_launch_times(sba_problem* p, int mode, int depth_mode, const double rot[3],
                                  const double tran[3], double d1, double d2, double huber_delta,
                                  int repeat, float* launch_ms);

/* `steps` complete, host-synchronous sweeps in a row -- each one exactly what an LM iteration costs (launch,
 * reduction, all-reduce if installed, result on the host before the next launch) -- without a language binding
 * between them.  Returns the last pack and the wall-clock seconds of the loop.                               */
int sba_problem_eval_steps(sba_problem* p, int mode, int depth_mode, const double rot[3],
                           const double tran[3], double d1, double d2, double huber_delta, int steps,
                           double pack[SBA_PACK_SIZE], double* seconds);

/* Host-only: expand a pack into the 6x6 system (no device needed).                         */
int sba_expand_pack(int mode, const double pack[SBA_PACK_SIZE], sba_normal_eq* out);

/* ---- Levenberg-Marquardt solve (replaces ceres::Solve for the rot / tran / joint stage) -- */
/* rot and tran are updated in place like init_rot / init_tran in the reference
 * (spherical_bundle_adjuster.cpp:202-209).                                                  */
int sba_problem_solve(sba_problem* p, int mode, int depth_mode, double rot[3], double tran[3],
                      double d1, double d2, const sba_lm_options* opt, sba_lm_summary* summary);

/* d-only stage (spherical_bundle_adjuster.cpp:1004-1063, `Solve(opt, &problem_d, &summary)` at :197): ONE
 * bounded trust-region problem over all per-match depth pairs (5 residuals per match: the reprojection
 * 3-vector and lambda*exp(-c*d1), lambda*exp(-c*d2); no loss; lower bound 0; the reference uses lambda = c = 1).
 * Needs per-match depths uploaded (they are the initial values, init_d) and updates them on the device, so a
 * following SBA_DEPTH_PER_MATCH sweep sees the refined depths.  d12_out (double[2n], may be NULL) receives
 * them in init_d layout.  opt NULL = defaults (huber_delta / tran_param are ignored).  Every trust-region step
 * goes through Ceres' projected Armijo line search first (the problem is bounds-constrained and the reference
 * leaves max_num_line_search_step_size_iterations at 20): the first trial, step size 1, is evaluated by the same
 * device pass that computes the step; each contraction costs one more pass.  With a transport attached (sharded
 * problem) the nine global reductions of every pass are all-reduced, all ranks take the same steps, and every
 * rank receives its own shard's depths (at most 8 shards, see sba_problem_set_shard).                       */
int sba_problem_solve_depths(sba_problem* p, const double rot[3], const double tran[3], double lambda,
                             double c, const sba_lm_options* opt, double* d12_out, sba_lm_summary* summary);

/* ---- joint solve: depths, rotation and translation free together ------------------------ */
/* The reference's joint functor ba_spherical_costfunctor (spherical_bundle_adjuster.cpp:843-889): one 3-residual
 * Huber block per match over (d_i[2], rot[3], tran[3]),  e_i = d2_i x2_i - d1_i R(rot) x1_i + tran, no bounds and no
 * regulariser (those belong to the d-only functor).  Parameters: the 2n per-match depths of the handle and the camera.
 * The depth blocks are private to a match, so every LM iteration eliminates them per match on the device (a damped 2x2
 * block) and solves the reduced camera system (<= 6 x 6, the Schur complement) on the host: two streaming passes per
 * iteration, trust-region schedule as sba_problem_solve / sba_problem_solve_depths, no line search.
 * Gauge: with SBA_TRAN_FREE the cost is homogeneous of degree 2 in (d, tran) inside Huber's quadratic region, so
 * (d, tran) -> 0 is a minimiser.  The useful form pins |tran| with SBA_TRAN_SPHERE: opt == NULL means the defaults WITH
 * tran_param = SBA_TRAN_SPHERE for the two entry points below; an explicit SBA_TRAN_FREE runs the functor as written.
 * A handle with a shard, communicator, peer set or all-reduce hook, and a problem without per-match depths, is refused
 * with SBA_ERR_UNSUPPORTED; a non-finite start with SBA_ERR_NUMERIC (the handle stays usable, its depths unchanged).
 * Only that failure leaves the depths as they were: a solve that fails later (five invalid steps in a row, a device wait
 * that times out and poisons the handle) leaves the last accepted depths, or an unfinished candidate, in the handle.       */
typedef struct sba_joint_eq {     /* parameter order [rot0..2 tran0..2], unscaled, undamped camera side */
  double S[36], gs[6];            /* reduced camera system / gradient at the given depth damping          */
  double V[36], gc[6];            /* unreduced camera block: equals sba_problem_eval(SBA_MODE_RT, PER_MATCH) */
  double cost, sum_w, n_outlier, gd_max;   /* gd_max: max-norm of the depth gradient                       */
} sba_joint_eq;

/* One reduce pass at (rot, tran), the uploaded depths, depth damping from `radius` (+inf: none).  The depth columns are
 * Jacobi-scaled at this point (opt->jacobi_scaling) before min / max_lm_diagonal clamp their damping.                 */
int sba_problem_eval_joint(sba_problem* p, const double rot[3], const double tran[3], double radius,
                           const sba_lm_options* opt, sba_joint_eq* out);

/* Joint LM from (rot, tran) and the uploaded depths.  The refined depths stay in the handle (folded planes marked
 * stale, as sba_problem_solve_depths does) and are copied to d12_out (double[2n], may be NULL).  summary (may be NULL):
 * num_evaluations counts device passes of either kind.                                                             */
int sba_problem_solve_joint(sba_problem* p, double rot[3], double tran[3], const sba_lm_options* opt,
                            sba_lm_summary* summary, double* d12_out);

/* Covariance of the joint problem at (rot, tran) and the handle's depths -- what ceres::Covariance gives a Ceres user --
 * without a host Jacobian: the robustified problem (sqrt(rho')-scaled Jacobian, Ceres' apply_loss_function = true),
 * undamped, in the tangent space of the gauge (dimension m = 5 with SBA_TRAN_SPHERE, 6 with SBA_TRAN_FREE).  With S the
 * reduced camera system of sba_problem_eval_joint at radius = +inf, P the 6 x m projection of the gauge and U_i, W_i, s_i
 * a match's scaled 2x2 depth block, its 2x6 coupling and its depth scaling:
 *     cov            = P (P^T S P)^-1 P^T                                       6 x 6 over [rot | tran], rank m
 *     depth_cov[3 i] = (var d1_i, var d2_i, cov(d1_i, d2_i))  of  s_i (U_i^-1 + U_i^-1 W_i cov W_i^T U_i^-1) s_i
 * (the depth-camera cross blocks are not formed).  Unscaled: multiply by sigma^2 = 2 cost / dof for residuals of unknown
 * variance.  Two streaming passes; depth_cov == NULL skips the second.
 * Degenerate matches: det(U) / (U11 U22) is sin^2 of the angle between the rays R x1 and x2.  A match whose value is
 * <= min_sin2_parallax (>= 0; negative or NaN: SBA_ERR_INVALID_ARG) or not finite is left out of the problem: it adds
 * nothing to S, cost or sum_w, counts in n_degenerate, and its depth_cov row is (+inf, +inf, 0).
 * opt == NULL: the defaults with tran_param = SBA_TRAN_SPHERE (huber_delta, jacobi_scaling and tran_param are read).
 * Refusals: those of sba_problem_solve_joint.  SBA_ERR_NUMERIC -- the handle stays usable, nothing is written -- when
 * n_used < m, S is not finite, or a pivot of the unit-diagonal projected S is not above m * DBL_EPSILON (a rank-deficient
 * gauge or scene).  The handle's depths and planes are not touched: a later solve returns the bits it returns without
 * this call.                                                                                                          */
typedef struct sba_joint_cov {
  double cov[36];              /* ambient [rot0..2 tran0..2], rank m */
  double cost, sum_w;          /* over the used matches               */
  long long n_used, n_degenerate;
  int dim, dof;                /* m; n_used - m                       */
} sba_joint_cov;
int sba_problem_covariance_joint(sba_problem* p, const double rot[3], const double tran[3],
                                 const sba_lm_options* opt, double min_sin2_parallax,
                                 sba_joint_cov* out, double* depth_cov /* double[3n] or NULL */);

/* ---- triangulated structure: one 3-D point per match, its 3 x 3 covariance, and a cut driven by it ---- */
/* At (rot, tran) and the handle's depths, in camera 2's frame (the frame of the residual), with u_i = R(rot) x1_i:
 *     X_i = ((d1_i u_i - tran) + d2_i x2_i) / 2                   the midpoint of the two ray ends
 *     Sigma_X,i = G_d s_i U_i^-1 s_i G_d^T + K_i cov K_i^T        G_d = [u_i | x2_i] / 2,  K_i = -[A_i | I] / 2 - G_d s_i U_i^-1 W_i
 *     q_i = trace(Sigma_X,i) / (X_i . X_i)                        dimensionless: independent of the gauge's scale
 * -- the covariance of X_i under the joint covariance of sba_problem_covariance_joint over (d_i, rot, tran), the depth-camera
 * cross blocks -s_i U_i^-1 W_i cov included.  Unscaled like that covariance: multiply Sigma_X and q by sigma^2 = 2 cost / dof.
 * xyz [3n], xyz_cov [6n] (per match xx, yy, zz, xy, xz, yz) and score [n] (q) may each be NULL; an output that is not asked
 * for is not computed.  A degenerate match (the rule and min_sin2_parallax of sba_problem_covariance_joint) keeps its X_i as
 * computed, has the covariance row (+inf, +inf, +inf, 0, 0, 0) and q_i = +inf, and adds nothing to the camera system.
 * out, opt, the refusals and SBA_ERR_NUMERIC are those of sba_problem_covariance_joint (same bits in out); on failure nothing
 * is written.  Three launches: that call's reduce pass, its host finish, one streaming pass.  No value depends on a
 * reduction beyond cov: the same bits on every run and for every grid.  The handle's depths and planes are not touched.  */
int sba_problem_structure_joint(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                double min_sin2_parallax, sba_joint_cov* out, double* xyz /* double[3n] or NULL */,
                                double* xyz_cov /* double[6n] or NULL */, double* score /* double[n] or NULL */);
/* The same with the three destinations in DEVICE memory (for example torch tensors): the kernel stores straight into them
 * and nothing but `out` crosses to the host.  Each pointer must be 16-byte aligned (SBA_ERR_INVALID_ARG otherwise).  The work
 * is enqueued on the handle's stream and the call returns after that stream has been waited for.                       */
int sba_problem_structure_joint_device(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                       double min_sin2_parallax, sba_joint_cov* out, double* xyz, double* xyz_cov,
                                       double* score);
/* values[j] = the ranks[j]-th smallest (0-based) of the scores q_i above, selected on the device as
 * sba_problem_residual_order_stats selects: bit for bit an element of `score`, +inf (degenerate matches) above every finite
 * score, NaN above +inf.  1 <= num_ranks <= 8, every ranks[j] < n.                                                      */
int sba_problem_structure_order_stats(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                      double min_sin2_parallax, const size_t* ranks, int num_ranks, double* values);
/* *threshold = scale * q_(rank) (one IEEE f64 multiplication; scale finite and >= 0), then the matches with
 * q_i <= *threshold stay, through the compaction of sba_problem_compact as in sba_problem_keep_below: afterwards the handle is
 * what a fresh upload of the kept matches would be.  A NaN score is dropped; a degenerate match stays only under a threshold
 * of +inf.  The cut is homogeneous in sigma^2, so the unscaled scores serve.                                             */
int sba_problem_structure_keep_below(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                     double min_sin2_parallax, size_t rank, double scale, double* threshold, size_t* n_kept,
                                     long long* kept_index);

/* ---- spherical resection: a further frame's pose from triangulated landmarks ---------------- */
/* Registration of a new frame against existing structure.  The handle's LEFT side is the landmark X_i = d1_i x1_i (the
 * rounded product, as every per-match sweep forms it) in the frame the pose maps from; its RIGHT side y_i = x2_i is the
 * bearing in the new frame (any length > 0: only its direction counts).  THE d2 COLUMN IS NEVER READ.  The landmarks fix
 * the scale, so the pose has all six degrees of freedom and no gauge.  Residual as everywhere, the right depth free per
 * match and eliminated in closed form:
 *     e_i(rot, tran, d) = d y_i - R(rot) X_i + tran        c_i = -R(rot) X_i + tran
 *     d_i* = -(y_i . c_i) / (y_i . y_i)                    the minimiser over d (Huber's rho is monotone in |e|^2)
 *     r_i  = c_i + d_i* y_i = P_i c_i                      P_i = I - y_i y_i^T / (y_i . y_i)
 *     cost = 1/2 sum rho(|r_i|^2)                          rho = Huber with delta = opt->huber_delta (<= 0: none)
 * P_i depends on the data only, so d r_i / d (rot, tran) = P_i [A_i | I] exactly, A_i the rotation Jacobian of the explicit
 * sweep (small-angle handling included), and with w_i = rho' (P idempotent)
 *     H = sum w_i [A | I]^T P_i [A | I]   (6 x 6 over [rot | tran]),      g = sum w_i [A | I]^T r_i.
 * One streaming reduction per evaluation (56 B per match with f64 planes), block rows folded in a fixed order: the same
 * bits on every run.  Once d_i* is stored into the handle's d2 plane (sba_problem_resection_depths) the per-match machinery
 * sees this very problem: sba_problem_residuals(PER_MATCH) returns r_i, and sba_problem_eval(SBA_MODE_RT, PER_MATCH) at the
 * same point has the same cost, n_outlier and g (r is perpendicular to y); only H differs, by sum w J^T y^ y^^T J.
 * n_behind counts the matches with d_i* <= 0 (the landmark lies behind the bearing); they are counted, nothing else.
 * Refusals, all before the first device call: a poisoned handle and one never uploaded as everywhere; no per-match depths,
 * a shard, communicator, peer set or all-reduce hook: SBA_ERR_UNSUPPORTED; a non-finite (rot, tran): SBA_ERR_NUMERIC.
 * Non-finite sums: SBA_ERR_NUMERIC, the handle stays usable.  n == 0 evaluates to zeros.
 * SBA_RESECT_GRID (read per call): at most this many blocks in the reduce, moments and depth passes (tests).            */
typedef struct sba_resection_eq {
  sba_normal_eq eq;            /* H, g, cost, sum_w, n_outlier as above */
  double n_behind;
} sba_resection_eq;
/* opt (may be NULL: the defaults) is read for huber_delta only. */
int sba_problem_eval_resection(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                               sba_resection_eq* out);
/* LM over (rot, tran) from the given start: the schedule of sba_problem_solve (SBA_MODE_RT), one reduce pass per
 * evaluation.  opt == NULL: the defaults, tran_param = SBA_TRAN_FREE (SBA_TRAN_SPHERE is honoured if asked: |tran| stays).
 * summary and n_behind (at the result) may be NULL.  store_depths != 0: sba_problem_resection_depths at the result.       */
int sba_problem_solve_resection(sba_problem* p, double rot[3], double tran[3], const sba_lm_options* opt,
                                sba_lm_summary* summary, double* n_behind, int store_depths);
/* d_i* at (rot, tran) into the handle's d2 plane (the folded planes are marked stale) and, if d2_out != NULL, to the
 * host.  No reduction: the bits do not depend on the grid.                                                              */
int sba_problem_resection_depths(sba_problem* p, const double rot[3], const double tran[3], double* d2_out /* double[n] or NULL */);
/* Linear starting point (DLT).  y is parallel to M X - tau, so [y]x (M X - tau) = 0 is linear in the 12 entries of
 * [M | tau]; with X~ = (X, -1) and Q_i = (y . y) I - y y^T the 12 x 12 moment matrix over the column-major vec([M | tau])
 * is sum (X~ X~^T) (x) Q_i: 60 distinct sums, one streaming pass.  The host takes the eigenvector of the smallest
 * eigenvalue, the sign with det M > 0, projects M onto SO(3) (scale = mean singular value), tran = tau / scale, and
 * the rotation vector by a log map that is well-behaved at angle 0 and near pi.  Exact on noise-free data from 6 matches in
 * general position; NOT robust to outliers: a start for a cut set or a small motion.  info: the eigenvalues lambda1 <=
 * lambda2 and the largest, lambda12; sv: the three singular values of M over their mean (1, 1, 1 on exact data); n_behind
 * at the result.  moments (may be NULL): the 60 sums, slot 6 p + q with p the index of (a <= b) in the upper triangle of
 * X~ X~^T row by row and q that of (c <= d) in Q.  SBA_ERR_NUMERIC (the handle stays usable, rot and tran unwritten):
 * fewer than 6 matches, a non-finite result, or lambda2 <= 12 * 64 * DBL_EPSILON * lambda12 -- a null space of more than
 * one dimension at rounding level, such as a planar landmark set (four).  Anything less degenerate is the caller's call.   */
typedef struct sba_resection_guess_info {
  double lambda1, lambda2, lambda12;
  double sv[3];
  double scale;                /* mean singular value of M: the length of the null vector's rotation part */
  long long n;
  double n_behind;
} sba_resection_guess_info;
int sba_problem_resection_guess(sba_problem* p, double rot[3], double tran[3], sba_resection_guess_info* info,
                                double* moments /* double[60] or NULL */);
/* Candidate poses scored against every match: n_inlier[k] = number of matches with |r_i|^2 <= threshold^2 at candidate k
 * (r_i as sba_problem_eval_resection forms it; threshold^2 is formed once on the host; a non-finite residual is no inlier).
 * One streaming pass for all candidates; the counts are sums of integers: the same on every run and for every grid, and
 * n - n_inlier[k] is sba_problem_eval_resection's n_outlier at huber_delta = threshold.  Refusals, all before the first
 * device call and with nothing written: a NULL argument: SBA_ERR_INVALID_ARG; the handle refusals of the resection; a
 * threshold that is not finite and > 0, count outside 1 .. 1024: SBA_ERR_INVALID_ARG; a non-finite candidate:
 * SBA_ERR_NUMERIC.  n == 0 gives zeros.                                                                                 */
int sba_problem_score_resection(sba_problem* p, const double* rot /* [count][3] */, const double* tran /* [count][3] */,
                                int count, double threshold, long long* n_inlier /* [count] */);
/* Robust starting point: sampled minimal DLT trials, their consensus taken on the device.
 *   1. Trial t seeds s = seed * 0x2545F4914F6CDD1D + t * 0xD6E8FEB86659FD93 + 1 and draws j = splitmix64(s) % n again and
 *      again, skipping a j it already holds, until it holds sample_size distinct matches (draw order; host).
 *   2. One small kernel gathers the sampled rows (X = d1 x1, y) out of the planes; they come back in one copy.
 *   3. Per trial the 60 DLT moments of its rows in draw order and the finish of sba_problem_resection_guess (host, spread
 *      over sba_set_host_threads threads; the result does not depend on their number).  A refused finish: the trial is invalid.
 *   4. Every valid trial's pose is scored as by sba_problem_score_resection, all in one pass.
 *   5. The largest count wins, the lowest trial index among equals.
 *   6. refit != 0: the DLT moments over the winner's inliers only (one more streaming pass), the finish, and the refit's
 *      own score; the refit is returned if its count is >= the winner's, the winner otherwise or if the finish refuses.
 *   7. n_behind at the returned pose from one reduce pass, as sba_problem_resection_guess has it.
 * info->refit: lambda1, lambda2, lambda12, sv, scale and n (the inliers refitted) of the refit's finish, zeros if none was
 * asked for; its n_behind is not filled.  trial_inliers / trial_rot / trial_tran (each may be NULL): every trial's count
 * (-1: refused) and pose (zeros: refused).  Refusals, all before the first device call and with nothing written: a NULL p,
 * opt, rot, tran or info: SBA_ERR_INVALID_ARG; the handle refusals of the resection; a threshold that is not finite and
 * > 0, trials outside 1 .. 1024 or sample_size outside 6 .. 64 (0: the default): SBA_ERR_INVALID_ARG; fewer matches than
 * sample_size: SBA_ERR_NUMERIC.  No trial finishes (every sample degenerate, e.g. a planar landmark set): SBA_ERR_NUMERIC,
 * rot / tran unwritten, the handle stays usable.                                                                         */
typedef struct sba_resection_consensus_options {
  int trials;                  /* 1 .. 1024; 0 = 128 */
  int sample_size;             /* 6 .. 64; 0 = 6 */
  unsigned long long seed;
  double threshold;            /* > 0, finite; landmark units */
  int refit;                   /* != 0: linear refit over the best trial's inliers */
} sba_resection_consensus_options;
typedef struct sba_resection_consensus_info {
  long long n, n_inlier;                   /* matches; inliers at the returned pose */
  long long best_trial, best_trial_inliers;
  long long n_valid_trials;                /* trials whose DLT finish did not refuse */
  int refit_used;                          /* the returned pose is the refit */
  sba_resection_guess_info refit;
  double n_behind;                         /* at the returned pose */
} sba_resection_consensus_info;
int sba_problem_resection_guess_consensus(sba_problem* p, const sba_resection_consensus_options* opt, double rot[3], double tran[3],
                                          sba_resection_consensus_info* info,
                                          long long* trial_inliers /* [trials] or NULL; -1 = trial refused */,
                                          double* trial_rot /* [trials][3] or NULL */, double* trial_tran /* [trials][3] or NULL */);

/* ---- spherical resection weighted by the landmarks' covariances; the pose covariance ---------- */
/* The resection above with every landmark's 3 x 3 covariance Sigma_i (landmark frame; the row sba_problem_structure_joint
 * writes: xx, yy, zz, xy, xz, yz) in place of the unit one.  The weights are FROZEN at a reference pose the caller gives:
 *     S_i = cov_scale R(rot_w) Sigma_i R(rot_w)^T + bearing_sigma^2 d_i*(rot_w, tran_w)^2 (y_i . y_i) I
 *     M_i = S_i^-1 - S_i^-1 y y^T S_i^-1 / (y^T S_i^-1 y)        the information left once the bearing's depth is eliminated
 *     s_i = r_i^T M_i r_i                                         from e = d y - R X + t, e ~ N(0, S_i); a chi^2 with 2 d.o.f.
 *     cost = 1/2 sum rho(s_i)                                     rho = Huber, delta = opt->huber_delta NOW IN SIGMA UNITS
 *     H = sum w_i [A | I]^T M_i [A | I],   g = sum w_i [A | I]^T M_i r_i,   w_i = rho'(s_i)
 * M_i y_i = 0: the eliminated depth d_i*, sba_problem_resection_depths and n_behind are those of the unweighted resection.
 * The weights do not depend on the pose solved for, so g is the exact gradient and H the exact Gauss-Newton matrix.
 * Zero weight (M_i = 0): a Sigma row with a non-finite entry (the degenerate rows of the structure, NaN), a projected S_i
 * that is not positive definite (Sigma = 0 with bearing_sigma = 0, a negative variance), a d_i* at the reference that is not
 * finite.  Such a match adds nothing to any sum (sum_w, n_outlier and n_behind included) and is counted in n_zero_weight,
 * an integer sum: the same on every run and for every grid.
 * On the handle: a copy of the Sigma rows (48 B per match) and three f64 planes of the factored weight (24 B per match),
 * allocated at first use.  EVERY upload and EVERY compaction (sba_problem_compact, _keep_inliers, _keep_below,
 * _structure_keep_below) drops both: the weighted calls then answer SBA_ERR_UNSUPPORTED until the covariances are set and
 * frozen again.  Depth rewrites (sba_problem_set_depths, the depth stages, sba_problem_resection_depths) leave them alone.
 * Refusals of every call below, before the first device call and with nothing written: a NULL argument:
 * SBA_ERR_INVALID_ARG; the handle refusals of the resection; covariances not set, or (eval / weights / covariance) weights
 * not frozen: SBA_ERR_UNSUPPORTED.  SBA_RESECT_GRID caps the weighted reduce pass as it caps the unweighted one.           */
/* cov: 6 n doubles on the host.  cov_scale (finite, > 0, else SBA_ERR_INVALID_ARG) multiplies every row: the place for the
 * pair's sigma^2 = 2 cost / dof.  Setting covariances discards frozen weights.                                            */
int sba_problem_resection_set_landmark_cov(sba_problem* p, const double* cov /* double[6 n] */, double cov_scale);
/* The same from DEVICE memory on the handle's device: 16-byte aligned (else SBA_ERR_INVALID_ARG), copied on the handle's
 * stream; the call returns once the copy is done.                                                                         */
int sba_problem_resection_set_landmark_cov_device(sba_problem* p, const void* cov_dev /* double[6 n] */, double cov_scale);
/* One streaming pass (104 B read, 24 B written per match with f64 planes): the factored weights at (rot_w, tran_w).
 * bearing_sigma: finite and >= 0, else SBA_ERR_INVALID_ARG; a non-finite pose: SBA_ERR_NUMERIC.  n_zero_weight may be NULL.
 * No floating-point reduction: the stored bits do not depend on the grid.                                                 */
int sba_problem_resection_freeze_weights(sba_problem* p, const double rot_w[3], const double tran_w[3], double bearing_sigma,
                                         long long* n_zero_weight);
/* The frozen M_i as rows (xx, yy, zz, xy, xz, yz), zeros for a match of zero weight: for inspection and tests. */
int sba_problem_resection_weights(sba_problem* p, double* info /* double[6 n], host */);
/* sba_problem_eval_resection with the weights as frozen: one streaming reduction (80 B per match with f64 planes; Sigma is
 * not read).  The evaluation pose need not be the reference pose.                                                          */
int sba_problem_eval_resection_weighted(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                        sba_resection_eq* out);
/* reweight_rounds (1 .. 8, else SBA_ERR_INVALID_ARG) times: freeze at the current pose with bearing_sigma, then the LM of
 * sba_problem_solve_resection with the weighted evaluator from that pose.  opt == NULL: the defaults, SBA_TRAN_FREE.  summary
 * (may be NULL) is that of the last round, its seconds_total that of the whole call; n_behind (may be NULL) at the result;
 * store_depths as sba_problem_solve_resection.  The weights stay frozen where the last round froze them.                  */
int sba_problem_solve_resection_weighted(sba_problem* p, double rot[3], double tran[3], const sba_lm_options* opt,
                                         double bearing_sigma, int reweight_rounds, sba_lm_summary* summary, double* n_behind,
                                         int store_depths);
/* The covariance of the resected pose: one weighted reduce pass at (rot, tran) with the weights as frozen, then cov = H^-1
 * by a 6 x 6 Cholesky factorisation on the host.  sigma2 = 2 cost / dof is reported, NOT applied: with honest Sigma_i and
 * bearing_sigma it is near 1.  dof <= 0, non-finite sums or a failed factorisation: SBA_ERR_NUMERIC, nothing written, the
 * handle stays usable.  opt (may be NULL: the defaults) is read for huber_delta only.                                    */
typedef struct sba_resection_cov {
  double cov[36];              /* over [rot | tran], row-major */
  double cost, sum_w;
  long long n_used;            /* n - n_zero_weight */
  long long n_zero_weight;     /* of the freeze */
  double n_outlier;
  long long dof;               /* 2 n_used - 6 */
  double sigma2;               /* 2 cost / dof */
} sba_resection_cov;
int sba_problem_resection_covariance(sba_problem* p, const double rot[3], const double tran[3], const sba_lm_options* opt,
                                     sba_resection_cov* out);

/* ---- the landmark map: landmarks that live across frames, improved by every registered frame's bearings ---------- */
/* A handle of its own (the map outlives any one pair or frame): n landmarks X_i with 3 x 3 covariances Sigma_i (landmark
 * frame; rows xx, yy, zz, xy, xz, yz as sba_problem_structure_joint writes them) and a count of accepted observations per
 * landmark, as nine f64 planes and one u32 plane on the device, padded to whole 16-byte vectors.  It talks to a problem
 * handle through device rows only: sba_problem_structure_joint_device -> sba_landmarks_set_device, and sba_landmarks_get_device
 * -> sba_problem_upload_device (as `left`) + sba_problem_resection_set_landmark_cov_device.
 * sba_landmarks_fuse is ONE streaming pass: per observation (landmark i, bearing y of any length > 0, from the frame at the
 * pose (rot, tran) with covariance Sigma_pose over [rot | tran], absent = 0) the exact linear-Gaussian update
 *     c = -R X + t,  d* = -(y . c) / (y . y),  r = c + d* y                          as the resection forms them
 *     S = R Sigma R^T + bearing_sigma^2 d*^2 (y . y) I + [A | I] Sigma_pose [A | I]^T
 *     M = S^-1 - S^-1 y y^T S^-1 / (y^T S^-1 y),   chi2 = r^T M r                    2 degrees of freedom
 *     X+ = X + Sigma R^T M r,   Sigma+ = Sigma - Sigma R^T M R Sigma
 * computed through the basis and the Cholesky factor of the weighted resection (csrc/sba_landmarks.hpp).  Every observation
 * falls into one class, tested in this order: SKIPPED (a non-finite entry of X or Sigma, S not positive definite across
 * the bearing, a non-finite d* -- a zero bearing --, a non-finite result; chi2 = NaN), BEHIND (d* <= 0), GATED (chi2 >
 * chi2_gate), FUSED.  Only a fused landmark is rewritten, and its count incremented.  The five counts are integer sums and
 * there is no floating-point reduction: every result is the same on every run and for every grid (SBA_RESECT_GRID caps it).
 * The pose term treats the pose as independent of the bearings and of the other landmarks: a pose resected from the same
 * bearings is correlated with them, and landmarks fused at one pose become correlated with each other; neither is modelled.
 * Refusals, all before the first device call with nothing written and the handle usable: a NULL argument, a bad option, a
 * bad idx or m: SBA_ERR_INVALID_ARG; a non-finite pose: SBA_ERR_NUMERIC; a poisoned handle: SBA_ERR_HIP.                  */
typedef struct sba_landmarks sba_landmarks;
int sba_landmarks_create(sba_landmarks** out, int device, void* stream /* hipStream_t or NULL: own stream */);
int sba_landmarks_destroy(sba_landmarks* h);
int sba_landmarks_size(const sba_landmarks* h, size_t* n);
/* Replace the map: xyz 3 n and cov 6 n doubles on the host.  cov_scale (finite, > 0) multiplies every covariance row as it
 * is packed; every observation count becomes 0.  n == 0 empties the map.                                                  */
int sba_landmarks_set(sba_landmarks* h, const double* xyz /* double[3 n] */, const double* cov /* double[6 n] */, size_t n,
                      double cov_scale);
/* The same from DEVICE rows on the handle's device, 16-byte aligned (else SBA_ERR_INVALID_ARG): what
 * sba_problem_structure_joint_device wrote.  Returns once the rows have been read.                                        */
int sba_landmarks_set_device(sba_landmarks* h, const void* xyz_dev, const void* cov_dev, size_t n, double cov_scale);
/* The map as host rows; either array may be NULL. */
int sba_landmarks_get(sba_landmarks* h, double* xyz /* double[3 n] or NULL */, double* cov /* double[6 n] or NULL */);
/* The map as rows in the caller's DEVICE memory (16-byte aligned, either may be NULL), exactly n rows each, in the layout
 * sba_problem_upload_device reads as `left` and sba_problem_resection_set_landmark_cov_device reads.  Complete on return.  */
int sba_landmarks_get_device(sba_landmarks* h, void* xyz_dev, void* cov_dev);
/* Accepted observations per landmark since the last set. */
int sba_landmarks_counts(sba_landmarks* h, uint32_t* out /* [n] */);
typedef struct sba_landmark_fuse_options {
  double bearing_sigma;        /* radians; finite and >= 0 */
  double chi2_gate;            /* > 0; +inf: no gate; NaN or <= 0 is refused */
  const double* pose_cov;      /* 36 doubles, row-major over [rot | tran] (sba_resection_cov.cov), or NULL: none.  Finite,
                                  symmetric to the bit, diagonal >= 0 */
  int apply;                   /* 0: a dry run -- chi2 and counts only, nothing stored */
} sba_landmark_fuse_options;
typedef struct sba_landmark_fuse_result {
  long long n_obs;             /* = n_skipped + n_behind + n_gated + n_fused */
  long long n_skipped, n_behind, n_gated, n_fused;
} sba_landmark_fuse_result;
/* idx == NULL: the dense form, m must equal n, observation j is landmark j and a zero bearing means "not seen" (skipped).
 * Otherwise observation j is landmark idx[j]: strictly increasing and < n, validated on the host in one pass.  bearings:
 * 3 m doubles on the host.  chi2_out (m doubles, may be NULL) receives every observation's chi2.  An empty map or m == 0:
 * zeros and SBA_OK.                                                                                                      */
int sba_landmarks_fuse(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */, size_t m,
                       const double rot[3], const double tran[3], const sba_landmark_fuse_options* opt,
                       sba_landmark_fuse_result* res, double* chi2_out /* [m] or NULL */);

/* ---- the landmark map, edited on the device: scores, prune, append, gather ------------------------------------------- */
/* One turn of incremental mapping without the map leaving the device: sba_landmarks_gather_device the landmarks a frame
 * matched -> sba_problem_upload_device + sba_problem_resection_set_landmark_cov_device -> resect -> sba_landmarks_fuse ->
 * sba_landmarks_append_device what the new pair triangulated -> sba_landmarks_prune what stayed bad.  The observation
 * counts survive every edit; only sba_landmarks_set zeroes them.
 *   score_i = ((Sigma_xx + Sigma_yy) + Sigma_zz) / ((X.x X.x + X.y X.y) + X.z X.z)      trace Sigma / X . X, as the structure's
 * in exactly this order in f64 without contraction: float64 arithmetic in the same order gives the same bits.  Nothing is
 * special-cased: a non-finite input gives a non-finite score, X = 0 gives +inf or NaN.
 * A prune puts every landmark into one class, tested in this order: INVALID (a non-finite entry of X or Sigma, a negative
 * variance), UNCERTAIN (!(score <= max_score)), UNOBSERVED (count < min_count), MASKED (mask[i] == 0), KEPT.  With apply the
 * handle then equals a fresh sba_landmarks_set of the kept rows in their old order with their old counts attached: a stable
 * compaction into a second plane allocation the handle keeps, after which the two are swapped (a steady prune / append cycle
 * allocates nothing once both have grown to the map's largest size).  The class counts are integer sums: every result is
 * the same on every run and for every grid.
 * Refusals, all before the first device call with nothing written and the handle unchanged and usable: a NULL handle or
 * required pointer, a bad option, an index out of range, misaligned device rows, a size whose byte counts overflow:
 * SBA_ERR_INVALID_ARG; a poisoned handle: SBA_ERR_HIP.                                                                     */
int sba_landmarks_scores(sba_landmarks* h, double* out /* [n] */);
typedef struct sba_landmark_prune_options {
  double max_score;            /* >= 0; +inf: no cut; NaN or negative is refused */
  uint32_t min_count;          /* accepted observations a landmark needs; 0: no cut */
  const uint8_t* mask;         /* [n] on the host, 0 = drop, or NULL: none */
  int apply;                   /* 0: a dry run -- the counts and `kept` only, the map unchanged */
} sba_landmark_prune_options;
typedef struct sba_landmark_prune_result {
  long long n_before;          /* = n_invalid + n_uncertain + n_unobserved + n_masked + n_kept */
  long long n_invalid, n_uncertain, n_unobserved, n_masked, n_kept;
} sba_landmark_prune_result;
/* kept (n entries of room, or NULL) receives the old indices of the n_kept kept landmarks, ascending. */
int sba_landmarks_prune(sba_landmarks* h, const sba_landmark_prune_options* opt, sba_landmark_prune_result* res,
                        int64_t* kept /* [n] or NULL */);
/* n_add rows in sba_landmarks_set's layout behind the map's n: the first n landmarks and their counts stay, the new ones
 * follow with count 0 and cov_scale applied -- as if set had been called with the concatenated rows and the old counts
 * restored.  n_add == 0 changes nothing; onto an empty map this is set.  The device rows: 16-byte aligned, exactly n_add
 * of each are read, complete on return.                                                                                   */
int sba_landmarks_append(sba_landmarks* h, const double* xyz /* double[3 n_add] */, const double* cov /* double[6 n_add] */,
                         size_t n_add, double cov_scale);
int sba_landmarks_append_device(sba_landmarks* h, const void* xyz_dev, const void* cov_dev, size_t n_add, double cov_scale);
/* Rows idx[j] of the map in sba_landmarks_get's row layout, exactly m of each; any output may be NULL.  idx: on the host,
 * any order, repeats allowed, 0 <= idx[j] < n, validated in one pass.  The device form writes 16-byte aligned DEVICE rows:
 * what sba_problem_upload_device reads as `left` and sba_problem_resection_set_landmark_cov_device reads.                  */
int sba_landmarks_gather(sba_landmarks* h, const int64_t* idx /* [m] */, size_t m, double* xyz /* double[3 m] or NULL */,
                         double* cov /* double[6 m] or NULL */, uint32_t* counts /* [m] or NULL */);
int sba_landmarks_gather_device(sba_landmarks* h, const int64_t* idx /* [m], host */, size_t m, void* xyz_dev, void* cov_dev);

/* ---- the landmark map: a frame's pose and its landmarks solved jointly ------------------------------------------------ */
/* sba_landmarks_register replaces the chain gather -> upload -> weighted resection -> its covariance -> sba_landmarks_fuse by one
 * call on the map, and removes that chain's two approximations: the pose is no longer treated as independent of the bearings
 * it was estimated from, and the landmarks' correlation through the shared pose enters every posterior.  Unknowns: the pose
 * (rot, tran) and every observed landmark X_j with the map's row as its prior N(Xb_j, Sigma_j); the bearing y_j (any length
 * > 0) is measured with isotropic noise s_j^2 = bearing_sigma^2 d*_j^2 (y_j . y_j) across the ray, FROZEN at the start pose and
 * Xb_j.  There is no pose prior: the landmarks fix gauge and scale.  With the pose held every landmark is eliminated exactly, so
 * an evaluation is one streaming pass over the map (csrc/sba_landmarks_register.hpp):
 *     S = R Sigma R^T + s_j^2 I,  W as in sba_landmarks_fuse,  u = W r,  chi2 = u . u,  T = Sigma R^T W^T,  Xh = Xb + T u
 *     J_w = W [A(Xh) | I],   H = sum J_w^T J_w,   g = sum J_w^T u,   cost = 1/2 sum chi2
 * and at the solution, with the pose covariance Sigma_c = H^-1:  X+ = Xh,  Sigma+ = Sigma - T T^T + T J_w Sigma_c J_w^T T^T.
 * Every observation falls into one class: SKIPPED (a non-finite entry of X or Sigma, a zero or non-finite bearing, a non-finite
 * d*, S not positive definite across the bearing at the freeze or at the solution, a non-finite result; chi2 = NaN), BEHIND
 * (d* <= 0 at the freeze or at the solution), GATED (chi2 > chi2_gate AT THE SOLUTION), FUSED.  Observations skipped or behind at
 * the freeze take no part in the solve.  GATED observations DID take part in it, and so did those found behind only at the
 * solution: the solve has no robust loss, and a caller who wants them out registers again without them (chi2_out and a dry run
 * tell which).  Only a fused landmark is rewritten, and its count incremented.  sba_landmarks_register_robust (below) is the
 * same solve under a Huber loss, for frames that carry wrong matches.
 * Refusals, all before the first device call with nothing written and the handle usable: a NULL argument, a bad bearing_sigma,
 * chi2_gate, idx or m: SBA_ERR_INVALID_ARG; lm.huber_delta != 0: SBA_ERR_UNSUPPORTED; a non-finite pose: SBA_ERR_NUMERIC; a
 * poisoned handle: SBA_ERR_HIP.  After the freeze, with the map untouched: fewer than 3 observations that take part, a failed
 * solve or an H that is not positive definite at the solution: SBA_ERR_NUMERIC.  An empty map or m == 0: SBA_OK, zero counts
 * and the start pose.                                                                                                     */
typedef struct sba_landmark_register_options {
  double bearing_sigma;        /* radians; finite and >= 0 */
  double chi2_gate;            /* > 0; +inf: no gate; NaN or <= 0 is refused */
  int apply;                   /* 0: a dry run -- the pose, its covariance, chi2 and counts, nothing stored */
  sba_lm_options lm;           /* huber_delta must be 0.  max_num_iterations = 0: register at the given pose -- the freeze, one
                                  evaluation, the covariance, the write-back */
} sba_landmark_register_options;
typedef struct sba_landmark_register_result {
  double rot[3], tran[3];      /* the solved pose */
  double cov[36];              /* Sigma_c, row-major over [rot | tran]: the layout of sba_resection_cov.cov */
  sba_lm_summary summary;
  long long n_obs;             /* = n_skipped + n_behind + n_gated + n_fused */
  long long n_skipped, n_behind, n_gated, n_fused;
  long long n_used;            /* observations that entered the sums at the solution */
} sba_landmark_register_result;
typedef struct sba_landmark_register_eval {
  double H[36];                /* row-major symmetric 6 x 6 over [rot | tran] */
  double g[6];
  double cost;
  long long n_used;            /* observations that entered the sums */
  long long n_behind;          /* of which: d* <= 0 at the evaluation pose */
} sba_landmark_register_eval;
/* One evaluation at (rot, tran) with the noise frozen at (rot_ref, tran_ref); the map is not written.  opt->apply and
 * opt->chi2_gate (checked all the same) play no part. */
int sba_landmarks_eval_register(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */,
                                size_t m, const double rot[3], const double tran[3], const double rot_ref[3],
                                const double tran_ref[3], const sba_landmark_register_options* opt,
                                sba_landmark_register_eval* eval);
/* The solve from (rot0, tran0) and, with opt->apply, the write-back.  idx, bearings and m as for sba_landmarks_fuse (idx ==
 * NULL: the dense form, m == n, a zero bearing means "not seen").  chi2_out (m doubles, may be NULL) receives every
 * observation's chi2 at the solution, NaN where skipped.                                                                */
int sba_landmarks_register(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */, size_t m,
                           const double rot0[3], const double tran0[3], const sba_landmark_register_options* opt,
                           sba_landmark_register_result* res, double* chi2_out /* [m] or NULL */);

/* ---- the landmark map: the joint registration under a robust loss ------------------------------------------------------ */
/* THE OBJECTIVE.  With f_j the block of landmark j in sba_landmarks_register's F (its bearing term plus its prior term), the loss
 * sits on every block, as Ceres applies a loss to a residual block:
 *     F_rho = sum_j rho( min_X f_j(X, pose) )
 * rho is monotone, so the minimisation over X_j passes through it: eliminating the landmark is still exact, Xh_j is unchanged,
 * and F_rho(pose) = sum_j rho(chi2_j) with chi2_j = u . u as above remains.  rho is the project's Huber, rho(s) = s for
 * s <= delta^2 and 2 delta sqrt(s) - delta^2 beyond, w = rho'(s), delta = lm.huber_delta on the whitened, dimensionless |u|.
 *     H = sum w_j J_w^T J_w  (Gauss-Newton, no second-order loss term),  g = sum w_j J_w^T u  (the exact gradient of 1/2 F_rho),
 *     cost = 1/2 sum rho(chi2_j),  n_outlier = the observations that entered the sums with chi2_j > delta^2
 * THE WRITE-BACK is sba_landmarks_register's with Sigma_c = H_rho^-1 at the solution and classes by chi2_gate, and chi2_gate >
 * delta^2 IS REFUSED (+inf counts as larger): an observation the loss downweights has w < 1, the conditional covariance of its
 * block would be Sigma_cond / w, and fusing it would inflate the landmark.  With chi2_gate <= delta^2 every fused observation had
 * weight exactly 1, so its posterior X+ = Xh, Sigma+ = Sigma_cond + G Sigma_c G^T is the weighted problem's own, and every
 * downweighted observation is GATED: its landmark stays untouched, byte for byte.
 * opt: sba_landmark_register_options with lm.huber_delta finite and > 0.  The records are the non-robust ones followed by
 * n_outlier.  The _device twins take `bearings` as a DEVICE pointer to 3 m doubles in the same row layout (8-byte aligned), on
 * the handle's device and complete on its stream, and sba_landmarks_register_robust_device writes chi2_out to DEVICE memory (m
 * doubles, or NULL).  The kernels read the caller's bearings in place; only the dense form over an odd n, or from a pointer that
 * is not 16-byte aligned, is first copied device to device, because its 16-byte vector loads would otherwise end behind the
 * caller's array.  idx stays on the host: it is checked there before the first device call.
 * Refusals, all before the first device call with nothing written and the handle usable: everything sba_landmarks_register
 * refuses, with the same codes, the loss excepted; lm.huber_delta NaN, infinite or <= 0, chi2_gate > delta^2, a misaligned
 * device pointer: SBA_ERR_INVALID_ARG.  After the freeze the same SBA_ERR_NUMERIC cases as sba_landmarks_register.            */
typedef struct sba_landmark_register_robust_result {
  double rot[3], tran[3];      /* the solved pose */
  double cov[36];              /* Sigma_c = H_rho^-1, row-major over [rot | tran] */
  sba_lm_summary summary;
  long long n_obs;             /* = n_skipped + n_behind + n_gated + n_fused */
  long long n_skipped, n_behind, n_gated, n_fused;
  long long n_used;            /* observations that entered the sums at the solution */
  long long n_outlier;         /* of which: chi2 > delta^2 at the solution */
} sba_landmark_register_robust_result;
typedef struct sba_landmark_register_robust_eval {
  double H[36];                /* row-major symmetric 6 x 6 over [rot | tran] */
  double g[6];
  double cost;
  long long n_used;            /* observations that entered the sums */
  long long n_behind;          /* of which: d* <= 0 at the evaluation pose */
  long long n_outlier;         /* of which: chi2 > delta^2 */
} sba_landmark_register_robust_eval;
int sba_landmarks_eval_register_robust(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */,
                                       size_t m, const double rot[3], const double tran[3], const double rot_ref[3],
                                       const double tran_ref[3], const sba_landmark_register_options* opt,
                                       sba_landmark_register_robust_eval* eval);
int sba_landmarks_register_robust(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */,
                                  size_t m, const double rot0[3], const double tran0[3], const sba_landmark_register_options* opt,
                                  sba_landmark_register_robust_result* res, double* chi2_out /* [m] or NULL */);
int sba_landmarks_eval_register_robust_device(sba_landmarks* h, const int64_t* idx /* [m], host, or NULL */,
                                              const void* bearings_dev /* double[3 m], device */, size_t m, const double rot[3],
                                              const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                              const sba_landmark_register_options* opt, sba_landmark_register_robust_eval* eval);
int sba_landmarks_register_robust_device(sba_landmarks* h, const int64_t* idx /* [m], host, or NULL */,
                                         const void* bearings_dev /* double[3 m], device */, size_t m, const double rot0[3],
                                         const double tran0[3], const sba_landmark_register_options* opt,
                                         sba_landmark_register_robust_result* res, void* chi2_out_dev /* double[m], device, or NULL */);

/* ---- the landmark map: the joint registration under a redescending (Hampel) loss ------------------------------------ */
/* Huber's influence is bounded but not zero: a wrong match far out keeps pulling with |w u| = delta while H_rho counts it with
 * a small weight, so sba_landmarks_register_robust's Sigma_c is optimistic on frames with wrong matches.  The same objective
 * F_rho = sum_j rho(chi2_j) under Hampel's three-part loss removes that.  With s = chi2_j, r = sqrt(s), 0 < a < b < c:
 *     s <= a^2          w = 1                           rho = s
 *     a^2 < s <= b^2    w = a / r                       rho = 2 a r - a^2
 *     b^2 < s <= c^2    w = a (c - r) / ((c - b) r)     rho = a (b + c) - a^2 - a (c - r)^2 / (c - b)
 *     s > c^2           w = 0                           rho = a (b + c) - a^2
 * w = rho'(s), rho is C1, a = base.lm.huber_delta.  H = sum w J_w^T J_w, g = sum w J_w^T u, cost = 1/2 sum rho as above;
 * n_outlier = the used observations with s > a^2, n_rejected = those with s > c^2 (weight exactly 0).  b = c = +inf is Huber.
 * THE WRITE-BACK is sba_landmarks_register_robust's, with Sigma_c = H_rho^-1 and chi2_gate > a^2 refused: Hampel's weight is
 * exactly 1 up to a, so every fused observation had weight 1 and every downweighted or rejected one is GATED, its landmark
 * untouched byte for byte.
 * THE OBJECTIVE IS NOT CONVEX.  With huber_first != 0 the call first runs sba_landmarks_register_robust's solve (delta = a, the
 * same lm options, the same frozen noise) from rot0 | tran0, reports its pose and iteration count in rot_huber, tran_huber,
 * huber_iterations, and runs the Hampel solve from there on the same frozen noise; summary is the second solve's.  With
 * huber_first == 0 the Hampel solve starts at rot0 | tran0 and the three fields are the start pose and 0.
 * Refusals, all before the first device call with nothing written and the handle usable: everything
 * sba_landmarks_register_robust refuses, with the same codes (chi2_gate > a^2 among them); b or c NaN, b <= a, c <= b, exactly
 * one of them infinite: SBA_ERR_INVALID_ARG.  After the freeze the same SBA_ERR_NUMERIC cases, and n_used - n_rejected < 3 at
 * the solution (fewer than three observations carry weight): SBA_ERR_NUMERIC with the map untouched.  The _device twins as above. */
typedef struct sba_landmark_register_hampel_options {
  sba_landmark_register_options base;  /* base.lm.huber_delta = a */
  double b, c;                 /* finite with a < b < c, or both +inf */
  int huber_first;             /* != 0: the Huber solve first, the Hampel solve from its minimiser */
} sba_landmark_register_hampel_options;
typedef struct sba_landmark_register_hampel_result {
  double rot[3], tran[3];      /* the solved pose */
  double cov[36];              /* Sigma_c = H_rho^-1, row-major over [rot | tran] */
  sba_lm_summary summary;      /* of the Hampel solve */
  long long n_obs;             /* = n_skipped + n_behind + n_gated + n_fused */
  long long n_skipped, n_behind, n_gated, n_fused;
  long long n_used;            /* observations that entered the sums at the solution */
  long long n_outlier;         /* of which: chi2 > a^2 at the solution */
  long long n_rejected;        /* of which: chi2 > c^2 at the solution, weight 0 */
  double rot_huber[3], tran_huber[3];  /* the Huber stage's minimiser, or the start pose */
  int huber_iterations;        /* the Huber stage's summary.num_iterations, or 0 */
} sba_landmark_register_hampel_result;
typedef struct sba_landmark_register_hampel_eval {
  double H[36];                /* row-major symmetric 6 x 6 over [rot | tran] */
  double g[6];
  double cost;
  long long n_used;            /* observations that entered the sums */
  long long n_behind;          /* of which: d* <= 0 at the evaluation pose */
  long long n_outlier;         /* of which: chi2 > a^2 */
  long long n_rejected;        /* of which: chi2 > c^2 */
} sba_landmark_register_hampel_eval;
int sba_landmarks_eval_register_hampel(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */,
                                       size_t m, const double rot[3], const double tran[3], const double rot_ref[3],
                                       const double tran_ref[3], const sba_landmark_register_hampel_options* opt,
                                       sba_landmark_register_hampel_eval* eval);
int sba_landmarks_register_hampel(sba_landmarks* h, const int64_t* idx /* [m] or NULL */, const double* bearings /* double[3 m] */,
                                  size_t m, const double rot0[3], const double tran0[3], const sba_landmark_register_hampel_options* opt,
                                  sba_landmark_register_hampel_result* res, double* chi2_out /* [m] or NULL */);
int sba_landmarks_eval_register_hampel_device(sba_landmarks* h, const int64_t* idx /* [m], host, or NULL */,
                                              const void* bearings_dev /* double[3 m], device */, size_t m, const double rot[3],
                                              const double tran[3], const double rot_ref[3], const double tran_ref[3],
                                              const sba_landmark_register_hampel_options* opt, sba_landmark_register_hampel_eval* eval);
int sba_landmarks_register_hampel_device(sba_landmarks* h, const int64_t* idx /* [m], host, or NULL */,
                                         const void* bearings_dev /* double[3 m], device */, size_t m, const double rot0[3],
                                         const double tran0[3], const sba_landmark_register_hampel_options* opt,
                                         sba_landmark_register_hampel_result* res, void* chi2_out_dev /* double[m], device, or NULL */);

/* ---- the landmark map's descriptors, and a frame associated with the map on the device ------------
 * The map may keep one f32 descriptor row per landmark, packed, next to its planes.  A map that never receives descriptors
 * behaves as before, byte for byte, and allocates nothing for them.  On a map that keeps them: sba_landmarks_set / _set_device
 * drop them (the map is replaced); sba_landmarks_prune with apply moves the kept landmarks' rows to their rank with the planes
 * (the handle then equals a fresh set + set_descriptors of the kept rows; a dry run moves nothing; pruning to empty keeps dim);
 * sba_landmarks_append / _append_device add rows that are all NaN, which no frame row is ever associated with until they are
 * described (the matcher never chooses a train row with a non-finite component); fuse, register*, scores and gather* neither read
 * nor write them.
 *
 * set_descriptors: n_rows must equal the map's n, 1 <= dim <= 256, row_stride_bytes a multiple of 4 and >= 4 dim as for
 * sba_match_descriptors (a padded cv::Mat passes as is); a second call replaces the rows and may change dim; dim == 0 drops the
 * descriptors (desc is ignored).  The _device twin takes device rows on the handle's device, 4-byte aligned, complete on return.
 * descriptor_dim: 0 = the map keeps none.  get_descriptors: rows idx[j] (host indices, any order, repeats allowed, validated in
 * one pass as for sba_landmarks_gather) or, idx == NULL, all n rows (m is ignored), at a stride of out_stride_bytes.
 * append_described: sba_landmarks_append plus the new rows' descriptors; allowed when the map keeps descriptors of the same dim
 * or is empty (it then acts as set plus set_descriptors); the _device twin takes all three arrays on the device, xyz and cov
 * 16-byte aligned as for sba_landmarks_append_device.                                                                            */
int sba_landmarks_set_descriptors(sba_landmarks* h, const float* desc, size_t n_rows, int dim, size_t row_stride_bytes);
int sba_landmarks_set_descriptors_device(sba_landmarks* h, const void* desc_dev, size_t n_rows, int dim, size_t row_stride_bytes);
int sba_landmarks_descriptor_dim(const sba_landmarks* h, int* dim);
int sba_landmarks_get_descriptors(sba_landmarks* h, const int64_t* idx /* [m] or NULL: all n rows */, size_t m, float* out,
                                  size_t out_stride_bytes);
int sba_landmarks_append_described(sba_landmarks* h, const double* xyz /* double[3 n_add] */, const double* cov /* double[6 n_add] */,
                                   const float* desc, size_t n_add, int dim, size_t row_stride_bytes, double cov_scale);
int sba_landmarks_append_described_device(sba_landmarks* h, const void* xyz_dev, const void* cov_dev, const void* desc_dev, size_t n_add,
                                          int dim, size_t row_stride_bytes, double cov_scale);
/* sba_landmarks_associate: a frame's descriptors in, idx and the gathered bearings out -- exactly what sba_landmarks_register*_device
 * takes as idx (host) and bearings_dev.  THE RULE, which the device follows bit for bit:
 *   1. Match.   sba_match_descriptors' matcher with the frame rows as queries and the map's rows as train rows, unchanged: frame
 *               row j gets (i0, d0) and (i1, d1) and is ACCEPTED iff i1 >= 0, d0 < ratio * d1 in float and d0 <= max_distance in
 *               float.
 *   2. Claim.   Landmark i's claimants are the accepted rows with i0 == i.  Its winner is the claimant smallest in (bits of d0 as
 *               u32, j), compared lexicographically; d0 >= 0, so the bit order is the value order, and among equal distances the
 *               lowest frame row wins.
 *   3. Output.  Output k is the k-th smallest landmark that has a claimant: idx_out[k] = i, row_out[k] its winner, dist_out[k] the
 *               winner's d0, bearings_out[3 k .. 3 k + 2] a bitwise copy of frame_bearings[3 row .. 3 row + 2] (skipped when either
 *               pointer is NULL).  idx_out is strictly increasing and row_out has no repeats.
 *   4. Counts.  n_accepted = n_contested + n_associated; n_frame = m_frame.
 * Every output holds min(n, m_frame) rows; n_associated of them are written.  n < 2 or m_frame == 0: zeros and SBA_OK (with fewer
 * than two train rows nothing matches).  A frame row with a non-finite component matches nothing.  ratio: finite and > 0;
 * max_distance: > 0, +inf for none.  The _device form reads frame_desc_dev (4-byte aligned) and frame_bearings_dev (8-byte
 * aligned) on the handle's device and writes bearings_out_dev (16-byte aligned) there; idx_out, row_out and dist_out are on the
 * host in both forms.  The result has the same bytes on every run and for every grid.
 * Refusals, each before any device call, with nothing written and the handle usable: a NULL handle / opt / res / frame_desc, a
 * bad option, a dim that is not the map's, a map without descriptors, a bad stride, n or m_frame >= 2^31, a misaligned device
 * pointer: SBA_ERR_INVALID_ARG; a poisoned handle: SBA_ERR_HIP.                                                                  */
typedef struct sba_landmark_associate_options {
  float ratio;        /* the ratio test, as sba_match_descriptors' */
  float max_distance; /* an accepted row has d0 <= this; +inf: no cut */
} sba_landmark_associate_options;
typedef struct sba_landmark_associate_result {
  long long n_frame, n_accepted, n_contested, n_associated;
} sba_landmark_associate_result;
int sba_landmarks_associate(sba_landmarks* h, const float* frame_desc, size_t m_frame, int dim, size_t row_stride_bytes,
                            const double* frame_bearings /* double[3 m_frame] or NULL */, const sba_landmark_associate_options* opt,
                            sba_landmark_associate_result* res, int64_t* idx_out, int32_t* row_out, float* dist_out,
                            double* bearings_out /* each may be NULL */);
int sba_landmarks_associate_device(sba_landmarks* h, const void* frame_desc_dev, size_t m_frame, int dim, size_t row_stride_bytes,
                                   const void* frame_bearings_dev /* double[3 m_frame], device, or NULL */,
                                   const sba_landmark_associate_options* opt, sba_landmark_associate_result* res,
                                   int64_t* idx_out /* host */, int32_t* row_out /* host */, float* dist_out /* host */,
                                   void* bearings_out_dev /* double[3 min(n, m_frame)], device, 16-byte aligned, or NULL */);

/* ---- multi-GPU: one process (and one sba_problem) per GPU, correspondences sharded ------ */
/* Option A: native RCCL.  Rank 0 calls sba_comm_unique_id, ships the 128 bytes to the other
 * ranks by any host channel, then every rank calls sba_problem_comm_init_rank.  After that
 * every eval / solve all-reduces the 24-double pack once (ncclAllReduce, ncclDouble, ncclSum). */
#define SBA_COMM_ID_BYTES 128
int sba_comm_unique_id(char id[SBA_COMM_ID_BYTES]);
int sba_problem_comm_init_rank(sba_problem* p, int nranks, int rank, const char id[SBA_COMM_ID_BYTES]);
/* 1 if librccl could be loaded and bound in this process (0: reason in sba_last_error).  ncclCommInitRank is itself
 * a collective: a rank that cannot even load the library would leave the others waiting inside it, so ranks agree on
 * this BEFORE any of them calls sba_problem_comm_init_rank.                                                        */
int sba_rccl_available(void);
/* Tear the communicator down again (after a rank reported failure: all ranks destroy theirs and fall back together). */
int sba_problem_comm_destroy(sba_problem* p);
/* Option C: direct peer exchange, no collective library on the data path.  Every rank owns a 4 KiB inbox in
 * fine-grained device memory that all peers map through HIP IPC; per sweep one wave stores its 24 doubles into every
 * peer's inbox (over xGMI), polls its own inbox and sums the nranks contributions in rank order (bit-identical on all
 * ranks), then publishes to the host.  Set-up: every rank calls sba_problem_peer_export (allocates the inbox, returns
 * its 64-byte IPC handle), the handles are all-gathered by any host channel into handles[nranks][64], every rank calls
 * sba_problem_peer_connect, then all ranks together sba_problem_peer_selftest; on any failure call
 * sba_problem_peer_disable everywhere and use option A.  At most 8 ranks (one node).                            */
#define SBA_PEER_HANDLE_BYTES 64
int sba_problem_peer_export(sba_problem* p, int nranks, int rank, char handle[SBA_PEER_HANDLE_BYTES]);
int sba_problem_peer_connect(sba_problem* p, const char* handles);
int sba_problem_peer_selftest(sba_problem* p, int rounds, int* ok);
int sba_problem_peer_disable(sba_problem* p);
/* Option B: user hook (e.g. torch.distributed.all_reduce on a tensor aliasing device_buf).  */
int sba_problem_set_allreduce(sba_problem* p, sba_allreduce_fn fn, void* user);
/* Which shard of the correspondences this problem holds.  sba_problem_comm_init_rank and sba_problem_peer_export set
 * it themselves; with the user hook call it explicitly before sba_problem_solve_depths, whose two max-norms
 * (projected gradient, step) travel through the SUM all-reduce as one pack slot per shard each (hence at most 8
 * shards).                                                                                                         */
int sba_problem_set_shard(sba_problem* p, int rank, int nranks);
/* Device address of the 24-double result pack the hook / RCCL operates on (a sum over
 * correspondences in either kernel's layout, so summing it across shards is exact).            */
int sba_problem_pack_device_ptr(sba_problem* p, void** dev_ptr);

/* Host threads for the host-side loops that have any (the trials of the initial guess; the per-pair LM steps of
 * sba_batch_solve, from 64 pairs per thread) -- the counterpart of
 * the reference's set_omp(num_proc) (.cpp:835-841).  0 = one per hardware thread (at most 16); default 1, or
 * SBA_HOST_THREADS.  Process-wide; results do not depend on it.  A trial costs a few microseconds, so threads are
 * only started when there are at least 256 trials per thread (the reference's 80 trials run serially).           */
int sba_set_host_threads(int n);

/* ---- 8-point initial guess (eight_point_estimation / initial_guess, spherical_bundle_adjuster.cpp:47-181) ---- */
/* Device part: one pass over the uploaded correspondences accumulating A^T A of the rows kron(left_i, right_i)
 * (.cpp:53-68) for 64 interleaved groups, group(i) = (i / 2) % 64.  groups: double[64][45] (upper triangle,
 * row-major a <= b).  With a transport attached (sharded problem) the sums are all-reduced: every rank receives
 * the moments of the whole problem (group g = the union of all shards' group g) and so derives the same guess.  */
int sba_problem_epipolar_moments(sba_problem* p, double* groups);
/* Host part (no device needed): `trials` trials (80 in the reference, .cpp:130), each on a random
 * `subset_fraction` (0.25, .cpp:133) of the groups: null vector of A (smallest eigenvector of A^T A), rank-2
 * projection, decomposeEssentialMat, Euler angles, validity (< 1.57), consensus pick by 20-80 % trimmed mean
 * distance.  Outputs R_vec_out (Euler angles) and T_vec_out of the reference; the reference then starts the BA
 * from init_rot = -R_vec_out, init_tran = T_vec_out (.cpp:330-331).                                          */
int sba_initial_guess_from_moments(const double* groups, int trials, double subset_fraction,
                                   unsigned long long seed, double rot_euler[3], double tran[3],
                                   int* num_candidates);
/* Both parts.  SBA_GUESS_SAMPLING=reference in the environment routes this call to sba_problem_initial_guess_reference
 * (seed is then unused) for problems it supports.                                                            */
int sba_problem_initial_guess(sba_problem* p, int trials, double subset_fraction, unsigned long long seed,
                              double rot_euler[3], double tran[3], int* num_candidates);

/* ---- the same initial guess from the REFERENCE'S OWN random subsets (small problems) ------------------------- */
/* The random stream behind it.  The reference shuffles with std::random_shuffle on rand(), which it never seeds: glibc's
 * generator in its srand(1) state.  The library keeps its OWN copy of that generator (same algorithm, same values --
 * pinned against the real rand() by the tests), starting in the never-seeded state and running on from call to call like
 * the reference's stream does from image pair to image pair.  It does not borrow the process's rand(): once HIP is
 * initialised that stream is no longer the caller's alone (libhsa-runtime64 imports srand / rand).  SBA_GUESS_RAND=libc in
 * the environment switches to the process's rand() -- then draws made by other code of the process (a FLANN matcher's
 * kd-trees, as in the reference's own process) count, and so do the ROCm runtime's.
 * sba_reference_rand_seed(1) puts the stream back into the never-seeded state (any seed: as srand(seed));
 * sba_reference_rand_next() draws one value, as rand() would.                                                    */
int sba_reference_rand_seed(unsigned int seed);
int sba_reference_rand_next(void);
/* Host-only (no device needed): the match indices the reference's `trials` trials draw for a problem of n matches --
 * random_array (spherical_bundle_adjuster.hpp:182-211: std::iota + std::random_shuffle) constructed once per trial, its
 * first sample_n = (int)(n * subset_fraction) entries used (spherical_bundle_adjuster.cpp:130-141).  indices:
 * int[trials][sample_n].  Draws (n - 1) values per trial from the stream above, in libstdc++'s order.  *sample_n_out
 * receives sample_n (pass indices = NULL to query it without drawing).                                          */
int sba_reference_trial_subsets(int n, int trials, double subset_fraction, int* indices, int* sample_n_out);
/* Device part: A^T A of the rows kron(left_i, right_i) over each trial's index list.  indices: int[trials][sample_n]
 * (host), every entry < n; moments: double[trials][45] (host; upper triangle, row-major a <= b).  Single-GPU problems
 * only (an index list addresses the resident shard).                                                           */
int sba_problem_epipolar_subset_moments(sba_problem* p, const int* indices, int trials, int sample_n, double* moments);
/* Both parts + the consensus: what initial_guess (.cpp:118-181) computes, from the subsets the reference itself would
 * draw.  At most SBA_REFERENCE_SAMPLING_MAX_N matches (the reference's problem sizes; larger problems use the group
 * sampling of sba_problem_initial_guess), at least 4 (sample_n >= 1).                                          */
#define SBA_REFERENCE_SAMPLING_MAX_N (1 << 20)
int sba_problem_initial_guess_reference(sba_problem* p, int trials, double subset_fraction, double rot_euler[3],
                                        double tran[3], int* num_candidates);

/* ---- batched per-pair solve (BASELINE config C5: many ERP pairs, each its own two-view problem) ------- */
/* The reference handles one image pair per process run (main/main.cpp:6-34); a batch holds `num_pairs`
 * independent problems on one GPU: pair g owns correspondences [offsets[g], offsets[g+1]) of the
 * concatenated arrays (same layouts as sba_problem_upload; offsets has num_pairs+1 entries, ragged and empty
 * pairs allowed).  ONE sweep launch evaluates every pair at its own (rot, tran) -- the per-pair sweep state and the
 * mapping of the reduced moments to normal equations are computed on the device as well; sba_batch_solve runs one LM per
 * pair in lock-step (same schedule as sba_problem_solve).  Pairs are independent, so across GPUs they are
 * simply split between processes -- no collective.                                                        */
typedef struct sba_batch sba_batch;
int sba_batch_create(sba_batch** out, int device, void* stream);
int sba_batch_destroy(sba_batch* b);
int sba_batch_set_kernel(sba_batch* b, int kind);
int sba_batch_upload(sba_batch* b, const double* left_xyz, const double* right_xyz, const double* d12,
                     const size_t* offsets, int num_pairs, int store);
/* Re-send only the per-match depths (same layout as the d12 of sba_batch_upload, which must have carried depths): the
 * counterpart of sba_problem_set_depths -- sba_batch_solve_depths / sba_batch_solve_problem refine the depths in place, the
 * coordinates stay resident.  (sba_batch_upload with unchanged offsets / store keeps every allocation too and only moves data.) */
int sba_batch_set_depths(sba_batch* b, const double* d12);
int sba_batch_size(const sba_batch* b, int* num_pairs, int* blocks_per_pair);
/* rot, tran: double[num_pairs][3]; d1, d2: double[num_pairs] uniform depths per pair (NULL = 1.0; ignored with
 * SBA_DEPTH_PER_MATCH); packs: double[num_pairs][SBA_PACK_SIZE].                                          */
int sba_batch_eval(sba_batch* b, int mode, int depth_mode, const double* rot, const double* tran,
                   const double* d1, const double* d2, double huber_delta, double* packs);
/* `steps` host-synchronous batched steps in a C loop (bench / tuning): wall-clock mean per step and its split into
 * host preparation of the per-pair R|t state, launch-to-result on the device, and host conversion of the packs.  */
int sba_batch_eval_timed(sba_batch* b, int mode, int depth_mode, const double* rot, const double* tran,
                         const double* d1, const double* d2, double huber_delta, int steps, double* packs,
                         double* mean_step_ms, double* mean_prepare_ms, double* mean_device_ms,
                         double* mean_convert_ms);
/* The batched sweep kernel alone, `repeat` launches with a HIP event between every two (as
 * sba_problem_eval_launch_times): launch_ms[i] = device time of launch i.  repeat <= 4096.                        */
int sba_batch_sweep_launch_times(sba_batch* b, int mode, int depth_mode, const double* rot, const double* tran,
                                 const double* d1, const double* d2, double huber_delta, int repeat, float* launch_ms);
/* The same measurement on the dominant kernel of the step this batch really runs: with one block per pair the whole
 * step is ONE launch (batch_step_kernel: per-pair state read from mapped host memory, sweep, fold, conversion, packs and
 * sequence word published to the host -- launched here exactly as a step launches it, only the host does not wait
 * between launches), otherwise the batched sweep kernel as above.  sba_batch_step_is_fused: 1 / 0 (negative =
 * error) -- which of the two it is (SBA_BATCH_FUSED_STEP=0 in the environment keeps the three-kernel chain).        */
int sba_batch_step_launch_times(sba_batch* b, int mode, int depth_mode, const double* rot, const double* tran,
                                const double* d1, const double* d2, double huber_delta, int repeat, float* launch_ms);
int sba_batch_step_is_fused(const sba_batch* b);
/* One Levenberg-Marquardt solve per pair (what sba_problem_solve does for one problem).  rot / tran are updated in place per
 * pair; summaries (sba_lm_summary[num_pairs]) and status (int[num_pairs], SBA_OK or SBA_ERR_NUMERIC per pair) may be NULL.
 * With one block per pair the solvers run on the device: one launch covers the first sweeps of every pair, pairs that need
 * more go on in per-iteration launches whose blocks are dealt out to the pairs still iterating (DESIGN.md section 3.5;
 * SBA_BATCH_DYNAMIC / SBA_BATCH_LM_FIRST_SWEEPS in INTEGRATION.md section 7).                                          */
int sba_batch_solve(sba_batch* b, int mode, int depth_mode, double* rot, double* tran, const double* d1,
                    const double* d2, const sba_lm_options* opt, sba_lm_summary* summaries, int* status);

/* The 8-point initial guess (initial_guess, spherical_bundle_adjuster.cpp:47-181) of every pair of the batch -- what running
 * the reference once per pair does first.  Device part: the 64 x 45 group moments of every pair in one launch (one block per
 * pair; group = (match index WITHIN the pair / 2) % 64, as sba_problem_epipolar_moments on that pair alone; the sums differ
 * from it in summation order only).  groups: double[num_pairs][64][45].                                              */
int sba_batch_epipolar_moments(sba_batch* b, double* groups);
/* Both parts: pair g's result is what sba_initial_guess_from_moments makes of pair g's moments with the same trials /
 * subset_fraction / seed.  rot_euler, tran: double[num_pairs][3] (R_vec_out, T_vec_out of the reference, per pair);
 * num_candidates (may be NULL): int[num_pairs]; status (may be NULL): int[num_pairs], SBA_OK or SBA_ERR_NUMERIC (no valid
 * rotation candidate: that pair's outputs are zeros).  Returns SBA_ERR_NUMERIC when any pair failed.                  */
int sba_batch_initial_guess(sba_batch* b, int trials, double subset_fraction, unsigned long long seed, double* rot_euler,
                            double* tran, int* num_candidates, int* status);

/* The reference's whole per-pair pipeline -- do_bundle_adjustment's initial values and solve_problem
 * (spherical_bundle_adjuster.cpp:302-331, :183-217) -- for EVERY pair of the batch: what running main/main.cpp once per ERP
 * pair computes after matching.  use_initial_guess != 0: the 8-point consensus guess (trials, subset_fraction, seed as
 * sba_batch_initial_guess), init_rot = -R_vec_out, init_tran = T_vec_out (.cpp:330-331); a pair without a valid candidate
 * keeps the caller's rot / tran and is reported in status.  use_initial_guess == 0: rot / tran are the start values (the
 * alternative the reference keeps in a comment, .cpp:328-329).  Then the d-only stage on the uploaded depths (lambda = c = 1,
 * .cpp:1057-1058), the rot-only and the tran-only stage with init_d[0][0], init_d[1][0] of the pair as the depths of every
 * match (.cpp:941-942, :998-999).  rot, tran: double[num_pairs][3], in (start values) / out (result).  All of the following
 * may be NULL: d12_out (refined depths, as sba_batch_solve_depths), d_uniform double[num_pairs][2] (the two depths the
 * last stages used), guess_candidates int[num_pairs], the three summary arrays [num_pairs], status int[num_pairs] (first
 * failing stage's code per pair).  Returns SBA_ERR_NUMERIC when any pair failed; the other pairs' results are valid.   */
int sba_batch_solve_problem(sba_batch* b, int use_initial_guess, int trials, double subset_fraction, unsigned long long seed,
                            double* rot, double* tran, const sba_lm_options* opt, double* d12_out, double* d_uniform,
                            int* guess_candidates, sba_lm_summary* depth_summaries, sba_lm_summary* rot_summaries,
                            sba_lm_summary* tran_summaries, int* status);

/* The d-only stage (spherical_bundle_adjuster.cpp:196-197, functor :1004-1063) for EVERY pair of the batch: what
 * sba_problem_solve_depths does for one problem, per pair -- its own trust region, projected line search and convergence;
 * the solvers run on the device: the block that owns a pair runs the pair's first passes in one launch, pairs that need more go
 * on in per-pass launches whose blocks are dealt out to the pairs still iterating (SBA_BATCH_DEPTH_FIRST_PASSES=0: the one launch
 * runs every pair to the end; SBA_BATCH_DEVICE_DEPTH=0: host solvers in lock-step, one launch per pass -- these two agree to the
 * bit, the default to 1e-9 with equal counts).  rot, tran: double[num_pairs][3] (frozen);
 * needs per-match depths uploaded (the initial values) and refines them on the device, so that a following
 * SBA_DEPTH_PER_MATCH sweep / solve sees them; d12_out (may be NULL): double[offsets[num_pairs]][2], indexed like the uploaded d12
 * (the reference then takes d12_out[offsets[g]][0] and d12_out[offsets[g] + 1][0] as the pair's uniform depths of the rot /
 * tran stages, .cpp:941-942).  summaries / status as sba_batch_solve.  One 512-thread block per pair: made for
 * batches of many pairs (config C5); a batch of a few huge pairs is served, but by as many CUs as it has pairs.      */
int sba_batch_solve_depths(sba_batch* b, const double* rot, const double* tran, double lambda, double c,
                           const sba_lm_options* opt, double* d12_out, sba_lm_summary* summaries, int* status);

/* The joint solve (sba_problem_eval_joint / sba_problem_solve_joint: the reference's joint functor, .cpp:843-889) for EVERY pair
 * of the batch, on the batch's resident planes.  rot, tran: double[num_pairs][3].  opt == NULL means the defaults with
 * tran_param = SBA_TRAN_SPHERE (the gauge), as for the single-problem entry points; an explicit SBA_TRAN_FREE runs the
 * functor as written.  A batch without per-match depths is refused with SBA_ERR_UNSUPPORTED, a poisoned handle and one that was
 * never uploaded as everywhere; SBA_PUBLISH=0 is refused with SBA_ERR_UNSUPPORTED as by sba_batch_solve_depths.  One 256-thread
 * block per pair (the reduce pass needs one wave per SIMD to itself): made for batches of many pairs; a batch of a few huge pairs
 * is served, but by as many CUs as it has pairs.  A pair's sums are formed in an order that depends on its own matches only:
 * its results are the same bits alone in a batch, among other pairs, and in either pair layout.
 * sba_batch_eval_joint: one reduce pass per pair at (rot[g], tran[g]) and the batch's depths, depth damping from `radius`
 * (> 0, +inf: none; otherwise SBA_ERR_INVALID_ARG); out: sba_joint_eq[num_pairs] -- pair g's equals sba_problem_eval_joint on
 * pair g alone up to the summation order; an empty pair gives a zero system.                                                */
int sba_batch_eval_joint(sba_batch* b, const double* rot, const double* tran, double radius, const sba_lm_options* opt,
                         sba_joint_eq* out);
/* sba_batch_solve_joint: one joint LM per pair from (rot[g], tran[g]) -- in / out -- and the batch's depths.  The refined depths
 * stay in the batch's depth planes (a following SBA_DEPTH_PER_MATCH eval, solve, residuals or compaction sees them) and are
 * copied to d12_out (may be NULL; indexed like the uploaded d12, as sba_batch_solve_depths).  summaries / status (may be NULL)
 * as sba_batch_solve: status[g] is SBA_OK or SBA_ERR_NUMERIC, the call returns SBA_ERR_NUMERIC when any pair failed and the
 * other pairs' results are valid.  A pair whose start is non-finite fails that way with its depths, rot and tran unchanged.
 * An empty pair terminates at once on the gradient test, rot / tran unchanged.  The solvers run on the device, the whole solve
 * is one launch (the block that owns a pair keeps the pair's solver in LDS; at most 2 * max_num_iterations + 2 passes per pair,
 * a pair that would need more is reported with SBA_ERR_NUMERIC).  SBA_BATCH_DEVICE_JOINT=0: host solvers in lock-step, one
 * launch per pass -- the two drivers agree to the bit.                                                                        */
int sba_batch_solve_joint(sba_batch* b, double* rot, double* tran, const sba_lm_options* opt, sba_lm_summary* summaries,
                          int* status, double* d12_out);

/* sba_batch_covariance_joint: the covariance of the joint problem (sba_problem_covariance_joint) for EVERY pair of the batch.
 * Pair g gets what sba_problem_covariance_joint computes on pair g alone at (rot[g], tran[g]) and the batch's resident depths,
 * up to the summation order: the same robustified, undamped problem, gauge projection, degeneracy rule and (+inf, +inf, 0) rows.
 * out: sba_joint_cov[num_pairs]; depth_cov (may be NULL: no depth phase): double[offsets[num_pairs]][3], indexed like the
 * uploaded d12 and like d12_out of sba_batch_solve_joint (pair g's match i at row offsets[g] + i, which is row
 * offsets[g] - offsets[0] + i of the batch's own rows); status (may be NULL): int[num_pairs].
 * opt == NULL: the defaults with tran_param = SBA_TRAN_SPHERE.
 * Whole-call refusals, decided before a device is touched: those of sba_batch_solve_joint; out == NULL with pairs present,
 * or min_sin2_parallax negative or NaN: SBA_ERR_INVALID_ARG.
 * Per pair -- the contract of sba_batch_solve_joint: a pair whose rot / tran is not finite, whose n_used < m (an empty pair
 * included), whose S is not finite or whose unit-diagonal projected S has a pivot not above m * DBL_EPSILON FAILS:
 * status[g] = SBA_ERR_NUMERIC, out[g].cov all NaN and its depth_cov rows NaN (not zero: a zero covariance reads as
 * certainty); cost, sum_w, n_used, n_degenerate are those of its reduce pass, dim = m, dof = n_used - m.  The call returns
 * SBA_ERR_NUMERIC when any pair failed; the other pairs' results are valid and the handle stays usable.
 * The batch is not touched (depth planes, scaling state, layout): a later solve, residuals or compaction returns the bits it
 * returns without this call.  One 256-thread block per pair runs the pair's whole covariance -- reduce pass, finish, depth pass
 * -- in one launch; the per-match array comes back in one copy.  A pair's sums depend on its own matches only: its results are
 * the same bits alone in a batch, among other pairs, and in either pair layout.  SBA_BATCH_DEVICE_COV=0: a reduce launch, the
 * finish on the host, a depth launch -- the two drivers agree to the bit.                                                     */
int sba_batch_covariance_joint(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                               double min_sin2_parallax, sba_joint_cov* out /* [num_pairs] */,
                               double* depth_cov /* double[offsets[num_pairs]][3] or NULL */, int* status /* [num_pairs] or NULL */);

/* ---- the batched structure: every pair's triangulated landmarks, their covariances and the cut ---- */
/* sba_batch_structure_joint: the triangulated structure of the joint problem (sba_problem_structure_joint) for EVERY pair of the
 * batch.  Pair g gets what sba_problem_structure_joint computes on pair g alone at (rot[g], tran[g]) and the batch's resident
 * depths, up to the summation order of its Sigma_c: per match the midpoint of the two ray ends in camera 2's frame, its 3 x 3
 * covariance (xx, yy, zz, xy, xz, yz) under the joint covariance and the score trace / X.X; a degenerate match keeps its xyz and
 * has the covariance row (+inf, +inf, +inf, 0, 0, 0) and the score +inf.
 * out: sba_joint_cov[num_pairs] and status (may be NULL): int[num_pairs] -- those of sba_batch_covariance_joint at the same
 * arguments, bit for bit.  xyz: double[offsets[num_pairs]][3], xyz_cov: double[offsets[num_pairs]][6], score:
 * double[offsets[num_pairs]], indexed like the uploaded d12 (pair g's match i at row offsets[g] + i; rows below offsets[0] are
 * not touched); each may be NULL, and an output that is not asked for costs nothing.
 * Whole-call refusals, decided before a device is touched: those of sba_batch_covariance_joint.
 * Per pair -- the contract of sba_batch_solve_joint: a pair without a covariance (see sba_batch_covariance_joint) has
 * status[g] = SBA_ERR_NUMERIC and NaN in every row of every output asked for, xyz included; the call returns SBA_ERR_NUMERIC
 * when any pair failed, the other pairs' results are valid and the handle stays usable.
 * Two launches on the batch's stream with no host wait between them: the reduce pass and finish of
 * sba_batch_covariance_joint (SBA_BATCH_DEVICE_COV=0: its lock-step sequence), then the structure pass over a grid of
 * (num_pairs, blocks per pair) blocks -- clamp(CUs / num_pairs, 1, 256-vector tiles of the largest pair) blocks per pair,
 * SBA_BATCH_STRUCTURE_BPP overrides; the bits do not depend on it, nor on the pair layout, nor on the other pairs.  The host
 * form stages the outputs asked for through a scratch of the handle; the batch (depth planes, scaling state, layout) is not
 * touched.                                                                                                                    */
int sba_batch_structure_joint(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                              double min_sin2_parallax, sba_joint_cov* out /* [num_pairs] */, double* xyz, double* xyz_cov,
                              double* score, int* status /* [num_pairs] or NULL */);
/* The same with the three destinations in DEVICE memory (the batch's device): arrays of total = offsets[num_pairs] - offsets[0]
 * rows, the batch's own rows (pair g's match i at row offsets[g] - offsets[0] + i), each 16-byte aligned (else
 * SBA_ERR_INVALID_ARG and nothing is written) or NULL.  Nothing but out and status crosses to the host.                         */
int sba_batch_structure_joint_device(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                                     double min_sin2_parallax, sba_joint_cov* out /* [num_pairs] */, double* xyz, double* xyz_cov,
                                     double* score, int* status /* [num_pairs] or NULL */);
/* sba_problem_structure_order_stats for every pair: values[g][j] = the ranks[g][j]-th smallest (0-based) of pair g's scores,
 * bit for bit an element of sba_batch_structure_joint's score rows of that pair; +inf sorts above every finite score.  ranks
 * and values: [num_pairs][num_ranks], num_ranks 1 ... 8, ranks[g][j] < n[g]; an empty pair takes no part.  A pair without a
 * covariance has NaN values and status[g] = SBA_ERR_NUMERIC (the call then returns SBA_ERR_NUMERIC, the other pairs' values
 * are valid).  Refused before a device is touched: what sba_batch_structure_joint refuses (there is no out), NULL ranks /
 * values, num_ranks out of range, a rank that is not below its pair's size.                                                   */
int sba_batch_structure_order_stats(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                                    double min_sin2_parallax, const size_t* ranks, int num_ranks, double* values,
                                    int* status /* [num_pairs] or NULL */);
/* threshold[g] = scale[g] * q_(rank[g]) of pair g's scores (one IEEE multiplication), then every pair keeps its rows with
 * score <= threshold[g] through the compaction of sba_batch_compact, whose post-condition holds word for word; degenerate
 * matches (+inf) stay only under a +inf threshold.  rank, scale, threshold, n_kept: [num_pairs]; kept_index (may be NULL) as
 * sba_batch_keep_below.  A pair without a covariance is NOT cut: it keeps every row (n_kept[g] = n[g]), its threshold is NaN
 * and status[g] = SBA_ERR_NUMERIC; the other pairs are cut and the call returns SBA_ERR_NUMERIC -- the handle is then what
 * sba_batch_compact with that mask leaves.  An empty pair takes no part (NaN, 0).  Refused before a device is touched: what
 * sba_batch_structure_order_stats refuses, NULL rank / scale / threshold / n_kept, a scale that is not finite or negative.     */
int sba_batch_structure_keep_below(sba_batch* b, const double* rot, const double* tran, const sba_lm_options* opt,
                                   double min_sin2_parallax, const size_t* rank, const double* scale, double* threshold,
                                   size_t* n_kept, long long* kept_index, int* status /* [num_pairs] or NULL */);

/* ---- single matches of a batch: residuals, inlier sets, compaction ---- */
/* Rows r = 0 .. total - 1 with total = offsets[num_pairs] - offsets[0] of the current layout; row r is the caller's row
 * offsets[0] + r.  rot, tran, d1, d2 as for sba_batch_eval (per pair; NULL depths mean 1.0; ignored with
 * SBA_DEPTH_PER_MATCH).  Every output may be NULL:
 *   e_xyz    double[total][3]   each match's residual, formed as the batched sweep forms it
 *   sq_norm  double[total]      s = e.e
 *   inlier   uint8[total]       !(s > huber_delta^2); all 1 when huber_delta <= 0; a NaN residual is an inlier
 *   n_inlier size_t[num_pairs]  inliers per pair: n[g] - n_inlier[g] equals SBA_PACK_NOUT of sba_batch_eval's pack g at the
 *                               same arguments                                                                           */
int sba_batch_residuals(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                        const double* d2, double huber_delta, double* e_xyz, double* sq_norm, unsigned char* inlier,
                        size_t* n_inlier);
/* Keep the rows with keep[r] != 0 (host array of total bytes; may be NULL when total is 0), in order; each pair keeps its
 * own rows and may become empty.  n_kept (size_t[num_pairs], not NULL) receives every pair's kept count, kept_index (may be
 * NULL; capacity total) the kept row numbers.  Afterwards the handle is what sba_batch_upload of the kept rows (coordinates,
 * and depths if the batch has them) with the same store and offsets = the exclusive scan of n_kept from 0 would build: same
 * pairs, layout, blocks per pair and plane contents, so every later call gives the same bits as on such a handle;
 * sba_batch_set_depths then takes the new row count and d12_out of the solves is indexed by the new rows.  Compacted on the
 * device, deterministic; the per-pair count is the one synchronous step.  On an error the handle may be left without pairs
 * (SBA_ERR_NOT_UPLOADED after).                                                                                       */
int sba_batch_compact(sba_batch* b, const unsigned char* keep, size_t* n_kept, long long* kept_index);
/* sba_batch_residuals' inlier flags, then sba_batch_compact with them as keep -- the flags never leave the device: only
 * the per-pair counts come back before the new layout (and the kept row numbers, if asked for).                        */
int sba_batch_keep_inliers(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                           const double* d2, double huber_delta, size_t* n_kept, long long* kept_index);
/* sba_problem_residual_order_stats for every pair at its own (rot, tran, d1, d2), all pairs in the same launches: pair g
 * selects among its own n[g] rows of sba_batch_residuals' sq_norm.  ranks and values: [num_pairs][num_ranks], ranks[g][j] <
 * n[g]; an empty pair takes no part, its ranks are not looked at and its values are NaN.  A pair's values do not depend on
 * the other pairs.  Replaces sba_batch_residuals(sq_norm) + one host partition per pair.                                */
int sba_batch_residual_order_stats(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                                   const double* d2, const size_t* ranks, int num_ranks, double* values);
/* threshold[g] = scale[g] * s_(rank[g]) of pair g (NaN for an empty pair), then every pair keeps its rows with
 * s <= threshold[g] (a NaN s is dropped) through the compaction of sba_batch_compact, whose post-condition holds word for
 * word.  Flags and thresholds stay on the device until the end: only the per-pair counts and thresholds come back (and the
 * kept row numbers, if asked for).  rank, scale, threshold, n_kept: [num_pairs].  Replaces sba_batch_residuals(sq_norm) +
 * host partitions + sba_batch_compact with a host-built mask.                                                          */
int sba_batch_keep_below(sba_batch* b, int depth_mode, const double* rot, const double* tran, const double* d1,
                         const double* d2, const size_t* rank, const double* scale, double* threshold, size_t* n_kept,
                         long long* kept_index);

/* ---- callers / data formats either side of the path ------------------------------------- */
/* pixel -> unit sphere (spherical_bundle_adjuster.cpp:271-298).  keypoints: n records of
 * `stride_bytes` bytes whose first two floats are pt.x, pt.y (cv::KeyPoint: stride 28).
 * out_xyz: double[3n] host array (cv::Point3d layout).                                       */
int sba_keypoints_to_sphere(int device, const void* keypoints, size_t n, size_t stride_bytes,
                            int im_width, int im_height, double* out_xyz);

/* The four maps below end in a decision on an f64 expression of sin/cos/acos/atan2 -- an integer pixel index by
 * truncation, or a float32 by rounding.  The device computes every output and marks the few whose f64 value lies within
 * 1e-6 pixel of such a decision boundary (at pitch -90 whole pixel lines sit exactly on one); those are finished on the
 * host by the same source function compiled against the host C library, the one the reference runs on.  Results are
 * therefore bit-identical to the reference's arithmetic, not merely within a pixel.  The *_device forms take device
 * pointers and a HIP stream (NULL = the default stream); they synchronise that stream once (to read the list of
 * marked outputs) -- the image forms only the first time a geometry is seen, its source-index table is cached.     */

/* ERP -> cubemap strip (equi2cube.cpp:12-302).  erp: H x W x 3 bytes (8UC3, row-major, host).
 * out: cube_size x (6*cube_size) x 3 bytes, face order left,front,right,back,top,bottom
 * (equi2cube.cpp:292-298).  Source indices are clamped into the image (the reference does not
 * clamp, equi2cube.cpp:47-50; it can only differ at the exact pole).                        */
int sba_equi2cube(int device, const uint8_t* erp, int im_height, int im_width, int cube_size,
                  uint8_t* out);
/* Batched, device-resident form: erp_dev = batch x H x W x 3 bytes, out_dev = batch x S x 6S x 3
 * bytes, both on `device`; enqueued on `stream`.                                                 */
int sba_equi2cube_device(int device, void* stream, const void* erp_dev, int im_height, int im_width,
                         int cube_size, int batch, void* out_dev);

/* ---- key-point / image maps of the matchers (what turns matcher output into the BA path's input) ------ */
/* spherical_surf::rotate_keypoint (spherical_surf.cpp:110-123): in place on n records of stride_bytes whose
 * first two floats are pt.x, pt.y (band coordinates); adds the band offset H*3/8, rotates by the pitch angle
 * through rotate_pixel (:48-74) with the reference's integer truncations, writes ERP pixel coordinates back. */
int sba_rotate_keypoints(int device, void* keypoints, size_t n, size_t stride_bytes, float pitch_deg,
                         int im_width, int im_height);
int sba_rotate_keypoints_device(int device, void* stream, void* keypoints_dev, size_t n, size_t stride_bytes,
                                float pitch_deg, int im_width, int im_height);
/* equi2cube_surf::cube2equi_pixel (equi2cube_surf.cpp:19-76): in place, cube-strip pixel -> ERP pixel.       */
int sba_cube2equi_keypoints(int device, void* keypoints, size_t n, size_t stride_bytes, int cube_size,
                            int im_width, int im_height);
int sba_cube2equi_keypoints_device(int device, void* stream, void* keypoints_dev, size_t n, size_t stride_bytes,
                                   int cube_size, int im_width, int im_height);
/* spherical_surf::crop_rotated_image (spherical_surf.cpp:76-108): erp H x W x 3 bytes -> out (H/4) x W x 3,
 * the equatorial band of the image rotated by pitch_deg (inverse warping); pixels whose source falls outside
 * the image are 0 (the reference leaves them uninitialised).                                               */
int sba_crop_rotated_image(int device, const uint8_t* erp, int im_height, int im_width, float pitch_deg,
                           uint8_t* out);
/* Batched, device-resident form: erp_dev = batch x H x W x 3, out_dev = batch x (H/4) x W x 3.               */
int sba_crop_rotated_image_device(int device, void* stream, const void* erp_dev, int im_height, int im_width,
                                  float pitch_deg, int batch, void* out_dev);
/* Diagnostics: number of outputs of the cached source-index table that were decided on the host; -1 if that table has
 * not been built.  kind 0 = equi2cube (param = cube_size), 1 = crop (param = the bit pattern of the float pitch).   */
long sba_map_table_host_decided(int device, int kind, int param, int im_height, int im_width);
/* The tiled form of that table, which the gather kernel stages through LDS: number of 32 x 32 output tiles, how many of
 * them are staged (the rest gather from global memory), LDS bytes per frame.  0, or -1 if the table is not built.      */
int sba_map_table_tiles(int device, int kind, int param, int im_height, int im_width, int* tiles, int* staged_tiles,
                        int* lds_bytes_per_frame);

/* ---- descriptor matching (feature_matcher::match_two_image, feature_matcher.cpp:42-59) -------------------------- */
/* Exact L2 2-nearest neighbours of every query row among the train rows, then the reference's ratio test
 * d0 < ratio * d1 (0.3 there), in float on the reported distances.  Descriptors: f32 rows of `dim` values
 * (1 <= dim <= 256; SURF 64, extended SURF 128), `row_stride_bytes` apart (a multiple of 4, >= 4 * dim: a cv::Mat
 * passes as Mat::ptr<float>() and Mat::step).  Query = the left image (queryIdx), train = the right (trainIdx).
 *   nn_index / nn_dist  [n_query][2] (NULL = not wanted): the two neighbours, nearest first, and their Euclidean
 *                       distances (DMatch::distance); -1 and +inf where there is none.
 *   n_matched           the accepted queries; match_query / match_train / match_dist (capacity n_query each, NULL =
 *                       not wanted): the accepted (queryIdx, trainIdx, distance) in ascending query order -- the
 *                       reference's good_matches.
 * Ranking is lexicographic on (score, train index) -- the lowest index wins a tie; the two winners are rescored as
 * sum_k (q_k - t_k)^2 in f32 and reordered by (distance, index).  The result of a query is a pure function of the query row,
 * the train rows, dim and ratio.  A query row with a non-finite component matches nothing; a train row with one is never
 * chosen; with fewer than two train rows nothing matches (the reference reads knn_matches[i][1] then: undefined behaviour).
 * Deviation: OpenCV's FlannBasedMatcher (randomised kd-trees) is approximate; this is the exact answer it approximates.
 * The count is the one synchronous step.                                                                            */
int sba_match_descriptors(int device, const float* query, size_t n_query, const float* train, size_t n_train, int dim,
                          size_t row_stride_bytes, float ratio, int* nn_index, float* nn_dist, size_t* n_matched,
                          int* match_query, int* match_train, float* match_dist);
/* The same on device pointers and a HIP stream (NULL = the default stream); every output array is a device array.      */
int sba_match_descriptors_device(int device, void* stream, const float* query_dev, size_t n_query, const float* train_dev,
                                 size_t n_train, int dim, size_t row_stride_bytes, float ratio, int* nn_index_dev,
                                 float* nn_dist_dev, size_t* n_matched, int* match_query_dev, int* match_train_dev,
                                 float* match_dist_dev);
/* Many pairs in one launch: pair g matches query rows query_offsets[g] .. [g + 1] against train rows train_offsets[g] ..
 * [g + 1] (non-decreasing; empty pairs allowed).  Indices are local to the pair; nn_* are indexed by query row -
 * query_offsets[0]; n_matched[num_pairs]; the match_* arrays hold pair 0's matches, then pair 1's, ...              */
int sba_batch_match_descriptors(int device, const float* query, const size_t* query_offsets, const float* train,
                                const size_t* train_offsets, int num_pairs, int dim, size_t row_stride_bytes, float ratio,
                                int* nn_index, float* nn_dist, size_t* n_matched, int* match_query, int* match_train,
                                float* match_dist);
/* Match, then upload the matched key-points: afterwards the handle equals sba_problem_upload_keypoints() of the records
 * left_keypoints[match_left[i]], right_keypoints[match_right[i]] (i < *n_matched), with d12 = (d, d) per match when
 * init_depth points at a depth d (the reference's init_d fill, spherical_bundle_adjuster.cpp:325-326).  Key-point records
 * as sba_problem_upload_keypoints; descriptors as sba_match_descriptors, one row per key-point.  The gather runs on the
 * device: only the count and the indices (match_left / match_right, capacity n_left, NULL = not wanted) come back. */
int sba_problem_upload_matches(sba_problem* p, const void* left_keypoints, size_t n_left, const void* right_keypoints,
                               size_t n_right, size_t stride_bytes, int im_width, int im_height, const float* left_desc,
                               const float* right_desc, int dim, size_t row_stride_bytes, float ratio, const double* init_depth,
                               int store, size_t* n_matched, int* match_left, int* match_right);
/* The same for every pair of a batch (offsets as sba_batch_match_descriptors, for key-points and descriptors alike):
 * afterwards the batch equals sba_batch_upload() of sba_keypoints_to_sphere() of the matched records with offsets = the
 * exclusive scan of n_matched[num_pairs], and d12 = (init_depth[g], init_depth[g]) for the matches of pair g when
 * init_depth (double[num_pairs]) is given.  match_left / match_right: pair-local indices, concatenated in pair order.  */
int sba_batch_upload_matches(sba_batch* b, const void* left_keypoints, const size_t* left_offsets, const void* right_keypoints,
                             const size_t* right_offsets, int num_pairs, size_t stride_bytes, int im_width, int im_height,
                             const float* left_desc, const float* right_desc, int dim, size_t row_stride_bytes, float ratio,
                             const double* init_depth, int store, size_t* n_matched, int* match_left, int* match_right);

#ifdef __cplusplus
}
#endif
#endif /* SBA_HIP_H_ */
