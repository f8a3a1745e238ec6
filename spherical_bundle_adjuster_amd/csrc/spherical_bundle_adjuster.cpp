// See spherical_bundle_adjuster.hpp.  Stage order, frozen blocks, the init_d[0][0]/init_d[1][0] quirk,
// the printed lines and the log.txt row follow the reference (spherical_bundle_adjuster.cpp:183-217,
// :255-357); every numeric step goes through the C-ABI in include/sba_hip.h (HIP kernels + host LM).
#include "spherical_bundle_adjuster.hpp"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>

namespace {
constexpr double kPi = 3.14159265358979323846;
}

spherical_bundle_adjuster::~spherical_bundle_adjuster() {
  if (problem) sba_problem_destroy(problem);
}

void spherical_bundle_adjuster::set_omp(int n) {
  // The reference sets the process-global OpenMP thread count (.cpp:835-841) for its CPU loops and for
  // Ceres.  The GPU path has no host loops over matches; the one host loop worth threads is the 80 trials of the
  // initial guess, which run on that many host threads (the result does not depend on the count).
  num_proc = n;
  if (n >= 1) sba_set_host_threads(n);
  std::cout << "Number of process: " << num_proc << std::endl;
}

void spherical_bundle_adjuster::do_bundle_adjustment(const cv::Mat& im_left, const cv::Mat& im_right) {
  std::vector<cv::KeyPoint> left_key, right_key;
  int match_size = 0, total_key_num = 0;
  cv::Mat match_output;
  std::cout << "Do feature finding and matching" << std::endl;                         // .cpp:262
  if (matcher) {
    matcher(im_left, im_right, left_key, right_key, match_size, match_output, total_key_num);
  } else {
#ifdef SBA_WITH_OPENCV
    spherical_surf fm;                                                                  // .cpp:264-266, verbatim
    fm.set_omp(this->num_proc);
    fm.do_all(im_left, im_right, left_key, right_key, match_size, match_output, total_key_num);
#else
    std::cerr << "spherical_bundle_adjuster: built without OpenCV, so the reference's default matcher "
                 "(spherical_surf, SURF/FLANN) is not available: call set_matcher() or use "
                 "do_bundle_adjustment_from_matches()" << std::endl;
    return;
#endif
  }
  const int rc = do_bundle_adjustment_from_matches(left_key, right_key, match_size, im_left.cols, im_left.rows);
  if (rc != SBA_OK) std::cerr << "spherical_bundle_adjuster: " << sba_last_error() << std::endl;
}

int spherical_bundle_adjuster::do_bundle_adjustment_from_features(const std::vector<cv::KeyPoint>& left_kp,
                                                                  const std::vector<cv::KeyPoint>& right_kp,
                                                                  const std::vector<float>& left_desc,
                                                                  const std::vector<float>& right_desc, int dim, int im_width,
                                                                  int im_height) {
  if (dim < 1 || left_desc.size() != left_kp.size() * static_cast<size_t>(dim) ||
      right_desc.size() != right_kp.size() * static_cast<size_t>(dim))
    return SBA_ERR_INVALID_ARG;
  std::vector<int> query(left_kp.size()), train(left_kp.size());
  size_t n = 0;
  int rc = sba_match_descriptors(device, left_desc.data(), left_kp.size(), right_desc.data(), right_kp.size(), dim,
                                 sizeof(float) * static_cast<size_t>(dim), 0.3f, nullptr, nullptr, &n, query.data(), train.data(),
                                 nullptr);
  if (rc) return rc;
  std::cout << "matched : " << n << std::endl;
  std::vector<cv::KeyPoint> valid_key_left(n), valid_key_right(n);       // feature_matcher.cpp:105-110
  for (size_t i = 0; i < n; ++i) {
    valid_key_left[i] = left_kp[query[i]];
    valid_key_right[i] = right_kp[train[i]];
  }
  return do_bundle_adjustment_from_matches(valid_key_left, valid_key_right, static_cast<int>(n), im_width, im_height);
}

int spherical_bundle_adjuster::do_bundle_adjustment_from_matches(const std::vector<cv::KeyPoint>& left_key,
                                                                 const std::vector<cv::KeyPoint>& right_key,
                                                                 int match_size, int im_width, int im_height) {
  if (match_size < 0 || static_cast<size_t>(match_size) > left_key.size() ||
      static_cast<size_t>(match_size) > right_key.size())
    return SBA_ERR_INVALID_ARG;
  std::cout << "Do bundle adjustment" << std::endl;                                     // .cpp:300
  // pixel -> radian -> unit vector (.cpp:271-298) runs on the device and writes the coordinate planes directly:
  // the matched key-points go to the device once, the cv::Point3d arrays of the reference are never materialised on
  // the host, and the initial guess and all three solve stages work on that one resident copy.
  if (!problem) {
    int rc0 = sba_problem_create(&problem, device, nullptr);
    if (rc0) return rc0;
  }
  int rc = sba_problem_upload_keypoints(problem, left_key.data(), right_key.data(), static_cast<size_t>(match_size),
                                        sizeof(cv::KeyPoint), im_width, im_height, nullptr, SBA_STORE_F64);
  if (rc) return rc;
  std::vector<cv::Point3d> key_point_left_rect, key_point_right_rect;   // stay empty: the data is resident
  resident_left = &key_point_left_rect;
  resident_n = match_size;

  // Initial values (.cpp:302-331).  Default: the 8-point consensus (initial_guess, .cpp:304), then
  // init_rot = -Euler(R_vec_out) and init_tran = T_vec_out exactly like .cpp:330-331 -- including the reference's
  // use of the negated Euler triple as an angle-axis vector.  set_initial_guess(false) starts from the expected
  // values given on the command line instead, the alternative the reference keeps in a comment (.cpp:328-329).
  std::vector<std::array<double, 2>> init_d(match_size);
  for (auto& d : init_d) d = {expected_d, expected_d};                                   // .cpp:325-326
  double init_rot[3] = {expected_roll / 180 * kPi, expected_pitch / 180 * kPi, expected_yaw / 180 * kPi};
  double init_tran[3] = {expected_tx, expected_ty, expected_tz};
  if (use_initial_guess) {
    std::cout << "E matrix estimation with SVD" << std::endl;                           // .cpp:127
    double euler[3], tvec[3];
    int candidates = 0;
    guess_sampling_t how = guess_sampling;
    if (const char* env = std::getenv("SBA_GUESS_SAMPLING")) {
      if (std::strcmp(env, "groups") == 0) how = GUESS_GROUPS;
      else if (std::strcmp(env, "reference") == 0) how = GUESS_REFERENCE;
    }
    if (how == GUESS_AUTO) how = (match_size >= 4 && match_size <= kReferenceSamplingMaxN) ? GUESS_REFERENCE : GUESS_GROUPS;
    if (how == GUESS_REFERENCE)   // 80 x random_array(match_size), int(match_size * 0.25) matches each: .cpp:130-141
      rc = sba_problem_initial_guess_reference(problem, 80, 0.25, euler, tvec, &candidates);
    else
      rc = sba_problem_initial_guess(problem, 80, 0.25, guess_seed, euler, tvec, &candidates);
    if (rc) return rc;
    for (int i = 0; i < 3; ++i) { init_rot[i] = -euler[i]; init_tran[i] = tvec[i]; }     // .cpp:330-331
    res.guess_candidates = candidates;
  }

  sba_lm_options options;
  sba_lm_options_default(&options);
  options.max_num_iterations = 50;   // .cpp:336
  options.verbose = 1;               // minimizer_progress_to_stdout, .cpp:337

  rc = solve_problem(options, key_point_left_rect, key_point_right_rect, init_rot, init_tran, init_d, match_size);
  resident_left = nullptr;
  resident_n = -1;
  if (rc) return rc;

  for (int i = 0; i < 3; ++i) { res.rot[i] = init_rot[i]; res.tran[i] = init_tran[i]; }
  res.match_size = match_size;
  // log.txt row, same columns as .cpp:348-354
  std::ofstream log_file(log_path, std::ios_base::app);
  log_file << expected_roll << ',' << expected_pitch << ',' << expected_yaw << ','
           << init_rot[0] / kPi * 180.0 << ',' << init_rot[1] / kPi * 180.0 << ',' << init_rot[2] / kPi * 180.0 << ','
           << init_tran[0] << ',' << init_tran[1] << ',' << init_tran[2] << ',' << match_size << std::endl;
  // write_d_circle (.cpp:227-252, :356) draws into an image: outside the accelerated path.  write_log_d (.cpp:357):
  if (!depth_log_name.empty()) write_log_d(init_d, depth_log_name);
  std::cout << "Done." << std::endl;
  return SBA_OK;
}

void spherical_bundle_adjuster::write_log_d(const std::vector<std::array<double, 2>>& init_d,
                                            const std::string& name) const {
  std::ofstream log_d_file(name + ".txt", std::ios_base::app);
  for (const auto& d : init_d) log_d_file << d[0] << ',' << d[1] << '\n';
}

int spherical_bundle_adjuster::solve_problem(sba_lm_options& opt, std::vector<cv::Point3d>& key_point_left_rect,
                                             std::vector<cv::Point3d>& key_point_right_rect, double* init_rot,
                                             double* init_tran, std::vector<std::array<double, 2>>& init_d,
                                             int match_num) {
  int rc;
  if (!problem) {
    rc = sba_problem_create(&problem, device, nullptr);
    if (rc) return rc;
  }
  // One flat upload replaces the per-match `new AutoDiffCostFunction / new HuberLoss` of the four
  // add_residual loops (.cpp:870-889, :921-945, :978-1002, :1034-1063).  When do_bundle_adjustment_from_matches
  // already made these coordinates resident, only the depths (init_d) are sent.
  if (resident_left == &key_point_left_rect && resident_n == match_num && match_num > 0) {
    rc = sba_problem_set_depths(problem, reinterpret_cast<const double*>(init_d.data()));
  } else {
    if (key_point_left_rect.size() < static_cast<size_t>(match_num) ||
        key_point_right_rect.size() < static_cast<size_t>(match_num) || init_d.size() < static_cast<size_t>(match_num))
      return SBA_ERR_INVALID_ARG;
    rc = sba_problem_upload(problem, reinterpret_cast<const double*>(key_point_left_rect.data()),
                            reinterpret_cast<const double*>(key_point_right_rect.data()),
                            match_num > 0 ? reinterpret_cast<const double*>(init_d.data()) : nullptr,
                            static_cast<size_t>(match_num), SBA_STORE_F64);
  }
  if (rc) return rc;

  auto report = [](const char* stage, const sba_lm_summary& s) {
    std::printf("%s: iterations %d, initial cost %.6e, final cost %.6e, termination %d, %.3f ms (%.3f ms in sweeps)\n",
                stage, s.num_iterations, s.initial_cost, s.final_cost, s.termination, s.seconds_total * 1e3,
                s.seconds_eval * 1e3);
  };

  auto run_stages = [&](int num) -> int {
    // stage 1: d-only (.cpp:196-197) -- per-match bounded depth refinement, lambda = c = 1 (.cpp:1057-1058)
    if (num > 0) {
      rc = sba_problem_solve_depths(problem, init_rot, init_tran, 1.0, 1.0, &opt,
                                    reinterpret_cast<double*>(init_d.data()), &res.depth_stage);
      if (rc) return rc;
      report("d-only", res.depth_stage);
    }
    // stages 2 and 3 use init_d[0][0] and init_d[1][0] for EVERY match (.cpp:941-942, :998-999)
    const double d1 = num > 0 ? init_d[0][0] : 0.0;
    const double d2 = num > 1 ? init_d[1][0] : d1;

    rc = sba_problem_solve(problem, SBA_MODE_ROT, SBA_DEPTH_UNIFORM, init_rot, init_tran, d1, d2, &opt, &res.rot_stage);   // .cpp:202-203
    if (rc) return rc;
    report("rot-only", res.rot_stage);
    rc = sba_problem_solve(problem, SBA_MODE_TRAN, SBA_DEPTH_UNIFORM, init_rot, init_tran, d1, d2, &opt, &res.tran_stage); // .cpp:208-209
    if (rc) return rc;
    report("tran-only", res.tran_stage);

    // optional stage 4 (set_joint_refinement): depths, rotation and translation together, from the staged result.  The
    // handle still holds the d-only stage's depths; the sphere parameterisation keeps |tran| at its current length.
    res.joint_stage = sba_lm_summary{};
    if (joint_refinement && num > 0) {
      sba_lm_options jopt = opt;
      jopt.tran_param = SBA_TRAN_SPHERE;
      rc = sba_problem_solve_joint(problem, init_rot, init_tran, &jopt, &res.joint_stage, reinterpret_cast<double*>(init_d.data()));
      if (rc) return rc;
      report("joint", res.joint_stage);
      // optional (set_joint_covariance): how far to trust that pose -- the joint problem's covariance at it, scaled by the
      // residual variance the fit suggests.  A rank-deficient scene has none: that is reported, not an error of the run.
      if (joint_covariance) {
        sba_joint_cov cov;
        rc = sba_problem_covariance_joint(problem, init_rot, init_tran, &jopt, 0.0, &cov, nullptr);
        if (rc == SBA_ERR_NUMERIC) {
          std::printf("joint covariance: none (%s)\n", sba_last_error());
        } else if (rc) {
          return rc;
        } else {
          const double s2 = cov.dof > 0 ? 2.0 * cov.cost / cov.dof : 0.0;
          double sd[6];
          for (int a = 0; a < 6; ++a) sd[a] = std::sqrt(s2 * cov.cov[7 * a]);
          std::printf("joint covariance: 1-sigma rot (deg) %.6e %.6e %.6e, tran %.6e %.6e %.6e (sigma^2 = 2 cost / dof = %.6e, "
                      "%lld used, %lld degenerate)\n", sd[0] / kPi * 180.0, sd[1] / kPi * 180.0, sd[2] / kPi * 180.0, sd[3], sd[4], sd[5],
                      s2, cov.n_used, cov.n_degenerate);
        }
      }
      // optional (set_structure_output): what the joint solve leaves behind as structure -- one landmark per match with
      // its uncertainty score, as an ASCII PLY.  A rank-deficient scene has no covariance, hence no score: reported, no file.
      if (!structure_path.empty()) {
        std::vector<double> xyz(3 * static_cast<size_t>(num)), score(static_cast<size_t>(num));
        sba_joint_cov cov;
        rc = sba_problem_structure_joint(problem, init_rot, init_tran, &jopt, 0.0, &cov, xyz.data(), nullptr, score.data());
        if (rc == SBA_ERR_NUMERIC) {
          std::printf("joint structure: none (%s)\n", sba_last_error());
        } else if (rc) {
          return rc;
        } else {
          const double s2 = cov.dof > 0 ? 2.0 * cov.cost / cov.dof : 0.0;
          std::FILE* f = std::fopen(structure_path.c_str(), "w");
          if (!f) {
            std::printf("joint structure: cannot write %s\n", structure_path.c_str());
          } else {
            std::fprintf(f, "ply\nformat ascii 1.0\ncomment landmarks in the frame of camera 2; q = sigma^2 trace(cov) / |xyz|^2\n"
                            "element vertex %d\nproperty double x\nproperty double y\nproperty double z\nproperty double q\nend_header\n", num);
            for (int i = 0; i < num; ++i)
              std::fprintf(f, "%.17g %.17g %.17g %.17g\n", xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], s2 * score[i]);
            std::fclose(f);
            std::printf("joint structure: %d landmarks to %s (sigma^2 = %.6e, %lld degenerate)\n", num, structure_path.c_str(), s2,
                        cov.n_degenerate);
          }
        }
      }
    }
    return SBA_OK;
  };
  rc = run_stages(match_num);
  if (rc) return rc;

  // optional (set_outlier_rejection): the matches whose squared residual norm at the pose and depths reached lies above
  // scale * (its `quantile` order statistic) leave the handle -- selected, flagged and compacted on the device
  // (sba_problem_keep_below) -- and the same stages run once more on the rest, from the pose reached.
  res.kept_size = match_num;
  res.reject_threshold = 0.0;
  if (reject_quantile >= 0.0 && match_num > 0) {
    const size_t rank = static_cast<size_t>(std::floor(reject_quantile * static_cast<double>(match_num - 1)));
    std::vector<long long> kept_index(static_cast<size_t>(match_num));
    size_t kept = 0;
    rc = sba_problem_keep_below(problem, SBA_DEPTH_PER_MATCH, init_rot, init_tran, 1.0, 1.0, rank, reject_scale,
                                &res.reject_threshold, &kept, kept_index.data());
    if (rc) return rc;
    resident_left = nullptr;   // the handle no longer holds every match of the caller's arrays
    resident_n = -1;
    for (size_t k = 0; k < kept; ++k) init_d[k] = init_d[static_cast<size_t>(kept_index[k])];
    init_d.resize(kept);
    res.kept_size = static_cast<int>(kept);
    std::printf("outlier rejection: threshold %.6e, kept %zu / %d\n", res.reject_threshold, kept, match_num);
    rc = run_stages(static_cast<int>(kept));
    if (rc) return rc;
  }

  std::cout << "expected rotation vector " << expected_roll << ' ' << expected_pitch << ' ' << expected_yaw << ' ' << std::endl;
  std::cout << "rotation vector in degree " << init_rot[0] / kPi * 180.0 << ' ' << init_rot[1] / kPi * 180.0 << ' '
            << init_rot[2] / kPi * 180.0 << std::endl;
  std::cout << "translation vector " << init_tran[0] << ' ' << init_tran[1] << ' ' << init_tran[2] << std::endl;
  return SBA_OK;
}
