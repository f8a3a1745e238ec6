// Command-line driver with the reference's argument contract (main/main.cpp:8-27):
//   sba_main [--joint [--covariance] [--structure FILE]] [--reject Q,SCALE] <L> <R> <exp roll> <exp pitch> <exp yaw> <exp Tx> <exp Ty> <exp Tz> <exp d>
// --joint (anywhere on the line; not in the reference): refine depths, rotation and translation together after the
// tran-only stage (spherical_bundle_adjuster::set_joint_refinement).  Without it the run is the reference's three stages.
// --covariance (only together with --joint; not in the reference): after the joint stage print one more line, the 1-sigma of
// the rotation vector (degrees) and of the translation from the joint problem's covariance (set_joint_covariance).
// --structure FILE (only together with --joint; not in the reference): after the joint stage write the triangulated landmarks as
// an ASCII PLY, one vertex "x y z q" per match: the point in camera 2's frame and its uncertainty score (set_structure_output).
// --reject Q,SCALE (not in the reference): after the last stage drop the matches whose squared residual norm exceeds SCALE
// times its Q quantile, run the stages once more on the rest and report the cut (set_outlier_rejection).
// With OpenCV (SBA_WITH_OPENCV) <L>/<R> are ERP images and a matcher must be linked in by the
// integrator.  Without OpenCV <L>/<R> are files of cv::KeyPoint records (28 bytes
// each) preceded by a 16-byte header {int32 count, int32 im_width, int32 im_height, int32 dim}:
//   dim == 0  the records are matched already (same count, match i = record i);
//   dim > 0   count x dim f32 descriptors (row-major) follow the records; the two files may hold
//             different counts and are matched first (feature_matcher::match_two_image: exact
//             2-NN on the device, ratio test 0.3), both files with the same dim.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <thread>

#include "spherical_bundle_adjuster.hpp"

namespace {
bool read_keypoints(const char* path, std::vector<cv::KeyPoint>* out, std::vector<float>* desc, int* w, int* h, int* dim) {
  std::ifstream f(path, std::ios::binary);
  int32_t hdr[4];
  if (!f.read(reinterpret_cast<char*>(hdr), sizeof(hdr)) || hdr[0] < 0 || hdr[3] < 0) return false;
  out->resize(static_cast<size_t>(hdr[0]));
  *w = hdr[1];
  *h = hdr[2];
  *dim = hdr[3];
  if (hdr[0] > 0 && !f.read(reinterpret_cast<char*>(out->data()), sizeof(cv::KeyPoint) * out->size())) return false;
  desc->resize(out->size() * static_cast<size_t>(hdr[3]));
  return desc->empty() || static_cast<bool>(f.read(reinterpret_cast<char*>(desc->data()), sizeof(float) * desc->size()));
}
}  // namespace

int main(int argc, char** argv) {
  bool joint = false, covariance = false, reject = false;
  double reject_q = 0.0, reject_scale = 0.0;
  const char* structure = nullptr;
  {
    int kept = 1;
    for (int i = 1; i < argc; ++i) {
      if (std::strcmp(argv[i], "--joint") == 0) joint = true;
      else if (std::strcmp(argv[i], "--covariance") == 0) covariance = true;
      else if (std::strcmp(argv[i], "--structure") == 0 && i + 1 < argc) structure = argv[++i];
      else if (std::strcmp(argv[i], "--reject") == 0 && i + 1 < argc &&
               std::sscanf(argv[i + 1], "%lf,%lf", &reject_q, &reject_scale) == 2) { reject = true; ++i; }
      else argv[kept++] = argv[i];
    }
    argc = kept;
  }
  if (argc != 10 || (covariance && !joint) || (structure && !joint)) {
    if (covariance && !joint) std::cout << "--covariance needs --joint" << std::endl;
    if (structure && !joint) std::cout << "--structure needs --joint" << std::endl;
    std::cout << "usage : spherical_bundle_adjuster.out <L image> <R image> <exp roll> <exp pitch> <exp yaw> "
                 "<exp Tx> <exp Ty> <exp Tz> <exp d>" << std::endl;
    return 0;   // the reference returns 0 on a usage error too (main/main.cpp:11)
  }
  spherical_bundle_adjuster sph_ba(atof(argv[3]), atof(argv[4]), atof(argv[5]), atof(argv[6]), atof(argv[7]),
                                   atof(argv[8]), atof(argv[9]));
  sph_ba.set_omp(static_cast<int>(std::max(1u, std::thread::hardware_concurrency())));   // omp_get_num_procs(), main/main.cpp:31
  // SBA_INITIAL_GUESS=0: start from the expected values on the command line instead of the 8-point consensus
  if (const char* env = std::getenv("SBA_INITIAL_GUESS")) sph_ba.set_initial_guess(env[0] != '0');
  sph_ba.set_joint_refinement(joint);
  sph_ba.set_joint_covariance(covariance);
  if (structure) sph_ba.set_structure_output(structure);
  if (reject) sph_ba.set_outlier_rejection(reject_q, reject_scale);
  std::vector<cv::KeyPoint> left_key, right_key;
  std::vector<float> left_desc, right_desc;
  int w = 0, h = 0, w2 = 0, h2 = 0, dim = 0, dim2 = 0;
  if (!read_keypoints(argv[1], &left_key, &left_desc, &w, &h, &dim) ||
      !read_keypoints(argv[2], &right_key, &right_desc, &w2, &h2, &dim2) || dim != dim2 ||
      (dim == 0 && left_key.size() != right_key.size()) || w != w2 || h != h2) {
    std::cerr << "cannot read key-point files" << std::endl;
    return 1;
  }
  const int rc = dim > 0 ? sph_ba.do_bundle_adjustment_from_features(left_key, right_key, left_desc, right_desc, dim, w, h)
                         : sph_ba.do_bundle_adjustment_from_matches(left_key, right_key, static_cast<int>(left_key.size()), w, h);
  if (rc != SBA_OK) {
    std::cerr << "error " << rc << ": " << sba_last_error() << std::endl;
    return 2;
  }
  return 0;
}
