// TEST INFRASTRUCTURE: C entry points onto the reference's spherical_surf (spherical_surf.cpp, compiled unchanged next to this
// file): eular2rot, rotate_pixel, and the private crop_rotated_image and rotate_keypoint.  do_all is compiled and linked, never called.
//
// Two things the fixtures made here inherit from oracle/ref_build/include/opencv2/core.hpp, not from OpenCV:
//   * eular2rot's R_z * R_y * R_x runs through the stand-in's matrix product, whose summation order is ours.  Every call below
//     passes a pitch-only rotation (R_x = R_z = I): each term of the product is then multiplied by an exact 0 or 1, and the result
//     is exact in any order.
//   * crop_rotated_image skips pixels whose source falls outside the image; they read 0 because the stand-in Mat zero-fills.
#include <cstdint>
#include <cstring>
#include <vector>

#include "opencv2/core.hpp"
#include <omp.h>
#include <functional>
#include <iostream>
#include <set>
#include <sstream>
#include <utility>

// this translation unit opens the class: crop_rotated_image and rotate_keypoint are private
#define private public
#include "spherical_surf.hpp"
#undef private

extern "C" {

// eular2rot(Vec3f(0, RAD(pitch_deg), 0)) as crop_rotated_image and rotate_keypoint build it: R (9 doubles, row-major)
void ref_pitch_rotation(float pitch_deg, double* R) {
  spherical_surf s;
  cv::Mat m = s.eular2rot(cv::Vec3f(0, RAD(pitch_deg), 0));
  std::memcpy(R, m.data, 9 * sizeof(double));
}

// rotate_pixel on n (row, col) pairs under the pitch-only rotation
void ref_rotate_pixels(float pitch_deg, const int32_t* rc_in, size_t n, int width, int height, int32_t* rc_out) {
  spherical_surf s;
  cv::Mat m = s.eular2rot(cv::Vec3f(0, RAD(pitch_deg), 0));
  for (size_t i = 0; i < n; ++i) {
    const cv::Vec2i v = s.rotate_pixel(cv::Vec2i(rc_in[2 * i], rc_in[2 * i + 1]), m, width, height);
    rc_out[2 * i] = v[0];
    rc_out[2 * i + 1] = v[1];
  }
}

// crop_rotated_image on a caller's im_h x im_w 8UC3 image: out is (im_h / 4) x im_w x 3 bytes
void ref_crop_rotated_image(const uint8_t* im, int im_h, int im_w, float pitch_deg, uint8_t* out) {
  cv::Mat src(im_h, im_w, CV_8UC3);
  std::memcpy(src.data, im, static_cast<size_t>(im_h) * im_w * 3);
  spherical_surf s;
  cv::Mat o = s.crop_rotated_image(pitch_deg, src);
  std::memcpy(out, o.data, static_cast<size_t>(im_h / 4) * im_w * 3);
}

// rotate_keypoint in place on n (x, y) float pairs
void ref_rotate_keypoints(float* xy, size_t n, float pitch_deg, int width, int height) {
  std::vector<cv::KeyPoint> key(n);
  for (size_t i = 0; i < n; ++i) key[i].pt = cv::Point2f(xy[2 * i], xy[2 * i + 1]);
  spherical_surf s;
  s.rotate_keypoint(pitch_deg, key, width, height);
  for (size_t i = 0; i < n; ++i) { xy[2 * i] = key[i].pt.x; xy[2 * i + 1] = key[i].pt.y; }
}

}  // extern "C"
