// TEST INFRASTRUCTURE: C entry point onto the reference's public equi2cube_surf::cube2equi_pixel (equi2cube_surf.cpp, compiled
// unchanged next to this file).
#include <cstddef>

#include "equi2cube_surf.hpp"

extern "C" {

// n (x, y) float pairs in the 6 cube x cube strip -> (x, y) in the im_w x im_h equirectangular image
void ref_cube2equi_pixels(const float* xy_in, size_t n, int cube, int im_w, int im_h, float* xy_out) {
  equi2cube_surf s;
  for (size_t i = 0; i < n; ++i) {
    cv::Point2f in(xy_in[2 * i], xy_in[2 * i + 1]), out;
    s.cube2equi_pixel(in, out, cube, im_w, im_h);
    xy_out[2 * i] = out.x;
    xy_out[2 * i + 1] = out.y;
  }
}

}  // extern "C"
