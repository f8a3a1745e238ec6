// TEST INFRASTRUCTURE: C entry point onto the reference's equi2cube::get_all (equi2cube.cpp, compiled unchanged next to this file).
#include <cstdint>
#include <cstring>

#include "equi2cube.hpp"

extern "C" {

// The reference's own get_all on an "index image": pixel i of the im_h x im_w image holds i in its three bytes (little endian), so
// the cubemap it returns IS the source-index table.  table: cube x 6 cube int32.  The stand-in Mat's padded row (row == im_h) is
// filled with 0xff, so a pixel for which the reference reads one row past the image comes back as an index >= im_h * im_w
// (0xffffff); their number is returned.
long ref_equi2cube_table(int im_h, int im_w, int cube, int32_t* table) {
  cv::Mat im(im_h, im_w, CV_8UC3);
  const size_t n = static_cast<size_t>(im_h) * im_w;
  for (size_t i = 0; i < n; ++i) {
    im.data[3 * i + 0] = static_cast<unsigned char>(i & 0xff);
    im.data[3 * i + 1] = static_cast<unsigned char>((i >> 8) & 0xff);
    im.data[3 * i + 2] = static_cast<unsigned char>((i >> 16) & 0xff);
  }
  std::memset(im.data + 3 * n, 0xff, 3 * static_cast<size_t>(im_w) + 3);
  equi2cube e;
  cv::Mat out = e.get_all(im, cube);
  long beyond = 0;
  const size_t m = static_cast<size_t>(cube) * 6 * cube;
  for (size_t i = 0; i < m; ++i) {
    const int32_t v = out.data[3 * i] | (out.data[3 * i + 1] << 8) | (out.data[3 * i + 2] << 16);
    table[i] = v;
    if (static_cast<size_t>(v) >= n) ++beyond;
  }
  return beyond;
}

}  // extern "C"
