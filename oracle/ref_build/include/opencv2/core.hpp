// TEST INFRASTRUCTURE (oracle/ref_build only): a small WORKING stand-in for the OpenCV types and functions that four of the
// reference's translation units name (equi2cube.cpp, spherical_surf.cpp, equi2cube_surf.cpp, spherical_bundle_adjuster.cpp), so
// that those files compile unchanged without OpenCV.  Written for this project; none of it is OpenCV's text.
//
// What works, because the pinned functions run it: Mat allocation, copy (shared buffer), at<T>(), Mat_<T>(r, c) << a, b, ...,
// the product of two double matrices, hconcat, Vec, Point, KeyPoint.  Everything else is declared and never defined: the
// library is loaded lazily and the code paths that would call it (do_all, initial_guess, eight_point_estimation, ...) are never run.
//
// Three choices here are OURS, not OpenCV's, and the fixtures inherit them:
//   * Mat zero-fills its buffer (cv::Mat leaves it uninitialised), so "a pixel the reference does not write is 0" is this file's
//     doing -- crop_rotated_image's skipped pixels come out 0 for that reason only.
//   * Mat allocates one padded row (and one element) past rows * cols.  equi2cube.cpp reads row == rows where theta == pi; with
//     the pad that read is defined, and a shim can mark the pad so the read is recognisable.
//   * operator*(Mat, Mat) sums k = 0, 1, 2 in ascending order.  OpenCV's gemm may order the sum differently; for the pitch-only
//     rotations the fixtures use (R_x = R_z = I) every term is multiplied by an exact 0 or 1, so the product is exact in any order.
#pragma once
#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <memory>
#include <numeric>
#include <string>
#include <vector>

#define CV_8UC3 16
#define CV_32SC2 12
#define CV_64FC1 6
typedef long long int64;

namespace cv {
typedef std::string String;

template <typename T> struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T a, T b) : x(a), y(b) {}
};
typedef Point_<float> Point2f;
typedef Point_<double> Point2d;
template <typename T> struct Point3_ {
  T x, y, z;
  Point3_() : x(0), y(0), z(0) {}
  Point3_(T a, T b, T c) : x(a), y(b), z(c) {}
};
typedef Point3_<double> Point3d;

template <typename T, int N> struct Vec {
  T val[N];
  Vec() { for (int i = 0; i < N; ++i) val[i] = T(0); }
  Vec(T a, T b) { static_assert(N == 2, "two components"); val[0] = a; val[1] = b; }
  Vec(T a, T b, T c) { static_assert(N == 3, "three components"); val[0] = a; val[1] = b; val[2] = c; }
  T& operator[](int i) { return val[i]; }
  const T& operator[](int i) const { return val[i]; }
};
template <typename T, int N> Vec<T, N> operator-(const Vec<T, N>& a, const Vec<T, N>& b) {
  Vec<T, N> r;
  for (int i = 0; i < N; ++i) r.val[i] = a.val[i] - b.val[i];
  return r;
}
typedef Vec<unsigned char, 3> Vec3b;
typedef Vec<int, 2> Vec2i;
typedef Vec<float, 3> Vec3f;
typedef Vec<double, 2> Vec2d;
typedef Vec<double, 3> Vec3d;

struct Scalar {
  double val[4];
  Scalar(double a = 0, double b = 0, double c = 0, double d = 0) { val[0] = a; val[1] = b; val[2] = c; val[3] = d; }
};
struct Rect {
  int x, y, width, height;
  Rect(int x_, int y_, int w, int h) : x(x_), y(y_), width(w), height(h) {}
};
struct KeyPoint {
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
  KeyPoint() : size(0), angle(-1), response(0), octave(0), class_id(-1) {}
};
struct DMatch {
  int queryIdx, trainIdx, imgIdx;
  float distance;
  DMatch() : queryIdx(-1), trainIdx(-1), imgIdx(-1), distance(0) {}
};
static_assert(sizeof(KeyPoint) == 28 && sizeof(Point3d) == 24, "the layouts the product's C ABI takes");

inline size_t standin_elem_size(int type) { return type == CV_8UC3 ? 3 : 8; }   // CV_32SC2 and CV_64FC1: 8 bytes

struct Mat {
  int rows, cols;
  unsigned char* data;
  Mat() : rows(0), cols(0), data(nullptr), type_(0) {}
  Mat(int r, int c, int type) : rows(r), cols(c), type_(type) {
    // zero-filled, one padded row and one element beyond rows * cols (see the header of this file)
    buf_ = std::make_shared<std::vector<unsigned char>>((static_cast<size_t>(r + 1) * c + 1) * standin_elem_size(type), 0);
    data = buf_->data();
  }
  int type() const { return type_; }
  bool empty() const { return data == nullptr; }
  size_t elemSize() const { return standin_elem_size(type_); }
  template <typename T> T& at(int i, int j) { return reinterpret_cast<T*>(data)[static_cast<size_t>(i) * cols + j]; }
  template <typename T> const T& at(int i, int j) const { return reinterpret_cast<const T*>(data)[static_cast<size_t>(i) * cols + j]; }
  // declared only (never run)
  Mat row(int i) const;
  Mat inv() const;
  Mat clone() const;
  Mat operator()(const Rect& roi) const;

 private:
  int type_;
  std::shared_ptr<std::vector<unsigned char>> buf_;
};

template <typename T> struct DataType;
template <> struct DataType<double> { enum { type = CV_64FC1 }; };
template <> struct DataType<Vec2i> { enum { type = CV_32SC2 }; };
template <typename T> struct Mat_ : Mat {
  Mat_() {}
  Mat_(int r, int c) : Mat(r, c, DataType<T>::type) {}
};
typedef Mat_<Vec2i> Mat2i;

// Mat_<T>(r, c) << a, b, c, ... : fills row-major, converts to Mat
template <typename T> struct MatCommaInitializer_ {
  Mat_<T> m;
  size_t k;
  template <typename U> MatCommaInitializer_& operator,(U v) {
    reinterpret_cast<T*>(m.data)[k++] = static_cast<T>(v);
    return *this;
  }
  operator Mat() const { return m; }
  operator Mat_<T>() const { return m; }
};
template <typename T, typename U> MatCommaInitializer_<T> operator<<(const Mat_<T>& m, U v) {
  MatCommaInitializer_<T> init{m, 0};
  return (init, v);
}

// product of two CV_64FC1 matrices; k ascending (our order, see the header of this file)
inline Mat operator*(const Mat& a, const Mat& b) {
  Mat c(a.rows, b.cols, CV_64FC1);
  for (int i = 0; i < a.rows; ++i)
    for (int j = 0; j < b.cols; ++j) {
      double acc = a.at<double>(i, 0) * b.at<double>(0, j);
      for (int k = 1; k < a.cols; ++k) acc += a.at<double>(i, k) * b.at<double>(k, j);
      c.at<double>(i, j) = acc;
    }
  return c;
}

inline void hconcat(const std::vector<Mat>& src, Mat& dst) {
  int cols = 0;
  for (const Mat& m : src) cols += m.cols;
  Mat out(src.empty() ? 0 : src[0].rows, cols, src.empty() ? CV_8UC3 : src[0].type());
  const size_t es = out.elemSize();
  int at = 0;
  for (const Mat& m : src) {
    for (int i = 0; i < m.rows; ++i)
      std::memcpy(out.data + (static_cast<size_t>(i) * cols + at) * es, m.data + static_cast<size_t>(i) * m.cols * es, m.cols * es);
    at += m.cols;
  }
  dst = out;
}

// declared only (never run)
template <typename T> struct Ptr {
  T* p = nullptr;
  T* operator->() const { return p; }
};
struct Feature2D {};
struct DescriptorMatcher {};
void vconcat(const Mat* src, size_t n, Mat& dst);
void SVDecomp(const Mat& src, Mat& w, Mat& u, Mat& vt, int flags = 0);
void decomposeEssentialMat(const Mat& E, Mat& R1, Mat& R2, Mat& t);
void circle(Mat& img, Point2f center, int radius, const Scalar& color, int thickness = 1);
bool imwrite(const String& name, const Mat& img);
int64 getTickCount();
double getTickFrequency();
}  // namespace cv
