// TEST INFRASTRUCTURE (oracle/ref_build only).  ceres::AngleAxisRotatePoint is NOT in the reference's tree: the reference calls
// it (spherical_bundle_adjuster.cpp:857, :908, :965, :1019) and Ceres supplies it.  This is OUR restatement of what Ceres'
// documentation says the function computes -- Rodrigues' formula on the unit axis when theta^2 exceeds the double epsilon,
// pt + angle_axis x pt below it -- in the order of operations the documented formula reads in.  It is therefore one of the two
// stated edges of what "pinned by the reference's compiled code" means (the other: oracle/reference_shuffle.cpp pins the shuffle to
// libstdc++).  Everything around the call -- the functor bodies, which depths and which pose reach it, the loss, the bounds -- is
// the reference's own text, compiled unchanged.
#pragma once
#include <cmath>
#include <limits>

#include "ceres/ceres.h"

namespace ceres {

template <typename T> inline void AngleAxisRotatePoint(const T angle_axis[3], const T pt[3], T result[3]) {
  using std::cos;
  using std::sin;
  using std::sqrt;
  const T theta2 = angle_axis[0] * angle_axis[0] + angle_axis[1] * angle_axis[1] + angle_axis[2] * angle_axis[2];
  if (theta2 > T(std::numeric_limits<double>::epsilon())) {
    const T theta = sqrt(theta2);
    const T costheta = cos(theta);
    const T sintheta = sin(theta);
    const T theta_inverse = T(1.0) / theta;
    const T w[3] = {angle_axis[0] * theta_inverse, angle_axis[1] * theta_inverse, angle_axis[2] * theta_inverse};
    const T w_cross_pt[3] = {w[1] * pt[2] - w[2] * pt[1], w[2] * pt[0] - w[0] * pt[2], w[0] * pt[1] - w[1] * pt[0]};
    const T tmp = (w[0] * pt[0] + w[1] * pt[1] + w[2] * pt[2]) * (T(1.0) - costheta);
    result[0] = pt[0] * costheta + w_cross_pt[0] * sintheta + w[0] * tmp;
    result[1] = pt[1] * costheta + w_cross_pt[1] * sintheta + w[1] * tmp;
    result[2] = pt[2] * costheta + w_cross_pt[2] * sintheta + w[2] * tmp;
  } else {
    const T w_cross_pt[3] = {angle_axis[1] * pt[2] - angle_axis[2] * pt[1], angle_axis[2] * pt[0] - angle_axis[0] * pt[2],
                             angle_axis[0] * pt[1] - angle_axis[1] * pt[0]};
    result[0] = pt[0] + w_cross_pt[0];
    result[1] = pt[1] + w_cross_pt[1];
    result[2] = pt[2] + w_cross_pt[2];
  }
}

}  // namespace ceres
