// Host and device share of the landmark map's descriptors and of the association of a frame with the map (include/sba_hip.h:
// sba_landmarks_set_descriptors / _get_descriptors / _append_described / _associate): the claim key and its order, and the
// option, row and size checks of the entry points.  HIP-free; the kernels are in sba_landmarks_associate.hip, the entry points
// in sba_landmarks.cpp.  DESIGN.md section 3.28.
//
// The rule.  The matcher of section 3.10 runs with the frame rows as queries and the map's rows as train rows; frame row j gets
// (i0, d0), (i1, d1) and is ACCEPTED iff i1 >= 0, d0 < ratio * d1 in float and d0 <= max_distance in float.  Landmark i's
// claimants are the accepted rows with i0 == i; its winner is the claimant smallest in (bits of d0 as u32, j), compared
// lexicographically.  d0 >= 0, so the bit order is the value order, and among equal distances the lowest frame row wins.  The
// two halves are one u64 key, (bits(d0) << 32) | j, and the winner is the minimum of integers: it does not depend on the order
// in which the claimants arrive.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "sba_rotation.hpp"

namespace sba {

// What a landmark's slot holds while nobody has claimed it.  No key equals it: row 0xffffffff does not exist (m < 2^31).
constexpr unsigned long long kAssociateUnclaimed = ~0ull;

SBA_HD inline unsigned int associate_float_bits(float d) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(d);
#else
  unsigned int u;
  std::memcpy(&u, &d, sizeof(u));
  return u;
#endif
}
SBA_HD inline float associate_bits_float(unsigned int u) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(u);
#else
  float d;
  std::memcpy(&d, &u, sizeof(d));
  return d;
#endif
}

// The key of frame row `row` at distance d0 (>= 0, not NaN), and its two halves back.
SBA_HD inline unsigned long long associate_key(float d0, unsigned int row) {
  return (static_cast<unsigned long long>(associate_float_bits(d0)) << 32) | static_cast<unsigned long long>(row);
}
SBA_HD inline unsigned int associate_key_row(unsigned long long key) { return static_cast<unsigned int>(key & 0xffffffffull); }
SBA_HD inline float associate_key_distance(unsigned long long key) { return associate_bits_float(static_cast<unsigned int>(key >> 32)); }
// a wins over b: smaller in (bits of d0, row).
SBA_HD inline bool associate_key_before(unsigned long long a, unsigned long long b) { return a < b; }
// The distance cut of an accepted row: inclusive, false for a NaN distance.
SBA_HD inline bool associate_within(float d0, float max_distance) { return d0 <= max_distance; }

// Option, row and size checks of the entry points: nullptr = fine, otherwise what is wrong (SBA_ERR_INVALID_ARG).
inline const char* associate_check_options(float ratio, float max_distance) {
  if (!std::isfinite(ratio) || !(ratio > 0.f)) return "ratio must be finite and > 0";
  if (!(max_distance > 0.f)) return "max_distance must be > 0 (+inf: no cut)";
  return nullptr;
}
// Descriptor rows as sba_match_descriptors takes them: 1 <= dim <= 256, a stride that is a multiple of 4 and >= 4 dim.
inline const char* descriptor_check_rows(int dim, size_t row_stride_bytes) {
  if (dim < 1 || dim > 256) return "descriptor dimension out of range [1, 256]";
  if (row_stride_bytes % 4 != 0 || row_stride_bytes < 4 * static_cast<size_t>(dim)) return "row_stride_bytes must be a multiple of 4 and >= 4 * dim";
  return nullptr;
}
// The matcher counts rows in 32 bits and a key holds the frame row in 32.
inline const char* associate_check_sizes(size_t n, size_t m_frame) {
  const size_t limit = static_cast<size_t>(1) << 31;
  return n < limit && m_frame < limit ? nullptr : "the map and the frame must have fewer than 2^31 rows";
}

}  // namespace sba
