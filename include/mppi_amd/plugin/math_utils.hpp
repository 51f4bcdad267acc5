/**
 * math_utils.hpp — small helpers with the reference's names (reference: include/mppi/utils/math_utils.h:15-110, 149-156,
 * 166-283 and 534-540 for the quaternion helpers, 738-747).
 */
#ifndef MPPI_AMD_PLUGIN_MATH_UTILS_HPP_
#define MPPI_AMD_PLUGIN_MATH_UTILS_HPP_

#include <hip/hip_runtime.h>
#include "mppi_amd/det_math.h"

#ifndef SQ
#define SQ(a) ((a) * (a))
#endif

namespace mppi
{
namespace math
{
/** reference: utils/math_utils.h nearest_multiple_4 */
inline __host__ __device__ int nearest_multiple_4(const int& a)
{
  return ((a + 3) / 4) * 4;
}
inline __host__ __device__ int int_ceil(const int& a, const int& b)
{
  return a == 0 ? a : (a - 1) / b + 1;
}
inline __host__ __device__ float clamp(float value, float min, float max)
{
  return fminf(fmaxf(value, min), max);
}
/** reference: utils/math_utils.h:744-747 — the float overload the dynamics base class resolves to */
inline __host__ __device__ float sign(float value)
{
  return value >= 0 ? 1 : -1;
}
/** reference: utils/math_utils.h:90-94 */
inline __host__ __device__ float linInterp(const float x, const float x_min, const float x_max, const float y_min,
                                           const float y_max)
{
  return (x - x_min) / (x_max - x_min) * (y_max - y_min) + y_min;
}
/** |r - centre line| in units of half the track width (reference: utils/math_utils.h:149-156) */
inline __host__ __device__ float normDistFromCenter(const float r, const float r_in, const float r_out)
{
  const float r_center = (r_in + r_out) / 2.0f;
  const float r_width = r_out - r_in;
  return fabsf(r - r_center) / (r_width * 0.5f);
}
/** reference: utils/math_utils.h:45 */
constexpr float GRAVITY = 9.81f;

/* ---- quaternions (w, x, y, z) as float arrays; rotations in the NWU frame (reference: utils/math_utils.h:166-283, 534-540) ----
 * The reference evaluates these with rsqrtf / atan2f / asinf on the device and 1 / sqrtf on the host.  One flavour here, the
 * same on the MI355X and on a CPU: the norm is det::sqrt followed by a true division, the angles are det::atan2 and det::asin,
 * and every sum keeps the reference's left-to-right order. */
namespace detail
{
/** 1 / |q| with the four squares added in index order */
inline __host__ __device__ float quatInvNorm(const float q[4])
{
  return 1.0f / mppi::det::sqrt(SQ(q[0]) + SQ(q[1]) + SQ(q[2]) + SQ(q[3]));
}
}  // namespace detail

/** q_3 = q_1 x q_2 (Hamilton product), scaled to unit length unless normalize is false (math_utils.h:166-186) */
inline __host__ __device__ void QuatMultiply(const float q_1[4], const float q_2[4], float q_3[4], bool normalize = true)
{
  const float w1 = q_1[0], x1 = q_1[1], y1 = q_1[2], z1 = q_1[3];
  const float w2 = q_2[0], x2 = q_2[1], y2 = q_2[2], z2 = q_2[3];
  q_3[0] = w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2;
  q_3[1] = x1 * w2 + w1 * x2 - z1 * y2 + y1 * z2;
  q_3[2] = y1 * w2 + z1 * x2 + w1 * y2 - x1 * z2;
  q_3[3] = z1 * w2 - y1 * x2 + x1 * y2 + w1 * z2;
  if (normalize)
  {
    const float inv_norm = detail::quatInvNorm(q_3);
#pragma unroll
    for (int i = 0; i < 4; i++)
      q_3[i] *= inv_norm;
  }
}

/** the conjugate over the norm (math_utils.h:188-199) */
inline __host__ __device__ void QuatInv(const float q[4], float q_inv[4])
{
  const float inv_norm = detail::quatInvNorm(q);
  q_inv[0] = q[0] * inv_norm;
#pragma unroll
  for (int i = 1; i < 4; i++)
    q_inv[i] = -q[i] * inv_norm;
}

/** the rotation that takes q_1 to q_2: q_3 = q_2 x q_1^-1 (math_utils.h:206-211) */
inline __host__ __device__ void QuatSubtract(const float q_1[4], const float q_2[4], float q_3[4])
{
  float q_1_inv[4];
  QuatInv(q_1, q_1_inv);
  QuatMultiply(q_2, q_1_inv, q_3);
}

/** roll, pitch, yaw of the 3-2-1 sequence from body to world (math_utils.h:263-270); the pitch argument is clamped to
 *  [-1, 1] before the arcsine, as there */
inline __host__ __device__ void Quat2EulerNWU(const float q[4], float& r, float& p, float& y)
{
  const float w = q[0], x = q[1], yy = q[2], z = q[3];
  r = mppi::det::atan2(2.0f * z * yy + 2.0f * w * x, w * w + z * z - yy * yy - x * x);
  const float sin_pitch = -2.0f * w * yy + 2.0f * x * z;
  p = -mppi::det::asin(fmaxf(fminf(1.0f, sin_pitch), -1.0f));
  y = mppi::det::atan2(2.0f * yy * x + 2.0f * z * w, w * w + x * x - yy * yy - z * z);
}

/** third column of Quat2DCM's matrix: the body z axis in the world frame, all a thrust along body z needs */
inline __host__ __device__ void Quat2DCMColumn3(const float q[4], float col[3])
{
  col[0] = 2 * (q[1] * q[3] + q[0] * q[2]);
  col[1] = 2 * (q[2] * q[3] - q[0] * q[1]);
  col[2] = SQ(q[0]) - SQ(q[1]) - SQ(q[2]) + SQ(q[3]);
}

/** direction cosine matrix, body to world (math_utils.h:272-283) */
inline __host__ __device__ void Quat2DCM(const float q[4], float M[3][3])
{
  float col3[3];
  Quat2DCMColumn3(q, col3);
  M[0][0] = SQ(q[0]) + SQ(q[1]) - SQ(q[2]) - SQ(q[3]);
  M[0][1] = 2 * (q[1] * q[2] - q[0] * q[3]);
  M[0][2] = col3[0];
  M[1][0] = 2 * (q[1] * q[2] + q[0] * q[3]);
  M[1][1] = SQ(q[0]) - SQ(q[1]) + SQ(q[2]) - SQ(q[3]);
  M[1][2] = col3[1];
  M[2][0] = 2 * (q[1] * q[3] - q[0] * q[2]);
  M[2][1] = 2 * (q[2] * q[3] + q[0] * q[1]);
  M[2][2] = col3[2];
}

/** quaternion rate of the body rates (p, q, r): ed = 1/2 e x (0, p, q, r) (math_utils.h:534-540) */
inline __host__ __device__ void omega2edot(const float p, const float q, const float r, const float e[4], float ed[4])
{
  ed[0] = 0.5f * (-p * e[1] - q * e[2] - r * e[3]);
  ed[1] = 0.5f * (p * e[0] - q * e[3] + r * e[2]);
  ed[2] = 0.5f * (p * e[3] + q * e[0] - r * e[1]);
  ed[3] = 0.5f * (-p * e[2] + q * e[1] + r * e[0]);
}
}  // namespace math
}  // namespace mppi

/** reference: include/mppi/utils/angle_utils.cuh:21-27; evaluated with the bit-reproducible fmod of det_math.h */
namespace angle_utils
{
__host__ __device__ static inline float normalizeAngle(float angle)
{
  return mppi::det::normalizeAngle(angle);
}
/** the same value for |angle| < 1e7 rad, without the out-of-range test on the dependent chain (det_math.h) */
__host__ __device__ static inline float normalizeAngleBounded(float angle)
{
  return mppi::det::normalizeAngleBounded(angle);
}
__host__ __device__ static inline float shortestAngularDistance(float from, float to)
{
  return normalizeAngle(to - from);
}
}  // namespace angle_utils

#endif
