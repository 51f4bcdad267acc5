/**
 * three_d_texture_helper.hpp — generic 3-D map lookup for Dynamics / Cost plugins (a stack of elevation or occupancy layers, a
 * clearance volume, a time-indexed cost map): world pose -> map frame -> normalised texture coordinate -> trilinear (or
 * nearest) sample with clamp or border addressing per axis, and wrap addressing along z.
 *
 * Replaces the reference's ThreeDTextureHelper (include/mppi/utils/texture_helpers/three_d_texture_helper.cuh,
 * three_d_texture_helper.cu:135-282 the query, :28-130 updateTexture, :285-390 setExtent / copyDataToGPU; the transforms are its
 * base class's, texture_helper.cu:94-133, 270-289).  The reference samples with the CUDA texture unit (tex3D) on the device and
 * with an fp32 formula on the host.  As in two_d_texture_helper.hpp there is no image path here: queryTexture() evaluates the
 * reference's HOST formula in fp32, operation for operation, on the device too, so device, host and the tests' restatement
 * agree bit for bit.
 *
 * Layout: texel (layer z, row y, column x) of texture i at data[((z * height + y) * width + x) * NC + ch], NC channels per
 * texel (1 or 4: float / float4).  float3 arguments are plain float[3].  ThreeDTextureHelper is a POD that travels as a kernel
 * argument like every other plugin member; ThreeDTextureHelperHost (below) is the host side that owns the values.
 *
 * Behaviours of the reference's host formula that are KEPT:
 *   - the coordinate is un-normalised by the extent and moved by -0.5 (values sit at the cell centres);
 *   - addressing is per axis: clamp, border, and — on z only — wrap with the period depth - 1 (NOT depth);
 *   - the border test is `q > extent - 1 || q <= 0`: a coordinate of exactly 0 is border;
 *   - linear filtering takes min(floor(q), extent - 2) per axis and interpolates along x, then y, then z, each blend written
 *     `a * (1 - d) + b * d`;
 *   - point filtering rounds each axis (round half away from zero).
 * What differs, on purpose:
 *   - wrap on x or y makes the reference's host path throw; it is refused on the host when the parameters are set
 *     (ThreeDTextureHelperHost::updateAddressMode, mppi_texture3d_query) and never reaches a kernel.  A block that carries it
 *     anyway is sampled as clamp;
 *   - an axis of one texel reads texel 0 twice with d = 0 (the reference reads index -1);
 *   - a NaN coordinate samples texel 0 (the reference converts floor(NaN) to an int);
 *   - the z wrap is a closed form, not the reference's two `while` loops (wrapZ() shows that the values are the same).
 */
#ifndef MPPI_AMD_THREE_D_TEXTURE_HELPER_HPP_
#define MPPI_AMD_THREE_D_TEXTURE_HELPER_HPP_

#include <math.h>
#include <string.h>

#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "mppi_amd/det_math.h"
#include "mppi_amd/utils/texture_helpers/two_d_texture_helper.hpp"
#if defined(__HIPCC__)
#include "mppi_amd/engine/hip_owned.hpp"
#endif

namespace mppi
{
namespace texture
{
/** cudaAddressModeWrap; z axis of a 3-D texture only (AddressMode of two_d_texture_helper.hpp has clamp and border) */
constexpr int ADDRESS_WRAP = 2;

/** TextureParams2D (two_d_texture_helper.hpp) with a depth and a third address mode */
struct TextureParams3D
{
  const float* data = nullptr;  ///< [depth][height][width][NC], device (or host, for the host-side call) pointer
  int width = 0, height = 0, depth = 0;
  int use = 0;  ///< checkTextureUse()
  int address_mode[3] = { ADDRESS_CLAMP, ADDRESS_CLAMP, ADDRESS_CLAMP };
  int filter_mode = FILTER_LINEAR;
  float border_color[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
  float origin[3] = { 0.0f, 0.0f, 0.0f };
  float rotations[9] = { 1.0f, 0.0f, 0.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 1.0f };  ///< row-major 3x3
  float resolution[3] = { 1.0f, 1.0f, 1.0f };                                     ///< metres per texel
};

template <int NUM_TEXTURES, int NC = 1>
struct ThreeDTextureHelper
{
  static_assert(NC == 1 || NC == 4, "a texel is a float or a float4");
  static constexpr int CHANNELS = NC;
  TextureParams3D textures_[NUM_TEXTURES];

  MPPI_TEX_HD inline bool checkTextureUse(const int index) const
  {
    return textures_[index].use != 0;
  }

  /** texture_helper.cu:94-104 */
  MPPI_TEX_HD inline void worldPoseToMapPose(const int index, const float* input, float* output) const
  {
    const TextureParams3D& p = textures_[index];
    const float dx = input[0] - p.origin[0], dy = input[1] - p.origin[1], dz = input[2] - p.origin[2];
    const float* R = p.rotations;
    output[0] = R[0] * dx + R[1] * dy + R[2] * dz;
    output[1] = R[3] * dx + R[4] * dy + R[5] * dz;
    output[2] = R[6] * dx + R[7] * dy + R[8] * dz;
  }

  /** texture_helper.cu:106-124: metres -> texels -> normalised coordinate, z by the depth as well */
  MPPI_TEX_HD inline void mapPoseToTexCoord(const int index, const float* input, float* output) const
  {
    const TextureParams3D& p = textures_[index];
    output[0] = (input[0] / p.resolution[0]) / (float)p.width;
    output[1] = (input[1] / p.resolution[1]) / (float)p.height;
    output[2] = (input[2] / p.resolution[2]) / (float)p.depth;
  }

  /**
   * three_d_texture_helper.cu:211-221, the z wrap:  while (q > P) q -= P;  while (q < 0) q += P;  with P = depth - 1, an
   * integer below 2^24.  For |q| < 2^24, ulp(q) <= 1, so q and P are both multiples of u = min(ulp(q), 1).
   *   q > P: every `q - P` of the first loop is a multiple of u that is smaller in magnitude than q, hence representable: the loop
   *     is exact and ends at q - n P in (0, P], which is fmod(q, P) — exact by definition — unless that is 0, then P.
   *   q < 0: every `q + P` that is still negative is exact for the same reason; the loop's last addition starts from the exact
   *     value x = q + (n - 1) P in [-P, 0) and returns fl(x + P).  x is fmod(q, P) when that is non-zero (the result is
   *     fl(fmod + P), one rounding of the same real sum), and -P when it is zero (the result is 0).
   *   0 <= q <= P: unchanged.
   * The remainder is det::fmod's fast path (det_math.h: n = trunc(|q| / P) is within one of the true quotient, fma(-n, P, |q|) is
   * exact because the true remainder is representable, one +-P repairs the off-by-one), WITHOUT its library fallback: that
   * fallback is a per-lane branch into a loop.  Instead a coordinate at or beyond 2^20 periods — an infinite one included, whose
   * remainder would be NaN — is taken as 0 by a select.  The reference's loops would need a million trips there, and beyond 2^24
   * texels they round at every step or never end; no map is sampled that far out on purpose.  No branch, no loop.
   */
  MPPI_TEX_HD static inline float wrapZ(const float q_in, const float period)
  {
    const float P = period >= 1.0f ? period : 1.0f;  // depth 1 with wrap is refused on the host; no division by 0 here
    const bool far = !(mppi::det::fabs(q_in) < 1048576.0f * P);
    const float q = far ? 0.0f : q_in;
    const float aa = mppi::det::fabs(q);
    const float n = mppi::det::trunc(aa * (1.0f / P));
    float r = mppi::det::fma(-n, P, aa);
    const float rp = r + P, rm = r - P;
    r = (r < 0.0f) ? rp : ((r >= P) ? rm : r);
    r = mppi::det::copysign(r, q);  // fmod(q, P): the sign of q, |r| < P
    const float above = (r == 0.0f) ? P : r;
    const float below = (r == 0.0f) ? 0.0f : r + P;
    return (q > P) ? above : ((q < 0.0f) ? below : q);
  }

  /**
   * The eight taps and three weights of one trilinear lookup (three_d_texture_helper.cu:140-241).  No per-lane branch: the address
   * modes are selects on the coordinate and index min / max, except that the z wrap (a division and a dozen operations) sits
   * behind ONE wave-uniform branch on address_mode[2], a kernel argument, so that clamp and border addressing do not pay for it; in border mode an outside point is only FLAGGED and its taps are
   * those of the clamped coordinate (valid addresses; the caller substitutes the border colour with a final select), so a
   * caller can compute several footprints, issue all their loads, and only then blend.
   * Address arithmetic: one 32-bit texel index for the (z_min, y_min, x_min) corner and three 32-bit strides (0 where an axis
   * has one texel); the seven other corners are sums of those, so a corner costs one add and one 64-bit scaled add to the base.
   */
  struct LinearFootprint
  {
    int i000;        ///< texel index of (z_min, y_min, x_min), before the channel stride
    int sx, sy, sz;  ///< index strides to x_max, y_max, z_max
    float xd, yd, zd;
    bool border;
  };
  /** one axis: coordinate -> (clamped coordinate, outside flag) */
  MPPI_TEX_HD static inline float clampAxis(const float q, const int extent, bool& outside)
  {
    const float last = (float)(extent - 1);
    const bool hi = q > last, lo = q <= 0.0f;
    outside = hi || lo;
    return hi ? last : (lo ? 0.0f : q);
  }
  MPPI_TEX_HD inline LinearFootprint linearFootprint(const int index, const float* point) const
  {
    const TextureParams3D& p = textures_[index];
    const int w = p.width, h = p.height, d = p.depth;
    float qx = point[0] * (float)w - 0.5f;
    float qy = point[1] * (float)h - 0.5f;
    float qz = point[2] * (float)d - 0.5f;
    // a NaN coordinate (a diverged rollout) would reach (int)floorf(NaN): it samples texel 0
    qx = (qx == qx) ? qx : 0.0f;
    qy = (qy == qy) ? qy : 0.0f;
    qz = (qz == qz) ? qz : 0.0f;
    if (p.address_mode[2] == ADDRESS_WRAP)  // the same for every lane: the mode is a kernel argument
      qz = wrapZ(qz, (float)(d - 1));
    bool out_x, out_y, out_z;
    // clamp addressing; the identity for an inside point of border addressing and for a wrapped z (which lies in [0, depth - 1])
    qx = clampAxis(qx, w, out_x);
    qy = clampAxis(qy, h, out_y);
    qz = clampAxis(qz, d, out_z);
    LinearFootprint f;
    f.border = (p.address_mode[0] == ADDRESS_BORDER && out_x) || (p.address_mode[1] == ADDRESS_BORDER && out_y) ||
               (p.address_mode[2] == ADDRESS_BORDER && out_z);
    const int x_min = imax(imin((int)floorf(qx), w - 2), 0);
    const int y_min = imax(imin((int)floorf(qy), h - 2), 0);
    const int z_min = imax(imin((int)floorf(qz), d - 2), 0);
    // the reference writes (q - x_min) / (x_max - x_min); the denominator is 1, and a division by 1.0f returns its numerator
    // bit for bit.  A one-texel axis has no second sample: stride 0 and d = 0
    f.xd = (w > 1) ? (qx - (float)x_min) : 0.0f;
    f.yd = (h > 1) ? (qy - (float)y_min) : 0.0f;
    f.zd = (d > 1) ? (qz - (float)z_min) : 0.0f;
    f.sx = (w > 1) ? 1 : 0;
    f.sy = (h > 1) ? w : 0;
    f.sz = (d > 1) ? w * h : 0;
    f.i000 = (z_min * h + y_min) * w + x_min;
    return f;
  }

  /** corner c of a footprint: bit 0 x_max, bit 1 y_max, bit 2 z_max */
  MPPI_TEX_HD static inline int cornerIndex(const LinearFootprint& f, const int c)
  {
    return f.i000 + ((c & 1) ? f.sx : 0) + ((c & 2) ? f.sy : 0) + ((c & 4) ? f.sz : 0);
  }

  /** one texel: NC floats; four channels as ONE 16-byte load on the device (the data of a volume starts 16-byte aligned: it is
   *  an allocation of its own) */
  MPPI_TEX_HD inline void loadTexel(const TextureParams3D& p, const int texel, float* out) const
  {
    if (NC == 4)
    {
#if defined(__HIP_DEVICE_COMPILE__)
      const float4 t = *reinterpret_cast<const float4*>(p.data + (size_t)texel * 4);
      out[0] = t.x;
      out[1] = t.y;
      out[2] = t.z;
      out[3] = t.w;
#else
      memcpy(out, p.data + (size_t)texel * 4, 4 * sizeof(float));
#endif
    }
    else
    {
      out[0] = p.data[(size_t)texel];
    }
  }

  /** the interpolation itself, in the reference's order and expression form (three_d_texture_helper.cu:257-268); q[c] is the
   *  value at corner c of cornerIndex() */
  MPPI_TEX_HD static inline float interpolate(const LinearFootprint& f, const float* q, const int stride)
  {
    const float c_000 = q[0 * stride], c_100 = q[1 * stride], c_010 = q[2 * stride], c_110 = q[3 * stride];
    const float c_001 = q[4 * stride], c_101 = q[5 * stride], c_011 = q[6 * stride], c_111 = q[7 * stride];
    const float c_00 = c_000 * (1 - f.xd) + c_100 * f.xd;
    const float c_01 = c_001 * (1 - f.xd) + c_101 * f.xd;
    const float c_10 = c_010 * (1 - f.xd) + c_110 * f.xd;
    const float c_11 = c_011 * (1 - f.xd) + c_111 * f.xd;
    const float c_0 = c_00 * (1 - f.yd) + c_10 * f.yd;
    const float c_1 = c_01 * (1 - f.yd) + c_11 * f.yd;
    return c_0 * (1 - f.zd) + c_1 * f.zd;
  }

  /** the nearest texel (three_d_texture_helper.cu:273-277) and whether the point is border */
  MPPI_TEX_HD inline int pointIndex(const int index, const float* point, bool& border) const
  {
    const TextureParams3D& p = textures_[index];
    const int w = p.width, h = p.height, d = p.depth;
    float qx = point[0] * (float)w - 0.5f;
    float qy = point[1] * (float)h - 0.5f;
    float qz = point[2] * (float)d - 0.5f;
    qx = (qx == qx) ? qx : 0.0f;
    qy = (qy == qy) ? qy : 0.0f;
    qz = (qz == qz) ? qz : 0.0f;
    if (p.address_mode[2] == ADDRESS_WRAP)  // the same for every lane: the mode is a kernel argument
      qz = wrapZ(qz, (float)(d - 1));
    bool out_x, out_y, out_z;
    qx = clampAxis(qx, w, out_x);
    qy = clampAxis(qy, h, out_y);
    qz = clampAxis(qz, d, out_z);
    border = (p.address_mode[0] == ADDRESS_BORDER && out_x) || (p.address_mode[1] == ADDRESS_BORDER && out_y) ||
             (p.address_mode[2] == ADDRESS_BORDER && out_z);
    return ((int)roundf(qz) * h + (int)roundf(qy)) * w + (int)roundf(qx);
  }

  /** three_d_texture_helper.cu:135-282 (the host branch): trilinear interpolation or the nearest texel */
  MPPI_TEX_HD inline void queryTexture(const int index, const float* point, float* out) const
  {
    const TextureParams3D& p = textures_[index];
    if (p.filter_mode == FILTER_POINT)
    {
      bool border;
      const int texel = pointIndex(index, point, border);
      float v[NC];
      loadTexel(p, texel, v);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (int ch = 0; ch < NC; ch++)
      {
        // both values first, then the select — never `border ? &border_color : &data` (two_d_texture_helper.hpp has the story)
        float texel_value = v[ch];
#if defined(__HIP_DEVICE_COMPILE__)
        asm volatile("" : "+v"(texel_value));
#endif
        const float edge = p.border_color[ch];
        out[ch] = border ? edge : texel_value;
      }
      return;
    }
    const LinearFootprint f = linearFootprint(index, point);
    float q[8][NC];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int c = 0; c < 8; c++)  // all eight loads are issued before the first blend
      loadTexel(p, cornerIndex(f, c), q[c]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int ch = 0; ch < NC; ch++)
    {
      const float v = interpolate(f, &q[0][ch], NC);
      out[ch] = f.border ? p.border_color[ch] : v;
    }
  }

  /**
   * N lookups at world poses whose loads are all in flight together: footprints first, then the 8 N loads, then the blends (the
   * 2-D helper's batch form with twice the corners).  Same values as N single calls.  world: [N][3], out: [N][NC].
   */
  template <int N>
  MPPI_TEX_HD inline void queryTextureAtWorldPoseBatch(const int index, const float (*world)[3], float* out) const
  {
    const TextureParams3D& p = textures_[index];
    if (p.filter_mode == FILTER_POINT)
    {
      for (int n = 0; n < N; n++)
        queryTextureAtWorldPose(index, world[n], out + n * NC);
      return;
    }
    LinearFootprint f[N];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int n = 0; n < N; n++)
    {
      float map[3], tex[3];
      worldPoseToMapPose(index, world[n], map);
      mapPoseToTexCoord(index, map, tex);
      f[n] = linearFootprint(index, tex);
    }
    float q[N][8][NC];
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int n = 0; n < N; n++)
      for (int c = 0; c < 8; c++)
        loadTexel(p, cornerIndex(f[n], c), q[n][c]);
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (int n = 0; n < N; n++)
      for (int ch = 0; ch < NC; ch++)
      {
        const float v = interpolate(f[n], &q[n][0][ch], NC);
        out[n * NC + ch] = f[n].border ? p.border_color[ch] : v;
      }
  }

  /** texture_helper.cu:274-280 */
  MPPI_TEX_HD inline void queryTextureAtWorldPose(const int index, const float* input, float* out) const
  {
    float map[3], tex[3];
    worldPoseToMapPose(index, input, map);
    mapPoseToTexCoord(index, map, tex);
    queryTexture(index, tex, out);
  }

  /** texture_helper.cu:283-289 */
  MPPI_TEX_HD inline void queryTextureAtMapPose(const int index, const float* input, float* out) const
  {
    float tex[3];
    mapPoseToTexCoord(index, input, tex);
    queryTexture(index, tex, out);
  }

private:
  MPPI_TEX_HD static inline int imin(int a, int b)
  {
    return a < b ? a : b;
  }
  MPPI_TEX_HD static inline int imax(int a, int b)
  {
    return a > b ? a : b;
  }
};

/** what the reference's host path throws on (three_d_texture_helper.cu:165-168, 188-191, 222-225): wrap on x or y, an unknown
 *  mode on any axis; and wrap on a z axis of one layer, whose period is 0.  Empty when the modes can be sampled. */
inline std::string addressModesRefusal(const int* address_mode, int depth)
{
  for (int axis = 0; axis < 3; axis++)
  {
    const int mode = address_mode[axis];
    if (mode == ADDRESS_CLAMP || mode == ADDRESS_BORDER)
      continue;
    if (mode != ADDRESS_WRAP)
      return "unknown address mode " + std::to_string(mode) + " on axis " + std::to_string(axis);
    if (axis != 2)
      return std::string("wrap addressing exists on z only, not on ") + (axis == 0 ? "x" : "y");
    if (depth < 2)
      return "wrap addressing on z needs at least two layers (its period is depth - 1)";
  }
  return std::string();
}

/** largest volume a 32-bit texel index addresses */
inline bool extentIndexable(long long width, long long height, long long depth, int channels)
{
  return width > 0 && height > 0 && depth > 0 && width * height <= 0x7fffffffLL && width * height * depth * channels <= 0x7fffffffLL;
}

/** the reference's UpdateTextureException cases (three_d_texture_helper.cu:37-41) and those of setExtent (:288-293) */
struct TextureUpdateError : public std::runtime_error
{
  using std::runtime_error::runtime_error;
};

/**
 * Host side of ThreeDTextureHelper: owns the values of NUM_TEXTURES volumes, takes them a layer at a time (updateTexture, row-
 * or column-major) or whole, remembers which layers changed since the last copy (the reference's layer_copy_), and uploads only
 * those, as contiguous slices of one allocation per texture.
 *
 * copyTo(sink) is the copy itself, written against a two-method sink so that the slice logic runs where there is no device:
 *   const float* sink.allocate(int index, size_t floats)                 a new allocation for texture `index` (the old one goes);
 *                                                                        nullptr when it failed
 *   bool         sink.write(int index, size_t offset, const float* src, size_t floats)     false when it failed
 * A texture whose allocation or copy failed keeps its dirty flags (and asks for a new allocation again if that was what failed),
 * is not put in use by that copy, and copyTo() returns false.
 * copyToDevice() (below, where the compiler is hipcc) is copyTo() on DeviceTextureSink, whose allocations are HipBuffers
 * (engine/hip_owned.hpp).  After a copy, view() is the POD a kernel takes.
 */
template <int NUM_TEXTURES, int NC = 1>
class ThreeDTextureHelperHost
{
public:
  using Helper = ThreeDTextureHelper<NUM_TEXTURES, NC>;

  /** three_d_texture_helper.cu:285-315: a new extent resizes the values (zeroed: the layout changed) and marks every layer
   *  for the next copy.  The same extent again changes nothing.  Returns whether it changed. */
  bool setExtent(int index, int width, int height, int depth)
  {
    TextureParams3D& p = at(index);
    if (depth <= 0)
      throw TextureUpdateError("setExtent: a 3-D texture cannot have depth " + std::to_string(depth));
    if (!extentIndexable(width, height, depth, NC))
      throw TextureUpdateError("setExtent: extent " + std::to_string(width) + " x " + std::to_string(height) + " x " +
                               std::to_string(depth) + " is empty or beyond a 32-bit texel index");
    if (p.width == width && p.height == height && p.depth == depth)
      return false;
    p.width = width;
    p.height = height;
    p.depth = depth;
    values_[index].assign((size_t)width * height * depth * NC, 0.0f);
    dirty_[index].assign((size_t)depth, true);
    reallocate_[index] = true;
    return true;
  }

  /** three_d_texture_helper.cu:28-76: one layer, width * height texels of NC floats, row-major [y][x] or column-major [x][y] */
  void updateTexture(int index, int z_index, const std::vector<float>& values, bool column_major = false)
  {
    const TextureParams3D& p = at(index);
    const size_t w = (size_t)p.width, h = (size_t)p.height;
    if (values.size() != w * h * NC)
      throw TextureUpdateError("updateTexture: " + std::to_string(values.size()) + " floats for a layer of " + std::to_string(w * h * NC));
    if (z_index < 0 || z_index >= p.depth)
      throw TextureUpdateError("updateTexture: layer " + std::to_string(z_index) + " outside depth " + std::to_string(p.depth));
    float* layer = values_[index].data() + w * h * NC * (size_t)z_index;
    if (column_major)
    {
      for (size_t x = 0; x < w; x++)
        for (size_t y = 0; y < h; y++)
          memcpy(layer + (y * w + x) * NC, values.data() + (x * h + y) * NC, NC * sizeof(float));
    }
    else
    {
      memcpy(layer, values.data(), values.size() * sizeof(float));
    }
    dirty_[index][(size_t)z_index] = true;
  }

  /** the whole volume at once, [depth][height][width][NC] */
  void updateTexture(int index, const std::vector<float>& whole_volume)
  {
    const TextureParams3D& p = at(index);
    if (whole_volume.size() != values_[index].size() || whole_volume.empty())
      throw TextureUpdateError("updateTexture: " + std::to_string(whole_volume.size()) + " floats for a volume of " +
                               std::to_string(values_[index].size()));
    values_[index] = whole_volume;
    dirty_[index].assign((size_t)p.depth, true);
  }

  /** wrap on x or y, wrap on a one-layer z, an unknown mode: refused here, so that no launch ever carries them */
  void updateAddressMode(int index, int axis, int mode)
  {
    TextureParams3D& p = at(index);
    if (axis < 0 || axis > 2)
      throw TextureUpdateError("updateAddressMode: axis " + std::to_string(axis));
    int modes[3] = { p.address_mode[0], p.address_mode[1], p.address_mode[2] };
    modes[axis] = mode;
    const std::string why = addressModesRefusal(modes, p.depth > 0 ? p.depth : 2);
    if (!why.empty())
      throw TextureUpdateError("updateAddressMode: " + why);
    p.address_mode[axis] = mode;
  }
  void updateFilterMode(int index, int mode)
  {
    if (mode != FILTER_LINEAR && mode != FILTER_POINT)
      throw TextureUpdateError("updateFilterMode: mode " + std::to_string(mode));
    at(index).filter_mode = mode;
  }
  void updateBorderColor(int index, const float* rgba)
  {
    memcpy(at(index).border_color, rgba, sizeof(float) * 4);
  }
  void updateOrigin(int index, const float* origin)
  {
    memcpy(at(index).origin, origin, sizeof(float) * 3);
  }
  void updateRotation(int index, const float* row_major_3x3)
  {
    memcpy(at(index).rotations, row_major_3x3, sizeof(float) * 9);
  }
  void updateResolution(int index, float x, float y, float z)
  {
    TextureParams3D& p = at(index);
    p.resolution[0] = x;
    p.resolution[1] = y;
    p.resolution[2] = z;
  }

  const std::vector<float>& getCpuValues(int index) const
  {
    (void)at(index);
    return values_[index];
  }
  /** the reference's getLayerCopy(): which layers the next copy uploads */
  const std::vector<bool>& getLayerCopy(int index) const
  {
    (void)at(index);
    return dirty_[index];
  }
  /** the dirty layers as maximal runs (first layer, number of layers): the slices the next copy uploads
   *  (three_d_texture_helper.cu:336-377 builds the same runs while it copies) */
  std::vector<std::pair<int, int>> dirtySlices(int index) const
  {
    (void)at(index);
    std::vector<std::pair<int, int>> runs;
    const std::vector<bool>& d = dirty_[index];
    for (size_t z = 0; z < d.size(); z++)
    {
      if (!d[z])
        continue;
      if (!runs.empty() && runs.back().first + runs.back().second == (int)z)
        runs.back().second++;
      else
        runs.emplace_back((int)z, 1);
    }
    return runs;
  }

  /** uploads what changed (see the class comment); the texture is in use from its first successful copy on.  Returns whether
   *  every allocation and every write succeeded */
  template <class SINK>
  bool copyTo(SINK& sink)
  {
    bool all_ok = true;
    for (int i = 0; i < NUM_TEXTURES; i++)
    {
      TextureParams3D& p = params_.textures_[i];
      if (values_[i].empty())
        continue;
      bool ok = true;
      if (reallocate_[i])
      {
        device_[i] = sink.allocate(i, values_[i].size());
        ok = device_[i] != nullptr;
        reallocate_[i] = !ok;
        if (!ok)
          p.use = 0;  // the old allocation is gone
      }
      const size_t layer = (size_t)p.width * p.height * NC;
      if (ok)
        for (const std::pair<int, int>& run : dirtySlices(i))
          ok = sink.write(i, layer * (size_t)run.first, values_[i].data() + layer * (size_t)run.first, layer * (size_t)run.second) && ok;
      if (ok)
      {
        dirty_[i].assign(dirty_[i].size(), false);
        p.use = 1;
      }
      all_ok = all_ok && ok;
    }
    return all_ok;
  }

  /** the POD a kernel takes: parameters and the sink's allocations */
  Helper view() const
  {
    Helper v = params_;
    for (int i = 0; i < NUM_TEXTURES; i++)
      v.textures_[i].data = device_[i];
    return v;
  }
  /** the same parameters over the host's own values: queryTexture() on the host */
  Helper hostView() const
  {
    Helper v = params_;
    for (int i = 0; i < NUM_TEXTURES; i++)
    {
      v.textures_[i].data = values_[i].empty() ? nullptr : values_[i].data();
      v.textures_[i].use = values_[i].empty() ? 0 : 1;
    }
    return v;
  }

private:
  TextureParams3D& at(int index)
  {
    if (index < 0 || index >= NUM_TEXTURES)
      throw TextureUpdateError("texture index " + std::to_string(index) + " outside " + std::to_string(NUM_TEXTURES));
    return params_.textures_[index];
  }
  const TextureParams3D& at(int index) const
  {
    return const_cast<ThreeDTextureHelperHost*>(this)->at(index);
  }

  Helper params_;  ///< data pointers unused: view() / hostView() fill them
  std::vector<float> values_[NUM_TEXTURES];
  std::vector<bool> dirty_[NUM_TEXTURES];
  bool reallocate_[NUM_TEXTURES] = {};
  const float* device_[NUM_TEXTURES] = {};
};

#if defined(__HIPCC__)
/** copyTo()'s sink on the device: one HipBuffer per texture, slices by hipMemcpyAsync on `stream`.  The first error is kept and
 *  later writes are dropped; the caller's values must stay alive until the stream has been synchronised. */
template <int NUM_TEXTURES>
struct DeviceTextureSink
{
  mppi::engine::HipBuffer<float> buffers[NUM_TEXTURES];
  hipStream_t stream = nullptr;
  hipError_t status = hipSuccess;

  const float* allocate(int index, size_t floats)
  {
    const hipError_t e = buffers[index].alloc(floats);
    if (status == hipSuccess)
      status = e;
    return e == hipSuccess ? (const float*)buffers[index] : nullptr;
  }
  bool write(int index, size_t offset, const float* src, size_t floats)
  {
    if (status != hipSuccess || offset + floats > buffers[index].size())
      return false;
    status = hipMemcpyAsync(buffers[index] + offset, src, floats * sizeof(float), hipMemcpyHostToDevice, stream);
    return status == hipSuccess;
  }
};

/** ThreeDTextureHelper::copyToDevice (texture_helper.cu:147-190, three_d_texture_helper.cu:317-390): the changed layers of every
 *  texture into `sink`, then, with `synchronize`, a wait for the stream */
template <int NUM_TEXTURES, int NC>
inline hipError_t copyToDevice(ThreeDTextureHelperHost<NUM_TEXTURES, NC>& host, DeviceTextureSink<NUM_TEXTURES>& sink, bool synchronize = true)
{
  sink.status = hipSuccess;  // an earlier failure is retried: the host object kept what it could not upload marked
  (void)host.copyTo(sink);
  if (sink.status == hipSuccess && synchronize)
    sink.status = hipStreamSynchronize(sink.stream);
  return sink.status;
}
#endif

}  // namespace texture
}  // namespace mppi

#endif
