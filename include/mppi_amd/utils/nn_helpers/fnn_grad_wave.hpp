/**
 * fnn_grad_wave.hpp — the input Jacobian of the {IN, H, H, OUT} tanh network of the NN dynamics, one evaluation point per wave.
 *
 * What it is for: Dynamics::computeGrad of the AutoRally model (reference: ar_nn_model.cu:64-88) needs d(output) / d(input) of its
 * MLP, which the reference takes from FNNHelper::computeGrad (utils/nn_helpers/fnn_helper.cu:320-351), a host back-propagation
 * with Eigen.  Here it runs on the device, next to fnn_wave.hpp and with its lane assignment: lane j is hidden unit j.
 *
 *   forward     h1_j = tanh(sum_k W1[j][k] in_k + b1_j)          the fma chains of FNNWave::forward, k ascending
 *               h2_j = tanh(sum_k W2[j][k] h1_k + b2_j)          h1_k from lane k (v_readlane)
 *   backward    d2[o]_j = W3[o][j] (1 - h2_j^2)                  in lane j, one value per output o
 *               d1[o]_k = (sum_j W2[j][k] d2[o]_j) (1 - h1_k^2)  lane k walks COLUMN k of W2, j ascending, d2[o]_j from lane j
 *               J[o][i] = sum_k W1[k][i] d1[o]_k                 one product per lane, summed over the wave (wave::waveAllSum)
 *
 * The weights are read from `theta`, the parameter blob [W1 | b1 | W2 | b2 | W3 | b3] every form of the model shares
 * (fnn_helper.cu:176-183) — on the device a copy in LDS that the block staged once: lane k reading column k of W2 touches
 * consecutive words.  4 H + 2 H + IN dependent fmas and OUT * IN wave sums per point.
 *
 * Host and device evaluate the same operations in the same order: the per-lane pieces below are shared, the cross-lane traffic is
 * an array index on the host, and wave::waveAllSum is a pairwise tree over the 64 lanes in lane order (its four butterfly steps add
 * commutatively, then (r0 + r16) + (r32 + r48)), which treeSum64 spells out.  Lanes beyond H contribute +0.
 */
#ifndef MPPI_AMD_FNN_GRAD_WAVE_HPP_
#define MPPI_AMD_FNN_GRAD_WAVE_HPP_

#include <hip/hip_runtime.h>
#include "mppi_amd/det_math.h"
#include "mppi_amd/utils/wave_ops.hpp"

namespace mppi
{
template <int IN, int H, int OUT>
struct FNNGradWave
{
  static_assert(H <= 64, "one lane per hidden unit");
  static constexpr int NUM_PARAMS = IN * H + H + H * H + H + H * OUT + OUT;
  static constexpr int W1 = 0, B1 = W1 + IN * H, W2 = B1 + H, B2 = W2 + H * H, W3 = B2 + H;

  /* ---- what one lane computes; `from(k)` is the value lane k holds ---- */
  __host__ __device__ static inline float hidden1(const float* theta, const float (&in)[IN], const int j)
  {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < IN; k++)
      acc = mppi::det::fma(theta[W1 + j * IN + k], in[k], acc);
    return mppi::det::tanh(acc + theta[B1 + j]);
  }
  template <class FROM>
  __host__ __device__ static inline float hidden2(const float* theta, FROM h1_from, const int j)
  {
    float acc = 0.0f;
#pragma unroll
    for (int k = 0; k < H; k++)
      acc = mppi::det::fma(theta[W2 + j * H + k], h1_from(k), acc);
    return mppi::det::tanh(acc + theta[B2 + j]);
  }
  __host__ __device__ static inline float tanhSlope(const float h)
  {
    return 1.0f - h * h;
  }
  __host__ __device__ static inline float delta2(const float* theta, const float h2, const int o, const int j)
  {
    return theta[W3 + o * H + j] * tanhSlope(h2);
  }
  template <class FROM>
  __host__ __device__ static inline float delta1(const float* theta, FROM d2_from, const float h1, const int k)
  {
    float acc = 0.0f;
#pragma unroll
    for (int j = 0; j < H; j++)
      acc = mppi::det::fma(theta[W2 + j * H + k], d2_from(j), acc);
    return acc * tanhSlope(h1);
  }
  __host__ __device__ static inline float term(const float* theta, const float d1, const int i, const int k)
  {
    return theta[W1 + k * IN + i] * d1;
  }

#if defined(__HIP_DEVICE_COMPILE__)
  __device__ static inline float lane_value(const float v, const int k)
  {
    return __uint_as_float(__builtin_amdgcn_readlane(__float_as_uint(v), k));
  }
  /** all 64 lanes call it with the same `in`; J is the same in every lane on return.  theta: the blob, in LDS or HBM. */
  __device__ static inline void jacobian(const float* theta, const float (&in)[IN], float (&J)[OUT][IN])
  {
    const int lane = (int)(__builtin_amdgcn_workitem_id_x() & 63u);
    const bool live = lane < H;
    const int j = live ? lane : 0;  // lanes beyond the layer repeat unit 0 and add +0 to the sums
    const float h1 = hidden1(theta, in, j);
    const float h2 = hidden2(theta, [&](const int k) { return lane_value(h1, k); }, j);
#pragma unroll
    for (int o = 0; o < OUT; o++)
    {
      const float d2 = delta2(theta, h2, o, j);
      const float d1 = delta1(theta, [&](const int jj) { return lane_value(d2, jj); }, h1, j);
#pragma unroll
      for (int i = 0; i < IN; i++)
        J[o][i] = mppi::wave::waveAllSum(live ? term(theta, d1, i, j) : 0.0f);
    }
  }
#else
  /** wave::waveAllSum's order of additions */
  static inline float treeSum64(float (&v)[64])
  {
    for (int stride = 1; stride < 64; stride *= 2)
      for (int l = 0; l < 64; l += 2 * stride)
        v[l] = v[l] + v[l + stride];
    return v[0];
  }
  static inline void jacobian(const float* theta, const float (&in)[IN], float (&J)[OUT][IN])
  {
    float h1[H], h2[H], d2[H], d1[H], terms[64];
    for (int j = 0; j < H; j++)
      h1[j] = hidden1(theta, in, j);
    for (int j = 0; j < H; j++)
      h2[j] = hidden2(theta, [&](const int k) { return h1[k]; }, j);
    for (int o = 0; o < OUT; o++)
    {
      for (int j = 0; j < H; j++)
        d2[j] = delta2(theta, h2[j], o, j);
      for (int k = 0; k < H; k++)
        d1[k] = delta1(theta, [&](const int j) { return d2[j]; }, h1[k], k);
      for (int i = 0; i < IN; i++)
      {
        for (int l = 0; l < 64; l++)
          terms[l] = l < H ? term(theta, d1[l], i, l) : 0.0f;
        J[o][i] = treeSum64(terms);
      }
    }
  }
#endif
};
}  // namespace mppi
#endif
