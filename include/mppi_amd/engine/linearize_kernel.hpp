/**
 * linearize_kernel.hpp — the Jacobians A = d xdot / d x and B = d xdot / d u of a model at n points, one launch for all of them.
 *
 * The device side of Dynamics::computeGrad (plugin/dynamics.hpp: has_compute_grad): what the reference's DDP feedback evaluates on
 * the host once per time step of the nominal trajectory (include/mppi/ddp/ddp_model_wrapper.h:26).  The points are n (x, u)
 * pairs in device memory, x[n][S] and u[n][C] — arbitrary ones (mppi_linearize) or the state and control sequences of the last
 * computeControl where the finalize kernel left them (mppi_linearize_trajectory): the kernel only reads them.
 *
 * A block serves a run of consecutive points and builds their matrices in LDS, one row of S*S + S*C floats per point (the row
 * stride is odd: lanes writing the same entry of neighbouring points hit different banks):
 *   - lane-per-point models (compute_grad_lane): 64 points, one wave, lane p evaluates point p;
 *   - wave-per-point models (compute_grad_wave; the network model): LINEARIZE_WAVES = 16 points, one per wave, after the block has
 *     staged the model's shared region (the network's weights) once.  One point per wave keeps the launch as short as one
 *     evaluation — a trajectory of 150 points is 10 blocks on as many CUs — at the price of staging 5.6 KB per 16 points.
 * The rows are cleared before the model is called — its formula sets only the non-zero entries — and copied out by the whole
 * block, consecutive lanes to consecutive words: the matrices of a block are one contiguous range of A_out, and of B_out.
 * The model's method holds no barrier; the two block barriers here belong to the kernel (clear + stage | evaluate | copy out).
 */
#ifndef MPPI_AMD_ENGINE_LINEARIZE_KERNEL_HPP_
#define MPPI_AMD_ENGINE_LINEARIZE_KERNEL_HPP_

#include <hip/hip_runtime.h>
#include <type_traits>

#include "mppi_amd/plugin/dynamics.hpp"

namespace mppi
{
namespace kernels
{
constexpr int LINEARIZE_WAVES = 16;  ///< waves of a block of a wave-per-point model: one point each

struct LinearizeArgs
{
  const float* x_d;  ///< [n][S]
  const float* u_d;  ///< [n][C]
  float* A_d;        ///< [n][S][S]
  float* B_d;        ///< [n][S][C]
  int n;
};

template <class DYN_T>
constexpr int linearizeBlockWaves()
{
  return mppi::compute_grad_wave<DYN_T>::value ? LINEARIZE_WAVES : 1;
}
/** points per block */
template <class DYN_T>
constexpr int linearizeBlockPoints()
{
  return mppi::compute_grad_wave<DYN_T>::value ? LINEARIZE_WAVES : 64;
}
/** floats of one point's row in LDS: A then B, padded to an odd count */
template <class DYN_T>
constexpr int linearizeRowFloats()
{
  return (DYN_T::STATE_DIM * DYN_T::STATE_DIM + DYN_T::STATE_DIM * DYN_T::CONTROL_DIM) | 1;
}
template <class DYN_T>
inline int linearizeModelSharedBytes(const DYN_T& dyn)
{
  if constexpr (mppi::compute_grad_wave<DYN_T>::value)
    return (dyn.getGradSharedSizeBytes() + 15) / 16 * 16;
  else
    return 0;
}
template <class DYN_T>
inline size_t linearizeSharedBytes(const DYN_T& dyn)
{
  return (size_t)linearizeModelSharedBytes(dyn) + sizeof(float) * linearizeBlockPoints<DYN_T>() * linearizeRowFloats<DYN_T>();
}

template <class DYN_T>
__global__ void __launch_bounds__(64 * linearizeBlockWaves<DYN_T>()) linearizeKernel(DYN_T dynamics_obj, LinearizeArgs a, int model_shared_bytes)
{
  constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM;
  constexpr int SS = S * S, SC = S * C, ROW = linearizeRowFloats<DYN_T>();
  constexpr int WAVES = linearizeBlockWaves<DYN_T>(), THREADS = 64 * WAVES, POINTS = linearizeBlockPoints<DYN_T>();
  __builtin_assume(__builtin_amdgcn_workgroup_size_x() == THREADS);
  __builtin_assume(__builtin_amdgcn_workgroup_size_y() == 1);
  __builtin_assume(__builtin_amdgcn_workgroup_size_z() == 1);
  DYN_T* dynamics = &dynamics_obj;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* theta_s = reinterpret_cast<float*>(smem_raw);
  float* rows = reinterpret_cast<float*>(smem_raw + model_shared_bytes);

  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int p0 = (int)blockIdx.x * POINTS;
  const int np = min(POINTS, a.n - p0);  // >= 1: the grid is ceil(n / POINTS)

  for (int e = tid; e < np * ROW; e += THREADS)
    rows[e] = 0.0f;
  if constexpr (mppi::compute_grad_wave<DYN_T>::value)
    dynamics->initializeGrad(theta_s);
  __syncthreads();

  if constexpr (mppi::compute_grad_wave<DYN_T>::value)
  {
    for (int p = tid >> 6; p < np; p += WAVES)  // uniform in the wave
    {
      float x[S], u[C];
#pragma unroll
      for (int i = 0; i < S; i++)
        x[i] = a.x_d[(size_t)(p0 + p) * S + i];
#pragma unroll
      for (int i = 0; i < C; i++)
        u[i] = a.u_d[(size_t)(p0 + p) * C + i];
      (void)dynamics->computeGrad(x, u, rows + p * ROW, rows + p * ROW + SS, theta_s);
    }
  }
  else
  {
    if (tid < np)
    {
      float x[S], u[C];
#pragma unroll
      for (int i = 0; i < S; i++)
        x[i] = a.x_d[(size_t)(p0 + tid) * S + i];
#pragma unroll
      for (int i = 0; i < C; i++)
        u[i] = a.u_d[(size_t)(p0 + tid) * C + i];
      (void)dynamics->computeGrad(x, u, rows + tid * ROW, rows + tid * ROW + SS);
    }
  }
  __syncthreads();

  float* A_blk = a.A_d + (size_t)p0 * SS;
  for (int e = tid; e < np * SS; e += THREADS)
  {
    const int p = e / SS;
    A_blk[e] = rows[p * ROW + (e - p * SS)];
  }
  float* B_blk = a.B_d + (size_t)p0 * SC;
  for (int e = tid; e < np * SC; e += THREADS)
  {
    const int p = e / SC;
    B_blk[e] = rows[p * ROW + SS + (e - p * SC)];
  }
}

}  // namespace kernels
}  // namespace mppi

#endif
