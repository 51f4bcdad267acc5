/**
 * replay_kernel.hpp — n sampled rollouts of the last iteration run again, keeping what the rollout kernel only accumulates:
 * the output after every step, the cost of every step and the crash status after every step (mppi_replay_rollouts).
 *
 * The reference's visualizeKernel (core/mppi_common.cu:364-525) behind Controller::calculateSampledStateTrajectories
 * (controllers/controller.cu:55-124) and its getSampled{Output,Cost,CrashStatus}Trajectories.  The kernel never draws: a row is
 * a shaped, already clamped control sequence in device memory — row `idx` of the samples the last rollout launch saved
 * (cfg.save_samples), or, for idx == -1, the handle's current control sequence (the reference's slot 0, controller.cu:78-84) —
 * so every sampler is covered without code of its own.  Per row the plugin calls of the rollout kernel, in its order:
 *   initializeDynamics, initializeCosts; per step enforceConstraints, step, computeRunningCost (the crash status threaded
 *   through) + computeLikelihoodRatioCost; terminalCost.
 * enforceConstraints on a saved row is the identity unless the model has a control deadband (the rule then shrinks a control
 * twice).  The likelihood-ratio term is evaluated against the control mean that is on the device NOW: the mean the rollouts saw
 * after mppi_rollout_costs, the updated mean after mppi_compute_control / mppi_optimize (as in the reference, whose sampler
 * holds the new mean by the time the trajectories are asked for).
 *
 * Lanes: the layout the model's trajectory re-roll (finalize_kernel.hpp) uses.
 *   BY == 1, one lane per rollout          a wave is 64 rows, state in registers, no barrier;
 *   BY == 1, REP replicated lanes          a wave is 64 / REP rows (lane = column + (64 / REP) * replica, as in rolloutKernel);
 *                                          replica 0 of a row writes;
 *   BY > 1 (LDS + barrier contract)        one row per block (1, BY, 1), the rollout kernel's barriers between the phases of a
 *                                          step; the step cost is the sum over the y lanes in lane order.
 * Lanes past the last row run the last row again and write nothing: every lane of a wave reaches every plugin call (the MFMA
 * forms need all 64), every address stays in bounds.
 */
#ifndef MPPI_AMD_ENGINE_REPLAY_KERNEL_HPP_
#define MPPI_AMD_ENGINE_REPLAY_KERNEL_HPP_

#include <hip/hip_runtime.h>
#include "mppi_amd/plugin/managed.hpp"
#include "mppi_amd/plugin/math_utils.hpp"
#include "mppi_amd/plugin/parallel_utils.hpp"
#include "rollout_kernel.hpp"

namespace mppi
{
namespace kernels
{
struct ReplayArgs
{
  const float* x0_d;       ///< [S] initial state of the system
  const float* samples_d;  ///< [K_local][T][C] the saved rows of the system; nullptr when no index is >= 0
  const float* optimal_d;  ///< [T][C] the row of index -1
  const int* idx_d;        ///< [n] row indices in [-1, K_local)
  float* y_d;              ///< [n][T][O] output after step t
  float* cost_d;           ///< [n][T + 1] cost of step t; [T]: the terminal cost, undivided
  int* crash_d;            ///< [n][T] crash status after step t
  int n;
  int num_timesteps;
  int system;              ///< distribution index of the likelihood-ratio term
  float dt, lambda, alpha;
};

/** rows per block of the BY == 1 forms (one wave) */
template <class DYN_T>
constexpr int replayBlockRows()
{
  return 64 / replicated_lanes<DYN_T>::value;
}
template <class DYN_T, class COST_T>
__host__ inline size_t replaySharedBytes(const DYN_T& dyn, const COST_T& cost, int by)
{
  constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM, O = DYN_T::OUTPUT_DIM;
  const int slots = by == 1 ? replayBlockRows<DYN_T>() : 1;
  size_t n = calcClassSharedMemSize(&dyn, slots) + calcClassSharedMemSize(&cost, slots);
  if (by > 1)
    n += sizeof(float) * (3 * math::nearest_multiple_4(S) + math::nearest_multiple_4(O) + math::nearest_multiple_4(C) +
                          math::nearest_multiple_4(by) + 4);
  return n;
}

template <class DYN_T, class COST_T, class SAMPLING_T, int BY>
__global__ void __launch_bounds__(BY == 1 ? 64 : BY)
    replayKernel(DYN_T dynamics_obj, COST_T costs_obj, SAMPLING_T sampling_obj, const ReplayArgs a)
{
  constexpr int REP = replicated_lanes<DYN_T>::value;
  static_assert(REP == 1 || BY == 1, "replicated lanes run with one contract lane");
  static_assert(64 % REP == 0, "a wave holds whole rows");
  constexpr int LX = BY == 1 ? 64 : 1;
  MPPI_ASSUME_BLOCK_SHAPE(LX, BY, 1);
  DYN_T* dynamics = &dynamics_obj;
  COST_T* costs = &costs_obj;
  SAMPLING_T* sampling = &sampling_obj;
  constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM, O = DYN_T::OUTPUT_DIM;
  constexpr int ROWS = BY == 1 ? 64 / REP : 1;  // rows of a block == plugin slots
  const int T = a.num_timesteps;
  const float dt = a.dt;
  const int lane = (int)__builtin_amdgcn_workitem_id_x();
  const int ty = (int)__builtin_amdgcn_workitem_id_y();
  const int row_raw = (int)blockIdx.x * ROWS + (BY == 1 ? lane % ROWS : 0);
  const bool valid = row_raw < a.n;
  const int row = valid ? row_raw : a.n - 1;
  const bool writer = valid && (BY == 1 ? lane / ROWS == 0 : ty == 0);
  const int idx = a.idx_d[row];
  const float* urow = idx < 0 ? a.optimal_d : a.samples_d + (size_t)idx * T * C;
  const int sample_index = idx < 0 ? 0 : idx;  // (what the pure-noise rule of the likelihood-ratio term looks at)

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* theta_s = reinterpret_cast<float*>(smem_raw);
  float* theta_c = theta_s + calcClassSharedMemSize(dynamics, ROWS) / (int)sizeof(float);
  float* next_shared = theta_c + calcClassSharedMemSize(costs, ROWS) / (int)sizeof(float);

  float* y_out = a.y_d + (size_t)row * T * O;
  float* cost_out = a.cost_d + (size_t)row * (T + 1);
  int* crash_out = a.crash_d + (size_t)row * T;

  if constexpr (BY == 1)
  {
    float x[S], xn[S], xdot[S], u[C], y[O];
    int crash = 0;
#pragma unroll
    for (int i = 0; i < S; i++)
    {
      x[i] = a.x0_d[i];
      xn[i] = 0.0f;
      xdot[i] = 0.0f;
    }
#pragma unroll
    for (int i = 0; i < C; i++)
      u[i] = 0.0f;
#pragma unroll
    for (int i = 0; i < O; i++)
      y[i] = 0.0f;
    __syncthreads();
    dynamics->initializeDynamics(x, u, y, theta_s, 0.0f, dt);
    costs->initializeCosts(y, u, theta_c, 0.0f, dt);
    __syncthreads();
    for (int t = 0; t < T; t++)
    {
#pragma unroll
      for (int i = 0; i < C; i++)
        u[i] = urow[t * C + i];
      dynamics->enforceConstraints(x, u);
      dynamics->step(x, xn, xdot, u, y, theta_s, t, dt);
      const float c = costs->computeRunningCost(y, u, t, theta_c, &crash) +
                      sampling->computeLikelihoodRatioCost(u, nullptr, sample_index, t, a.system, a.lambda, a.alpha);
      if (writer)
      {
#pragma unroll
        for (int i = 0; i < O; i++)
          y_out[t * O + i] = y[i];
        cost_out[t] = c;
        crash_out[t] = crash;
      }
#pragma unroll
      for (int i = 0; i < S; i++)
        x[i] = xn[i];
    }
    const float terminal = costs->terminalCost(y, theta_c);
    if (writer)
      cost_out[T] = terminal;
  }
  else
  {
    float* x = next_shared;
    float* xn = x + math::nearest_multiple_4(S);
    float* xdot = xn + math::nearest_multiple_4(S);
    float* y = xdot + math::nearest_multiple_4(S);
    float* u = y + math::nearest_multiple_4(O);
    float* lane_cost = u + math::nearest_multiple_4(C);
    int* crash = reinterpret_cast<int*>(lane_cost + math::nearest_multiple_4(BY));
    for (int i = ty; i < S; i += BY)
    {
      x[i] = a.x0_d[i];
      xdot[i] = 0.0f;
    }
    for (int i = ty; i < C; i += BY)
      u[i] = 0.0f;
    for (int i = ty; i < O; i += BY)
      y[i] = 0.0f;
    if (ty == 0)
      crash[0] = 0;
    __syncthreads();
    dynamics->initializeDynamics(x, u, y, theta_s, 0.0f, dt);
    costs->initializeCosts(y, u, theta_c, 0.0f, dt);
    __syncthreads();
    for (int t = 0; t < T; t++)
    {
      for (int i = ty; i < C; i += BY)
        u[i] = urow[t * C + i];
      __syncthreads();
      dynamics->enforceConstraints(x, u);
      __syncthreads();
      dynamics->step(x, xn, xdot, u, y, theta_s, t, dt);
      __syncthreads();
      lane_cost[ty] = costs->computeRunningCost(y, u, t, theta_c, crash) +
                      sampling->computeLikelihoodRatioCost(u, nullptr, sample_index, t, a.system, a.lambda, a.alpha);
      __syncthreads();
      if (writer)
      {
        float acc = 0.0f;
        for (int j = 0; j < BY; j++)
          acc += lane_cost[j];
        cost_out[t] = acc;
        crash_out[t] = crash[0];
      }
      if (valid)
        for (int i = ty; i < O; i += BY)
          y_out[t * O + i] = y[i];
      __syncthreads();  // the next step rewrites u, y and the lane costs
      float* tmp = x;
      x = xn;
      xn = tmp;
    }
    const float terminal = costs->terminalCost(y, theta_c);
    if (writer)
      cost_out[T] = terminal;
  }
}

}  // namespace kernels
}  // namespace mppi

#endif
