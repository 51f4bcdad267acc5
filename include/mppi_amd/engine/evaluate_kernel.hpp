/**
 * evaluate_kernel.hpp — the trajectory cost of n control sequences the CALLER brings (mppi_evaluate_controls, mppi_warm_start):
 * the shifted previous solution, zeros, a braking manoeuvre, a library of primitives, another planner's plan.
 *
 * Row i is the cost the rollout kernel would give a rollout whose clamped controls are u[i], WITHOUT the likelihood-ratio term: a
 * candidate is not a sample of the current distribution, there is no mean it was drawn around.  Per row the plugin calls of the
 * rollout kernel, in its order:
 *   initializeDynamics, initializeCosts; per step enforceConstraints (once), step, computeRunningCost (the crash status threaded
 *   through); terminalCost.
 * The step costs are summed over t serially in fp32, the result is running / T + terminal / T (computeAndSaveCost,
 * mppi_common.cu:843-853, as initEvalKernel writes it), next to it the crash status after the last step.  No sampler, nothing kept
 * per step, a per-row initial state (x0_stride == S) or one for all rows (x0_stride == 0).
 *
 * Lanes: the three layouts of replayKernel (replay_kernel.hpp), those of the model's trajectory re-roll.
 *   BY == 1, one lane per row              a wave is 64 rows, state in registers, no barrier;
 *   BY == 1, REP replicated lanes          a wave is 64 / REP rows (lane = column + (64 / REP) * replica); replica 0 writes;
 *   BY > 1 (LDS + barrier contract)        one row per block (1, BY, 1), the rollout kernel's barriers between the phases of a
 *                                          step; the step cost is the sum over the y lanes in lane order.
 * A grid of ceil(n / rows) blocks.  Lanes past the last row run the last row again and write nothing: every lane of a wave reaches
 * every plugin call (the MFMA forms need all 64), every address stays in bounds.  Adjacent lanes read control rows T * C floats
 * apart, straight from HBM: a row's next steps are in the cache line its last step fetched.
 */
#ifndef MPPI_AMD_ENGINE_EVALUATE_KERNEL_HPP_
#define MPPI_AMD_ENGINE_EVALUATE_KERNEL_HPP_

#include <hip/hip_runtime.h>
#include "mppi_amd/plugin/managed.hpp"
#include "mppi_amd/plugin/math_utils.hpp"
#include "mppi_amd/plugin/parallel_utils.hpp"
#include "rollout_kernel.hpp"

namespace mppi
{
namespace kernels
{
struct EvaluateArgs
{
  const float* x0_d;  ///< [1][S] or [n][S] initial states
  int x0_stride;      ///< 0: every row starts from x0_d[0..S); S: row i starts from x0_d[i * S ..)
  const float* u_d;   ///< [n][T][C] the caller's control sequences, unclamped
  float* cost_d;      ///< [n] trajectory cost
  int* crash_d;       ///< [n] crash status after the last step
  int n;
  int num_timesteps;
  float dt;
};

/** rows per block of the BY == 1 forms (one wave) */
template <class DYN_T>
constexpr int evaluateBlockRows()
{
  return 64 / replicated_lanes<DYN_T>::value;
}
template <class DYN_T, class COST_T>
__host__ inline size_t evaluateSharedBytes(const DYN_T& dyn, const COST_T& cost, int by)
{
  constexpr int S = DYN_T::STATE_DIM, C = DYN_T::CONTROL_DIM, O = DYN_T::OUTPUT_DIM;
  const int slots = by == 1 ? evaluateBlockRows<DYN_T>() : 1;
  size_t n = calcClassSharedMemSize(&dyn, slots) + calcClassSharedMemSize(&cost, slots);
  if (by > 1)
    n += sizeof(float) * (3 * math::nearest_multiple_4(S) + math::nearest_multiple_4(O) + math::nearest_multiple_4(C) +
                          math::nearest_multiple_4(by) + 4);
  return n;
}

template <class DYN_T, class COST_T, int BY>
__global__ void __launch_bounds__(BY == 1 ? 64 : BY)
    evaluateKernel(DYN_T dynamics_obj, COST_T costs_obj, const EvaluateArgs a)
{
  constexpr int REP = replicated_lanes<DYN_T>::value;
  static_assert(REP == 1 || BY == 1, "replicated lanes run with one contract lane");
  static_assert(64 % REP == 0, "a wave holds whole rows");
  constexpr int LX = BY == 1 ? 64 : 1;
  MPPI_ASSUME_BLOCK_SHAPE(LX, BY, 1);
  DYN_T* dynamics = &dynamics_obj;
  COST_T* costs = &costs_obj;
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
  const float* urow = a.u_d + (size_t)row * T * C;
  const float* x0 = a.x0_d + (size_t)row * a.x0_stride;

  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  float* theta_s = reinterpret_cast<float*>(smem_raw);
  float* theta_c = theta_s + calcClassSharedMemSize(dynamics, ROWS) / (int)sizeof(float);
  float* next_shared = theta_c + calcClassSharedMemSize(costs, ROWS) / (int)sizeof(float);

  float running = 0.0f;
  if constexpr (BY == 1)
  {
    float x[S], xn[S], xdot[S], u[C], y[O];
    int crash = 0;
#pragma unroll
    for (int i = 0; i < S; i++)
    {
      x[i] = x0[i];
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
      running += costs->computeRunningCost(y, u, t, theta_c, &crash);
#pragma unroll
      for (int i = 0; i < S; i++)
        x[i] = xn[i];
    }
    const float terminal = costs->terminalCost(y, theta_c);
    if (writer)
    {
      a.cost_d[row] = running / (float)T + terminal / (float)T;
      a.crash_d[row] = crash;
    }
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
      x[i] = x0[i];
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
      lane_cost[ty] = costs->computeRunningCost(y, u, t, theta_c, crash);
      __syncthreads();
      if (ty == 0)
      {
        float acc = 0.0f;
        for (int j = 0; j < BY; j++)
          acc += lane_cost[j];
        running += acc;
      }
      __syncthreads();  // the next step rewrites u, y and the lane costs
      float* tmp = x;
      x = xn;
      xn = tmp;
    }
    const float terminal = costs->terminalCost(y, theta_c);
    if (writer)
    {
      a.cost_d[row] = running / (float)T + terminal / (float)T;
      a.crash_d[row] = crash[0];
    }
  }
}

}  // namespace kernels
}  // namespace mppi

#endif
