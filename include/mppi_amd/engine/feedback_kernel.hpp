/**
 * feedback_kernel.hpp — the DDP tracking gains K_t of a trajectory from its Jacobians, on the device: the consumer of
 * linearizeKernel's output (engine/linearize_kernel.hpp), which therefore never travels to the host.
 *
 * ddpBackwardKernel<S, C> is the backward pass of feedback_controllers/ddp_backward.hpp (the reference's ddp/ddp.h:88-124 with
 * DDPFeedback's costs): T - 1 steps, each needing the Vxx of the one before — a dependent chain, so ONE workgroup of ONE wave
 * walks it and the time is the chain's, not the flops'.  What the kernel is built around:
 *   - the entries of a step's small products are spread over the 64 lanes (entry e of a phase: lane e % 64, pass e / 64; S = 13,
 *     C = 4: 221 entries of W, 221 of Qm, 169 of Vxx — four, four and three passes); every entry is evaluated by the header's own
 *     function, whose chain order is fixed there, so the lane assignment cannot change a bit;
 *   - Vxx, F = [Phi | Bd], W, Qm and Lk live in LDS (3.8 KB at S = 13, C = 4); between the four phases of a step stands
 *     phaseSync(): mppi::lane_sync() — nothing for this one-wave block — and a wavefront-scope fence, which keeps the compiler
 *     from moving an LDS read over another lane's write; the hardware runs a wave's LDS operations in order.  No s_barrier;
 *   - A_{k-1}, B_{k-1} are loaded from global memory into registers at the top of step k and turned into F only in its last
 *     phase: the HBM / L2 round trip runs beside the step's arithmetic, none sits on the chain;
 *   - every lane factorises quu (C <= 4: a few dozen operations, all lanes the same values), so success is wave-uniform without
 *     a vote and the lanes j < S go on to solve their column of Lk and write its C gains.
 * The loop bound is the kernel argument T; there is no spinning, no atomic and no communication between blocks (there is one).
 *
 * Output: gains[T][S][C], [t][i][j] = L_t(j, i) (DDPFeedbackState::fb_gain_traj_, what mppi_set_feedback_gains takes), row T - 1
 * zero; status[2] = { ok, failing step or -1 }.  After a failed pivot at step k the rows k ... 0 are not written.
 */
#ifndef MPPI_AMD_ENGINE_FEEDBACK_KERNEL_HPP_
#define MPPI_AMD_ENGINE_FEEDBACK_KERNEL_HPP_

#include <hip/hip_runtime.h>

#include "mppi_amd/feedback_controllers/ddp_backward.hpp"
#include "mppi_amd/plugin/parallel_utils.hpp"

namespace mppi
{
namespace kernels
{
struct DdpBackwardArgs
{
  const float* A_d;    ///< [T][S][S] continuous-time, as linearizeKernel wrote it
  const float* B_d;    ///< [T][S][C]
  const float* Q_d;    ///< [S][S]
  const float* R_d;    ///< [C][C]
  const float* Qf_d;   ///< [S][S]
  float* gains_d;      ///< [T][S][C]
  int* status_d;       ///< [2]: ok, failing step
  float dt;
  int T;
};

/** between two phases of a step: the writes of every lane to LDS before, the reads after */
__device__ inline void ddpPhaseSync()
{
  mppi::lane_sync();
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

template <int S, int C>
__global__ void __launch_bounds__(64) ddpBackwardKernel(DdpBackwardArgs a)
{
  constexpr int N = S + C, SS = S * S, SC = S * C, NF = S * N, NQ = S * S + C * N;
  constexpr int PF = (NF + 63) / 64, PQ = (NQ + 63) / 64, PV = (SS + 63) / 64;
  __builtin_assume(__builtin_amdgcn_workgroup_size_x() == 64);
  __builtin_assume(__builtin_amdgcn_workgroup_size_y() == 1);
  __builtin_assume(__builtin_amdgcn_workgroup_size_z() == 1);
  __shared__ float V[SS], F[NF], W[NF], Qm[N * N], Lk[SC];

  const int lane = (int)__builtin_amdgcn_workitem_id_x();
  const int T = a.T;
  const float dt = a.dt;

  for (int e = lane; e < SC; e += 64)
    a.gains_d[(size_t)(T - 1) * SC + e] = 0.0f;
  if (T < 2)
  {
    if (lane == 0)
    {
      a.status_d[0] = 1;
      a.status_d[1] = -1;
    }
    return;
  }

  // this lane's entries, the same in every step: of F and W (row fi, column fj), of Qm (row qr, column qc, additive term
  // qcost) and of Vxx
  int fi[PF], fj[PF], qr[PQ], qc[PQ];
  float qcost[PQ];
#pragma unroll
  for (int p = 0; p < PF; p++)
  {
    const int e = min(lane + 64 * p, NF - 1);
    fi[p] = e / N;
    fj[p] = e - fi[p] * N;
  }
#pragma unroll
  for (int p = 0; p < PQ; p++)
  {
    ddp::qIndex<S, C>(min(lane + 64 * p, NQ - 1), qr[p], qc[p]);
    qcost[p] = ddp::costEntry<S, C>(a.Q_d, a.R_d, dt, qr[p], qc[p]);
  }

#pragma unroll
  for (int p = 0; p < PV; p++)
  {
    const int e = lane + 64 * p;
    if (e < SS)
      V[e] = ddp::terminalEntry<S>(a.Qf_d, e / S, e - (e / S) * S);
  }
  {
    const float* Ak = a.A_d + (size_t)(T - 2) * SS;
    const float* Bk = a.B_d + (size_t)(T - 2) * SC;
#pragma unroll
    for (int p = 0; p < PF; p++)
      if (lane + 64 * p < NF)
        F[lane + 64 * p] = ddp::fEntry<S, C>(Ak, Bk, dt, fi[p], fj[p]);
  }
  ddpPhaseSync();

  int failed = -1;
  for (int k = T - 2; k >= 0; k--)
  {
    // the next step's Jacobians: in flight until the last phase of this step
    float raw[PF];
    {
      const int kn = max(k - 1, 0);
      const float* An = a.A_d + (size_t)kn * SS;
      const float* Bn = a.B_d + (size_t)kn * SC;
#pragma unroll
      for (int p = 0; p < PF; p++)
        raw[p] = fj[p] < S ? An[fi[p] * S + fj[p]] : Bn[fi[p] * C + (fj[p] - S)];
    }

#pragma unroll
    for (int p = 0; p < PF; p++)
      if (lane + 64 * p < NF)
        W[lane + 64 * p] = ddp::wEntry<S, C>(V, F, fi[p], fj[p]);
    ddpPhaseSync();

#pragma unroll
    for (int p = 0; p < PQ; p++)
      if (lane + 64 * p < NQ)
        Qm[qr[p] * N + qc[p]] = ddp::qEntry<S, C>(F, W, qcost[p], qr[p], qc[p]);
    ddpPhaseSync();

    float L[C * C], d[C];
    if (!ddp::ldlt<S, C>(Qm, L, d))  // wave-uniform: every lane factorises the same quu
    {
      failed = k;
      break;
    }
    if (lane < S)
    {
      float x[C];
      ddp::gainColumn<S, C>(Qm, L, d, lane, x);
#pragma unroll
      for (int c = 0; c < C; c++)
      {
        Lk[c * S + lane] = x[c];
        a.gains_d[((size_t)k * S + lane) * C + c] = x[c];
      }
    }
    ddpPhaseSync();

#pragma unroll
    for (int p = 0; p < PV; p++)
    {
      const int e = lane + 64 * p;
      if (e < SS)
        V[e] = ddp::vEntry<S, C>(Qm, Lk, e / S, e - (e / S) * S);
    }
#pragma unroll
    for (int p = 0; p < PF; p++)
      if (lane + 64 * p < NF)
        F[lane + 64 * p] = ddp::fValue<S>(raw[p], dt, fi[p], fj[p]);
    ddpPhaseSync();
  }
  if (lane == 0)
  {
    a.status_d[0] = failed < 0 ? 1 : 0;
    a.status_d[1] = failed;
  }
}

}  // namespace kernels
}  // namespace mppi

#endif
