/**
 * merge_wave.hpp — the arithmetic of the softmin merge for ONE wave, shared by the merge kernel (csrc/reduce_kernels.hpp:
 * combineWave) and by the rollout kernel that merges the PREVIOUS iteration's block records itself while it samples
 * (engine/rollout_pipeline_kernel.hpp, STREAM_MERGE) — one definition, so that both produce the same bits.
 *
 * Lane l of the wave owns records l, l + 64, l + 128, l + 192 (MERGE_LANE_RECORDS = 4: up to 256 records).  Merge rule
 * (SURVEY.md §8e): rho = min_b rho_b; s_b = exp(-(rho_b - rho)/lambda); eta = sum_b s_b eta_b (double);
 * U[j] = sum_b s_b U_b[j]; u*[j] = U[j] / float(eta).  The sums over a lane's records run in ascending order, the sums over the
 * lanes through the DPP all-reduces of wave_ops.hpp (every lane, wave, block and rank gets the same bits).
 */
#ifndef MPPI_AMD_ENGINE_MERGE_WAVE_HPP_
#define MPPI_AMD_ENGINE_MERGE_WAVE_HPP_

#include <hip/hip_runtime.h>
#include <math.h>
#include "mppi_amd/det_math.h"
#include "mppi_amd/utils/wave_ops.hpp"

namespace mppi
{
namespace kernels
{
constexpr int MERGE_COLS = 4;          ///< columns of u* per wave (and per load: one 16-byte quad)
constexpr int MERGE_LANE_RECORDS = 4;  ///< records a lane keeps in registers: up to 256 records without a second pass

/** a record whose rollouts all cost +inf has rho_b = inf and U_b = eta_b = 0: scale 0 (inf - inf would be NaN when the global
 *  minimum is inf as well — then nothing has weight, as with the reference's global baseline) */
__device__ inline float mergeScale(const float rho_b, const float rho, const float lambda_inv)
{
  const float dist = rho_b - rho;
  return (dist == dist) ? mppi::det::exp(-lambda_inv * dist) : 0.0f;
}

/**
 * p / q for MANY p and ONE q (the merged columns over the normaliser): det::div_benign's Newton-Raphson core with the divisor's
 * part — v_rcp_f32 seed and its refinement — computed once (mergeDivisor) instead of with every quotient.  What a quotient
 * keeps is y = p r and the two corrections y = fma(fma(-q, y, p), r, y): five instructions (packed: five for two quotients)
 * for the ~12 of the compiler's expansion of `/`, and the same correctly rounded bits, as long as no operand needs the
 * expansion's scaling or fix-up.  That is the guard: both |q| and |p| have their biased exponent in
 * [MERGE_Q_EXP_LO, MERGE_Q_EXP_HI], i.e. lie in [2^-60, 2^60) (div_benign's range; it keeps y, the residuals and r normal).
 * Anything else — zeros of either sign, subnormals, infinities, NaNs, far-out magnitudes — is the IEEE division itself, so a
 * -0 quotient keeps its sign and a NaN its payload.  The host build is `/` throughout.
 * tests/test_sampler_trip_exact.py holds the arithmetic (restated in fmaf) and the device code to `/`, bit for bit.
 */
constexpr unsigned MERGE_Q_EXP_LO = 127 - 60, MERGE_Q_EXP_HI = 127 + 59;
struct MergeDivisor
{
  float q;      ///< the divisor
  float r;      ///< its refined reciprocal (device; unused on the host)
  int benign;   ///< q is inside the guard's range
};
__host__ __device__ inline bool mergeQuotientBenign(const float x)
{
  const unsigned e = (mppi::det::f2u(x) >> 23) & 0xffu;
  return e - MERGE_Q_EXP_LO <= MERGE_Q_EXP_HI - MERGE_Q_EXP_LO;
}
/** the divisor's side of the guard.  A significand of all ones is the one divisor whose refined reciprocal a seed 1 ulp off
 *  (v_rcp_f32's specification) can leave wrongly rounded — 1 / q sits just above a rounding tie there, the exception of
 *  Markstein's theorem on this iteration — and the last correction needs it right: such a q takes `/` */
__host__ __device__ inline bool mergeDivisorBenign(const float q)
{
  return mergeQuotientBenign(q) && (mppi::det::f2u(q) & 0x007fffffu) != 0x007fffffu;
}
__host__ __device__ inline MergeDivisor mergeDivisor(const float q)
{
  MergeDivisor d;
  d.q = q;
  d.benign = mergeDivisorBenign(q);
#if defined(__HIP_DEVICE_COMPILE__)
  const float r = __builtin_amdgcn_rcpf(q);
  d.r = mppi::det::fma(mppi::det::fma(-q, r, 1.0f), r, r);
#else
  d.r = 0.0f;
#endif
  return d;
}
/** out[c] = p[c] / d.q for the MERGE_COLS columns of a quad.  The p are wave-uniform where this is called (results of the DPP
 *  all-reduces), so the guard is ONE wave-uniform branch for the quad: either all four take the core — as two packed pairs
 *  (v_pk_mul_f32 / v_pk_fma_f32) — or all four take `/`. */
__host__ __device__ inline void mergeQuotients(const float (&p)[MERGE_COLS], const MergeDivisor& d, float (&out)[MERGE_COLS])
{
#if defined(__HIP_DEVICE_COMPILE__)
  static_assert(MERGE_COLS == 4, "two packed pairs");
  bool slow = d.benign == 0;
#pragma unroll
  for (int c = 0; c < MERGE_COLS; c++)
    slow = slow || !mergeQuotientBenign(p[c]);
  if (__builtin_amdgcn_ballot_w64(slow) == 0)
  {
    typedef float f32x2 __attribute__((ext_vector_type(2)));
    const f32x2 q = { d.q, d.q }, r = { d.r, d.r };
#pragma unroll
    for (int h = 0; h < MERGE_COLS; h += 2)
    {
      const f32x2 pp = { p[h], p[h + 1] };
      f32x2 y = pp * r;
      y = __builtin_elementwise_fma(__builtin_elementwise_fma(-q, y, pp), r, y);
      y = __builtin_elementwise_fma(__builtin_elementwise_fma(-q, y, pp), r, y);
      out[h] = y.x;
      out[h + 1] = y.y;
    }
    return;
  }
#endif
#pragma unroll
  for (int c = 0; c < MERGE_COLS; c++)
    out[c] = p[c] / d.q;
}
/** one quotient, the same guard and the same core (tests: mppi_det_eval) */
__host__ __device__ inline float mergeQuotient(const float p, const MergeDivisor& d)
{
#if defined(__HIP_DEVICE_COMPILE__)
  if (d.benign && mergeQuotientBenign(p))
  {
    float y = p * d.r;
    y = mppi::det::fma(mppi::det::fma(-d.q, y, p), d.r, y);
    y = mppi::det::fma(mppi::det::fma(-d.q, y, p), d.r, y);
    return y;
  }
#endif
  return p / d.q;
}

/** what the tails of the records give: the global baseline, this lane's scale factors, the normaliser (wave-uniform) */
struct MergeTails
{
  float rho;
  float s[MERGE_LANE_RECORDS];
  double eta, eta2;
  float eta_f;
  // eta_f prepared for mergeQuotients (fixed for the launch once the tails are merged): mergeDivisor()'s r and benign, kept as
  // plain members like the rest — as a MergeDivisor inside this struct they went through scratch in rolloutPipelineKernel
  float eta_r;
  int eta_benign;
  __host__ __device__ inline MergeDivisor etaDivisor() const
  {
    MergeDivisor d;
    d.q = eta_f;
    d.r = eta_r;
    d.benign = eta_benign;
    return d;
  }
};

/** rho_b / eta_b / eta2_b: the lane's records' tails (padding records: rho_b = inf, eta_b = eta2_b = 0).
 *  WITH_ETA2 = false: a wave that does not write the statistics skips the sum of w^2 and its all-reduce in double (out.eta2 = 0);
 *  rho, the scale factors and eta are the same instructions on the same data either way. */
template <bool WITH_ETA2 = true>
__device__ inline void mergeTails(const float (&rho_b)[MERGE_LANE_RECORDS], const float (&eta_b)[MERGE_LANE_RECORDS],
                                  const float (&eta2_b)[MERGE_LANE_RECORDS], const float lambda_inv, MergeTails& out)
{
  float m = rho_b[0];
#pragma unroll
  for (int i = 1; i < MERGE_LANE_RECORDS; i++)
    m = fminf(m, rho_b[i]);
  out.rho = mppi::wave::waveAllMin(m);
  double eta = 0.0, eta2 = 0.0;
#pragma unroll
  for (int i = 0; i < MERGE_LANE_RECORDS; i++)
  {
    const float s = mergeScale(rho_b[i], out.rho, lambda_inv);  // 0 for the padding records
    out.s[i] = s;
    eta += (double)s * (double)eta_b[i];
    if (WITH_ETA2)
      eta2 += (double)s * (double)s * (double)eta2_b[i];
  }
  out.eta = mppi::wave::waveAllSum(eta);
  out.eta2 = WITH_ETA2 ? mppi::wave::waveAllSum(eta2) : 0.0;
  out.eta_f = (float)out.eta;
  const MergeDivisor d = mergeDivisor(out.eta_f);
  out.eta_r = d.r;
  out.eta_benign = d.benign;
}

/** tot[c] = sum over all records of s_b U_b[col0 + c]; v[i][c]: the lane's records' column values (0 for padding) */
__device__ inline void mergeColumns(const float (&s)[MERGE_LANE_RECORDS], const float (&v)[MERGE_LANE_RECORDS][MERGE_COLS],
                                    float (&tot)[MERGE_COLS])
{
  float acc[MERGE_COLS];
#pragma unroll
  for (int c = 0; c < MERGE_COLS; c++)
    acc[c] = 0.0f;
#pragma unroll
  for (int i = 0; i < MERGE_LANE_RECORDS; i++)
#pragma unroll
    for (int c = 0; c < MERGE_COLS; c++)
      acc[c] += s[i] * v[i][c];
#pragma unroll
  for (int c = 0; c < MERGE_COLS; c++)
    tot[c] = mppi::wave::waveAllSum(acc[c]);
}

/** statistics block of a finished merge, [STATS_STRIDE = 8] floats: baseline, normaliser, free energy and its variance terms
 *  (reference: mppi_common.cu:1065-1081 computeFreeEnergy).  st[6] — the exchange-failure mark (a bounded wait that ran out) —
 *  is STICKY: no kernel clears it, so that a later successful merge cannot erase it before the host has looked; it is not
 *  written here.  One definition for the merge kernel and the merging control phase (finalize_kernel.hpp: mergeControlKernel). */
__device__ inline void mergeStatistics(const float rho, const float eta_f, const double eta2, const float lambda,
                                       const int num_rollouts_total, float* st)
{
  const float K = (float)num_rollouts_total;
  const float norm = eta_f / K;
  const float var = (float)eta2;
  const float fe = -lambda * mppi::det::log(norm) + rho;
  const float fe_var = lambda * (var / K - norm * norm);
  const float weird = fe_var / (norm * mppi::det::sqrt(K));
  st[0] = rho;
  st[1] = eta_f;
  st[2] = fe;
  st[3] = fe_var;
  st[4] = lambda * (weird + 0.5f * (weird * weird));
  st[5] = var;
  st[7] = 0.0f;
}
}  // namespace kernels
}  // namespace mppi

#endif
