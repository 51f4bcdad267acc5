/**
 * top_rollouts_kernel.hpp — the n lowest-cost rollouts of an iteration, selected on the device (mppi_top_rollouts).
 *
 * The reference keeps the best rollouts in a host list it walks over the K weights (controllers/controller.cu:126-179,
 * getTopNCosts / the top-N part of calculateSampledStateTrajectories); here the K costs never leave the device: one block reads
 * trajectory_costs_d where the rollout kernel left it and writes n indices and n costs.
 *
 * Order: ascending cost, ties to the lower index, NaN after every number (+inf included).  Made total by the key
 *   key(i) = orderedBits(cost[i]) << 32 | i
 * where orderedBits maps a float to an unsigned word of the same order (sign bit flipped for positive values, all bits for
 * negative ones; -0 counts as +0; every NaN maps to the largest word).  The index in the low word makes the keys of one launch
 * distinct, so "the n smallest keys" is exactly n rollouts and ties need no second pass.
 *
 *   1. radix select of the n-th smallest key: eight passes, one per 8-bit digit from the top; a pass counts the keys that share
 *      the digits found so far into a 256-bin LDS histogram (LDS atomics), a 256-lane scan finds the bin the n-th key falls into;
 *   2. compaction: every key <= the n-th one takes a slot of an LDS array (at most 256 of them: n <= TOP_ROLLOUTS_MAX);
 *   3. rank sort of the survivors in LDS (rank = number of smaller survivors — the keys are distinct), write-out.
 *
 * One block, no global atomics, no waiting on anything: every loop is bounded by K, by n or by a constant.  The costs are re-read
 * from global memory in every pass (K floats, L2-resident: 64 KB at K = 16384).
 */
#ifndef MPPI_AMD_ENGINE_TOP_ROLLOUTS_KERNEL_HPP_
#define MPPI_AMD_ENGINE_TOP_ROLLOUTS_KERNEL_HPP_

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mppi
{
namespace kernels
{
constexpr int TOP_ROLLOUTS_MAX = 256;       ///< largest n of one selection (the survivors are sorted in LDS)
constexpr int TOP_ROLLOUTS_THREADS = 1024;  ///< the one block of the launch

/** float -> unsigned word of the same order; NaN -> 0xFFFFFFFF (behind +inf = 0xFF800000), -0 -> the word of +0 */
__host__ __device__ inline uint32_t topRolloutsOrderedBits(const float f)
{
  if (f != f)
    return 0xFFFFFFFFu;
  if (f == 0.0f)
    return 0x80000000u;
  union
  {
    float f;
    uint32_t u;
  } c;
  c.f = f;
  return (c.u & 0x80000000u) ? ~c.u : (c.u | 0x80000000u);
}
__host__ __device__ inline uint64_t topRolloutsKey(const float cost, const int index)
{
  return ((uint64_t)topRolloutsOrderedBits(cost) << 32) | (uint32_t)index;
}

/** costs_d[K] -> idx_d[n], cost_d[n]; 1 <= n <= min(K, TOP_ROLLOUTS_MAX) (the caller checks).  grid = 1, block = TOP_ROLLOUTS_THREADS */
__global__ void __launch_bounds__(TOP_ROLLOUTS_THREADS)
    topRolloutsKernel(const float* __restrict__ costs_d, const int K, const int n, int* __restrict__ idx_d, float* __restrict__ cost_d)
{
  constexpr int NT = TOP_ROLLOUTS_THREADS;
  __shared__ unsigned hist[256];
  __shared__ unsigned scan[2][256];
  __shared__ unsigned sel[2];  // the digit the n-th key has in this pass, its rank among the keys of that bin
  __shared__ unsigned count;
  __shared__ uint64_t surv[TOP_ROLLOUTS_MAX];
  const int tid = (int)threadIdx.x;

  uint64_t prefix = 0;         // the digits of the n-th key found so far (block-uniform)
  unsigned remaining = (unsigned)n;  // rank (1-based) of the n-th key among the keys that share them
  for (int pass = 0; pass < 8; pass++)
  {
    const int shift = 56 - 8 * pass;
    if (tid < 256)
      hist[tid] = 0;
    __syncthreads();
    for (int i = tid; i < K; i += NT)
    {
      const uint64_t key = topRolloutsKey(costs_d[i], i);
      // (shift + 8 == 64 in the first pass: every key shares the empty prefix)
      if (pass == 0 || (key >> (shift + 8)) == prefix)
        atomicAdd(&hist[(unsigned)(key >> shift) & 0xFFu], 1u);
    }
    __syncthreads();
    // inclusive scan of the 256 bins (Hillis-Steele, eight rounds, two buffers)
    if (tid < 256)
      scan[0][tid] = hist[tid];
    __syncthreads();
    int src = 0;
    for (int d = 1; d < 256; d <<= 1)
    {
      if (tid < 256)
        scan[src ^ 1][tid] = scan[src][tid] + (tid >= d ? scan[src][tid - d] : 0u);
      src ^= 1;
      __syncthreads();
    }
    if (tid < 256)
    {
      const unsigned incl = scan[src][tid], excl = incl - hist[tid];
      if (excl < remaining && remaining <= incl)  // exactly one bin: the counts sum to at least `remaining`
      {
        sel[0] = (unsigned)tid;
        sel[1] = remaining - excl;
      }
    }
    __syncthreads();
    prefix = (prefix << 8) | sel[0];
    remaining = sel[1];
    __syncthreads();  // sel is rewritten by the next pass
  }
  // prefix is the n-th smallest key; the keys are distinct: exactly n of them are <= prefix
  if (tid == 0)
    count = 0;
  __syncthreads();
  for (int i = tid; i < K; i += NT)
  {
    const uint64_t key = topRolloutsKey(costs_d[i], i);
    if (key <= prefix)
    {
      const unsigned slot = atomicAdd(&count, 1u);
      if (slot < (unsigned)TOP_ROLLOUTS_MAX)
        surv[slot] = key;
    }
  }
  __syncthreads();
  const int m = min((int)count, min(n, TOP_ROLLOUTS_MAX));
  if (tid < m)
  {
    const uint64_t mine = surv[tid];
    int rank = 0;
    for (int j = 0; j < m; j++)
      rank += surv[j] < mine ? 1 : 0;
    const int index = (int)(uint32_t)mine;
    if (idx_d)
      idx_d[rank] = index;
    if (cost_d)
      cost_d[rank] = costs_d[index];
  }
}

}  // namespace kernels
}  // namespace mppi

#endif
