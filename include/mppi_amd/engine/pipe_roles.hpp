/**
 * pipe_roles.hpp — what the role waves of the pipelined rollout kernels share (rollout_pipeline_kernel.hpp,
 * rmppi_pipeline_kernel.hpp): the progress counters in LDS that couple sampler, dynamics and cost waves, the in-kernel
 * timers of the A/B builds, and the VGPR pin of the cost waves' private copy of the cost plugin.
 */
#ifndef MPPI_AMD_PIPE_ROLES_HPP_
#define MPPI_AMD_PIPE_ROLES_HPP_

#include <hip/hip_runtime.h>
#include <cstdint>

namespace mppi
{
namespace kernels
{
/** progress counters live in LDS: address-space-3 pointers keep the polls on ds_read instead of flat loads */
typedef volatile __attribute__((address_space(3))) int* lds_counter_t;
typedef int pipe_int4 __attribute__((ext_vector_type(4)));
typedef volatile __attribute__((address_space(3))) pipe_int4* lds_counter4_t;

/**
 * Blocks until *ctr >= need.  `cached` is the consumer's last observed value: the producer usually runs ahead, so most
 * calls return without touching LDS.
 */
__device__ inline void pipeWait(lds_counter_t ctr, const int need, int& cached)
{
  if (cached >= need)
    return;
  int v = __builtin_amdgcn_readfirstlane(*ctr);
  while (v < need)
  {
    __builtin_amdgcn_s_sleep(1);
    v = __builtin_amdgcn_readfirstlane(*ctr);
  }
  cached = v;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}
__device__ inline void pipePublish(lds_counter_t ctr, const int value, const int lane)
{
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  if (lane == 0)
    *ctr = value;
}
/**
 * pipePublish for a producer whose data went to LDS ONLY (ring slots, LDS sample rows).  The LDS unit executes the DS
 * instructions of a wave in issue order (that order is what lgkmcnt counts), so the counter store below cannot become visible
 * before the data stores in front of it: no s_waitcnt is needed, only the compiler must keep the order.  The release fence of
 * pipePublish cost the dynamics wave of rolloutPipelineKernel an exposed LDS write round trip per trip (in-kernel timers,
 * profiles/r04_cartpole_pipe_timing*.json).  NOT for data stored to global memory (the HBM-row variants' sampler waves).
 */
__device__ inline void pipePublishLds(lds_counter_t ctr, const int value, const int lane)
{
  asm volatile("" ::: "memory");
  if (lane == 0)
    *ctr = value;
  asm volatile("" ::: "memory");
}
/* ---- A/B instrumentation (tools/pipe_timing.py; never defined in a product build): where the role waves of
 * rolloutPipelineRepKernel spend their time.  Every wave of the first PIPE_TIMING_BLOCKS blocks accumulates s_memtime ticks
 * (constant 100 MHz on gfx950: 10 ns — coarse per event, unbiased over the hundreds of events of a launch) per category. */
#if defined(MPPI_PIPE_TIMING)
constexpr int PIPE_TIMING_BLOCKS = 256, PIPE_TIMING_WAVES = 24, PIPE_TIMING_SLOTS = 8;
static __device__ unsigned long long g_pipe_timing[PIPE_TIMING_BLOCKS * PIPE_TIMING_WAVES * PIPE_TIMING_SLOTS];
struct PipeTimer
{
  unsigned long long acc[PIPE_TIMING_SLOTS] = {};
  unsigned long long t0 = 0;
  __device__ inline void start()
  {
    t0 = __builtin_amdgcn_s_memtime();
  }
  __device__ inline void stop(const int slot)
  {
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    acc[slot] += t1 - t0;
    t0 = t1;
  }
  /** per-trip record of one wave (the dynamics wave of rolloutPipelineKernel): row 4 + kind of the block's table, entry trip */
  __device__ inline void trip(const int block, const int kind, const int trip_idx, const int lane, const unsigned long long v) const
  {
    if (block < PIPE_TIMING_BLOCKS && lane == 0 && trip_idx < 4 * PIPE_TIMING_SLOTS && kind < 5)
      g_pipe_timing[(block * PIPE_TIMING_WAVES + 4 + 4 * kind) * PIPE_TIMING_SLOTS + trip_idx] = v;
  }
  __device__ inline void flush(const int block, const int wave, const int lane) const
  {
    if (block < PIPE_TIMING_BLOCKS && wave < PIPE_TIMING_WAVES && lane == 0)
      for (int i = 0; i < PIPE_TIMING_SLOTS; i++)
        g_pipe_timing[(block * PIPE_TIMING_WAVES + wave) * PIPE_TIMING_SLOTS + i] = acc[i];
  }
};
#define PIPE_T(x) x
#else
#define PIPE_T(x)
#endif

/** pins every 32-bit word of a (trivially copyable) object to a VGPR: see the cost wave of rolloutPipelineRepKernel */
template <class T>
__device__ inline void vgprResident(T& obj)
{
  static_assert(sizeof(T) % 4 == 0, "whole words");
  uint32_t* w = reinterpret_cast<uint32_t*>(&obj);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 4); i++)
    asm volatile("" : "+v"(w[i]));
}

}  // namespace kernels
}  // namespace mppi

#endif
