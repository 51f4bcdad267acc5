/**
 * model_launch.hpp — the one path every kernel launch of ModelT (model_instance.hpp) takes, and what a launch site needs next to
 * it: the LDS size of a block, the refusal of a request beyond it, what a launch family asks of a block (BlockPlan), and the
 * compile-time block shape lists with the one walk over them (forShape).
 */
#ifndef MPPI_AMD_MODEL_LAUNCH_HPP_
#define MPPI_AMD_MODEL_LAUNCH_HPP_

#include <hip/hip_runtime.h>
#include <map>
#include <mutex>
#include <string>
#include <utility>

#include "mppi_amd.h"

/**
 * hipFuncAttributeMaxDynamicSharedMemorySize of a kernel, raised only when a launch needs more than was granted before: the
 * attribute call is a runtime round trip (function lookup, locks) that every rollout launch of a > 48 KiB block paid in front of
 * its dispatch — on the host's critical path of mppi_compute_control, where the first launch's enqueue time decides when the
 * device starts.  The grant is per (device, kernel) and monotonic, so handles sharing a kernel on a device never lower each
 * other's limit.
 */
inline hipError_t ensureDynamicLds(const void* fn, size_t smem)
{
  if (smem <= 48 * 1024)
    return hipSuccess;
  static std::mutex mu;
  static std::map<std::pair<int, const void*>, size_t> granted;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  size_t& g = granted[std::make_pair(dev, fn)];
  if (smem <= g)
    return hipSuccess;
  const hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)smem);
  if (e == hipSuccess)
    g = smem;
  return e;
}

namespace mppi
{
namespace engine
{
constexpr size_t MAX_LDS_BYTES = 160 * 1024;  // gfx950: 160 KiB per CU, one workgroup may take all of it

template <int X, int Y, int Z>
struct Shape
{
  static constexpr int x = X, y = Y, z = Z;
};
template <class... S>
struct Shapes
{
};
/** f(Shape<X, Y, Z>{}) for the shapes of a list, in its order, until a call returns true; false: none did */
template <class... S, class F>
inline bool anyShape(Shapes<S...>, F&& f)
{
  return (f(S{}) || ...);
}
/** for the shape of the list equal to (bx, by, bz): f(Shape<X, Y, Z>{}), X, Y, Z compile-time through its type; false: no such shape */
template <class LIST, class F>
inline bool forShape(LIST list, int bx, int by, int bz, F&& f)
{
  return anyShape(list, [&](auto s) {
    if (bx != s.x || by != s.y || bz != s.z)
      return false;
    f(s);
    return true;
  });
}

/** what a launch family asks of a block, from the one function both the LDS query and the launch go through: LDS bytes, threads,
 *  rollouts per block and, for the role-pipelined families, the ring(s) — none (0 steps) when not even the shortest fits */
template <class RING = int>
struct BlockPlan
{
  size_t smem;
  dim3 block;
  int rollouts;
  RING ring;
  dim3 grid(int num_rollouts) const
  {
    return dim3((num_rollouts + rollouts - 1) / rollouts);
  }
};

/** a launch function's refusal: the reason into `err`, the status back */
inline mppi_status refuse(mppi_status st, const char* why, std::string& err)
{
  err = why;
  return st;
}
/** "<what> needs N B of LDS per block; gfx950 has 163840" */
inline mppi_status ldsOverflow(const char* what, size_t smem, std::string& err)
{
  err = std::string(what) + " needs " + std::to_string(smem) + " B of LDS per block; gfx950 has " + std::to_string(MAX_LDS_BYTES);
  return MPPI_ERR_LDS_OVERFLOW;
}

/**
 * The tail of every launch site, after it has picked the kernel: the dynamic-LDS limit (ensureDynamicLds), the launch, and the
 * launch's own error as "<what> launch: ...".  These launches sit on mppi_compute_control's host critical path: nothing is
 * allocated unless something failed (`what` is a literal, the message is built on failure only).
 */
template <class KFN, class... ARGS>
inline mppi_status launchChecked(const char* what, KFN kfn, dim3 grid, dim3 block, size_t smem, hipStream_t stream,
                                 std::string& err, const ARGS&... args)
{
  hipError_t e = ensureDynamicLds(reinterpret_cast<const void*>(kfn), smem);
  if (e != hipSuccess)
  {
    err = std::string("hipFuncSetAttribute(MaxDynamicSharedMemorySize): ") + hipGetErrorString(e);
    return MPPI_ERR_HIP;
  }
  hipLaunchKernelGGL(kfn, grid, block, smem, stream, args...);
  e = hipGetLastError();
  if (e != hipSuccess)
  {
    err = std::string(what) + " launch: " + hipGetErrorString(e);
    return MPPI_ERR_HIP;
  }
  return MPPI_OK;
}

}  // namespace engine
}  // namespace mppi

#endif
