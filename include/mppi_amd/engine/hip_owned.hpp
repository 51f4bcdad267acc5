/**
 * hip_owned.hpp — owners of the engine's HIP resources: memory (HipBuffer), streams (HipStream) and events (HipEvent).
 *
 * Not copyable; a HipBuffer moves.  Allocation returns the hipError_t and never throws, and a failed allocation leaves the
 * owner empty (null, count 0).  alloc*() on an owner that holds memory frees it first (free, then allocate); to keep the old
 * buffer until the new one is ready, allocate into a local owner and move it in.  Nothing is zeroed.  A buffer converts to
 * its pointer implicitly: a hot-path access is the load of one pointer, as with the raw pointer it replaced.
 *
 * Allocating and freeing a HipBuffer — never accessing it — updates a process-wide count of live allocations and their bytes
 * (liveAllocations(), read by mppi_debug_live_allocations).
 */
#ifndef MPPI_AMD_ENGINE_HIP_OWNED_HPP_
#define MPPI_AMD_ENGINE_HIP_OWNED_HPP_

#include <hip/hip_runtime.h>

#include <atomic>
#include <cstddef>
#include <utility>

namespace mppi
{
namespace engine
{
struct LiveAllocations
{
  std::atomic<long long> count{ 0 }, bytes{ 0 };
};
inline LiveAllocations& liveAllocations()
{
  static LiveAllocations live;
  return live;
}

template <class T>
class HipBuffer
{
public:
  HipBuffer() = default;
  HipBuffer(const HipBuffer&) = delete;
  HipBuffer& operator=(const HipBuffer&) = delete;
  HipBuffer(HipBuffer&& o) noexcept
  {
    *this = std::move(o);
  }
  HipBuffer& operator=(HipBuffer&& o) noexcept
  {
    if (this != &o)
    {
      reset();
      p_ = std::exchange(o.p_, nullptr);
      dev_ = std::exchange(o.dev_, nullptr);
      n_ = std::exchange(o.n_, 0);
      host_ = o.host_;
    }
    return *this;
  }
  ~HipBuffer()
  {
    reset();
  }

  /** device memory (hipMalloc) */
  hipError_t alloc(size_t n)
  {
    reset();
    return track(hipMalloc((void**)&p_, n * sizeof(T)), n, false);
  }
  /** device memory with hipExtMallocWithFlags flags (fine-grained BAR inbox, uncached mailbox) */
  hipError_t allocExt(size_t n, unsigned flags)
  {
    reset();
    return track(hipExtMallocWithFlags((void**)&p_, n * sizeof(T), flags), n, false);
  }
  /** host memory (hipHostMalloc): pinned, or mapped into the device (hipHostMallocMapped), dev() then being its device address */
  hipError_t allocHost(size_t n, unsigned flags)
  {
    reset();
    hipError_t e = track(hipHostMalloc((void**)&p_, n * sizeof(T), flags), n, true);
    if (e == hipSuccess && (flags & hipHostMallocMapped))
    {
      e = hipHostGetDevicePointer((void**)&dev_, p_, 0);
      if (e != hipSuccess)
        reset();
    }
    return e;
  }
  /** frees the memory the way it was allocated (hipFree / hipHostFree) and leaves the owner empty */
  void reset()
  {
    if (!p_)
      return;
    (void)(host_ ? hipHostFree(p_) : hipFree(p_));
    liveAllocations().count--;
    liveAllocations().bytes -= (long long)bytes();
    p_ = dev_ = nullptr;
    n_ = 0;
  }

  operator T*() const
  {
    return p_;
  }
  T* get() const  ///< where a template would deduce HipBuffer (std::copy)
  {
    return p_;
  }
  T* dev() const  ///< the address a kernel uses: the pointer itself except for mapped host memory
  {
    return dev_;
  }
  size_t size() const
  {
    return n_;
  }
  size_t bytes() const
  {
    return n_ * sizeof(T);
  }

private:
  hipError_t track(hipError_t e, size_t n, bool host)
  {
    if (e != hipSuccess)
    {
      p_ = nullptr;
      return e;
    }
    dev_ = p_;
    n_ = n;
    host_ = host;
    liveAllocations().count++;
    liveAllocations().bytes += (long long)bytes();
    return e;
  }
  T* p_ = nullptr;
  T* dev_ = nullptr;
  size_t n_ = 0;
  bool host_ = false;
};

/** a stream or an event the owner created and destroys — or, adopt(), a caller's stream it uses and never destroys */
template <class H, hipError_t (*CREATE)(H*, unsigned), hipError_t (*DESTROY)(H)>
class HipHandle
{
public:
  HipHandle() = default;
  HipHandle(const HipHandle&) = delete;
  HipHandle& operator=(const HipHandle&) = delete;
  ~HipHandle()
  {
    reset();
  }
  hipError_t create(unsigned flags)
  {
    reset();
    const hipError_t e = CREATE(&h_, flags);
    own_ = e == hipSuccess;
    if (!own_)
      h_ = nullptr;
    return e;
  }
  void adopt(H h)
  {
    reset();
    h_ = h;
  }
  void reset()
  {
    if (own_)
      (void)DESTROY(h_);
    h_ = nullptr;
    own_ = false;
  }
  operator H() const
  {
    return h_;
  }
  bool owned() const
  {
    return own_;
  }

private:
  H h_ = nullptr;
  bool own_ = false;
};
using HipStream = HipHandle<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;
using HipEvent = HipHandle<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
}  // namespace engine
}  // namespace mppi

#endif
