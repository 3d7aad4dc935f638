// Owning handles of the engine's GPU resources: device memory, pinned host memory, streams, events.  An object OWNS its handle
// -- null by default, move-only, freed in the destructor -- and converts implicitly to the raw handle, so a launch site or a
// HIP call reads as it would with the raw pointer.  What only looks at memory something else owns stays a raw pointer
// (an object owns or views, never both).  Written over a policy `P` that makes and frees a handle, as
// row_dedup.h is over its atomics: the HIP policies at the end are the only part that needs hip_runtime.h, and a host program
// instantiates the same text with a counting fake (tests/test_hip_owned_cpu.py, under the host sanitizers).
//   error P::create(H* out, args...)   the error type's value-initialised value (hipSuccess) says *out was made, any other
//                                      that it was left alone; a memory policy's H is void*, its first argument the bytes
//   void  P::free(H h)                 gives a non-null handle back
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <atomic>

namespace drs {

// Handles alive in this process, over every engine: one relaxed increment where one is taken, one where it is given back,
// nothing per launch.  The read-only option "live_device_objects" reads it (arena_alloc / arena_free count the table arenas).
inline std::atomic<int64_t> g_live_objects{0};
inline void count_live(int64_t d) { g_live_objects.fetch_add(d, std::memory_order_relaxed); }
inline int64_t live_objects() { return g_live_objects.load(std::memory_order_relaxed); }

template <class H, class P>
class Owned {
 public:
  Owned() = default;
  Owned(const Owned&) = delete;
  Owned& operator=(const Owned&) = delete;
  Owned(Owned&& o) noexcept : h_(o.h_) { o.h_ = H(); }
  Owned& operator=(Owned&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = H(); }
    return *this;
  }
  ~Owned() { reset(); }
  operator H() const { return h_; }
  H get() const { return h_; }
  // frees what is held and takes `h` over (null: holds nothing afterwards)
  void reset(H h = H()) {
    if (h_) { P::free(h_); count_live(-1); }
    if ((h_ = h)) count_live(1);
  }
  // hands the handle to the caller, who frees it
  H release() {
    if (h_) count_live(-1);
    const H h = h_;
    h_ = H();
    return h;
  }
  // frees what is held, then makes a new handle; on failure the object is null
  template <class... A>
  auto create(A... args) {
    reset();
    H h = H();
    const auto r = P::create(&h, args...);
    if (r == decltype(r)()) reset(h);
    return r;
  }

 private:
  H h_ = H();
};

// ... of `count` elements of T (void: bytes), from a memory policy
template <class T, class P>
class Buffer : public Owned<T*, P> {
  template <class U> static size_t elem_bytes(U*) { return sizeof(U); }
  static size_t elem_bytes(void*) { return 1; }

 public:
  template <class... A>
  auto alloc(size_t count, A... args) {
    this->reset();
    void* p = nullptr;
    const auto r = P::create(&p, count * elem_bytes(static_cast<T*>(nullptr)), args...);
    if (r == decltype(r)()) this->reset(static_cast<T*>(p));
    return r;
  }
};

}  // namespace drs

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
namespace drs {
struct HipDeviceMem {
  static hipError_t create(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t create(void** p, size_t bytes, unsigned flags) { return hipExtMallocWithFlags(p, bytes, flags); }
  static void free(void* p) { (void)hipFree(p); }
};
struct HipPinnedMem {
  static hipError_t create(void** p, size_t bytes, unsigned flags) { return hipHostMalloc(p, bytes, flags); }
  static void free(void* p) { (void)hipHostFree(p); }
};
struct HipStream {   // idle before it goes: nothing of the engine is left running on a destroyed queue
  static hipError_t create(hipStream_t* s, unsigned flags) { return hipStreamCreateWithFlags(s, flags); }
  static void free(hipStream_t s) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
};
struct HipEvent {
  static hipError_t create(hipEvent_t* ev) { return hipEventCreate(ev); }
  static hipError_t create(hipEvent_t* ev, unsigned flags) { return hipEventCreateWithFlags(ev, flags); }
  static void free(hipEvent_t ev) { (void)hipEventDestroy(ev); }
};
template <class T> using DeviceBuf = Buffer<T, HipDeviceMem>;
template <class T> using PinnedBuf = Buffer<T, HipPinnedMem>;
using Stream = Owned<hipStream_t, HipStream>;
using Event = Owned<hipEvent_t, HipEvent>;
}  // namespace drs
#endif
