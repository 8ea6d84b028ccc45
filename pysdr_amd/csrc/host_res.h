// Owners of what the host half of libpysdr_hip.so (api.hip, api_objects.hip, api_cw.hip, api_psk.hip, api_fine.hip) holds on the device: typed device and pinned-host buffers,
// streams, events, and the two buffers of a pair that overlapped calls alternate between.  Move-only; the destructors
// free and nothing else does, so a struct of these needs no free list.  Plain C++ over the HIP runtime API.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>

namespace pysdr {

namespace detail {
struct DeviceMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipMalloc(p, bytes); }
  static hipError_t free(void* p) { return hipFree(p); }
};
struct PinnedMem {
  static hipError_t alloc(void** p, size_t bytes) { return hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static hipError_t free(void* p) { return hipHostFree(p); }
};
}  // namespace detail

// n elements of T in device (DevBuf) or pinned host (PinnedBuf) memory
template <class T, class Mem>
class Buf {
 public:
  Buf() = default;
  Buf(const Buf&) = delete;
  Buf& operator=(const Buf&) = delete;
  Buf(Buf&& o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
  Buf& operator=(Buf&& o) noexcept {
    if (this != &o) { (void)reset(); p_ = o.p_; n_ = o.n_; o.p_ = nullptr; o.n_ = 0; }
    return *this;
  }
  ~Buf() { (void)reset(); }

  hipError_t alloc(size_t n) {                       // (whatever it held goes first)
    hipError_t e = reset();
    if (e != hipSuccess) return e;
    void* p = nullptr;
    e = Mem::alloc(&p, n * sizeof(T));
    if (e != hipSuccess) return e;
    p_ = static_cast<T*>(p); n_ = n;
    return hipSuccess;
  }
  hipError_t alloc_zeroed(size_t n, hipStream_t st) {
    const hipError_t e = alloc(n);
    return e != hipSuccess ? e : hipMemsetAsync(p_, 0, n * sizeof(T), st);
  }
  // at least n elements: frees and reallocates (contents lost) only when too small, and says so
  hipError_t grow(size_t n, bool* grew = nullptr) {
    if (grew) *grew = n_ < n;
    return n_ < n ? alloc(n) : hipSuccess;
  }
  hipError_t reset() {
    const hipError_t e = p_ ? Mem::free(p_) : hipSuccess;
    p_ = nullptr; n_ = 0;
    return e;
  }
  T* get() const { return p_; }
  size_t size() const { return n_; }
  explicit operator bool() const { return p_ != nullptr; }

 private:
  T* p_ = nullptr;
  size_t n_ = 0;
};
template <class T> using DevBuf = Buf<T, detail::DeviceMem>;
template <class T> using PinnedBuf = Buf<T, detail::PinnedMem>;

template <class H, hipError_t (*Destroy)(H)>
class Handle {
 public:
  Handle() = default;
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; }
    return *this;
  }
  ~Handle() { reset(); }
  void reset() { if (h_) (void)Destroy(h_); h_ = nullptr; }
  H get() const { return h_; }
  operator H() const { return h_; }                  // passed straight to the runtime and the launch layer
  explicit operator bool() const { return h_ != nullptr; }

 protected:
  H h_ = nullptr;
};

class Stream : public Handle<hipStream_t, hipStreamDestroy> {
 public:
  hipError_t create(unsigned flags = hipStreamNonBlocking) { reset(); return hipStreamCreateWithFlags(&h_, flags); }
  hipError_t create(unsigned flags, int priority) { reset(); return hipStreamCreateWithPriority(&h_, flags, priority); }
};

class Event : public Handle<hipEvent_t, hipEventDestroy> {
 public:
  hipError_t create() { reset(); return hipEventCreate(&h_); }                                    // with timing
  hipError_t create(unsigned flags) { reset(); return hipEventCreateWithFlags(&h_, flags); }
};

// Two buffers of equal size that calls alternate between: `first` exists once allocated, `second` comes into being on
// demand.  Storage and selection only -- WHICH index is current (the context's par, a decimator's hist_cur, the call
// counter of the raw peaks) is the owner's business and is passed in.
template <class T>
struct BufPair {
  DevBuf<T> first, second;

  explicit operator bool() const { return (bool)first; }
  bool has_second() const { return (bool)second; }
  bool lacks_second() const { return first && !second; }
  T* buf(int i) const { return i ? second.get() : first.get(); }
  T* cur(int par) const { return buf(par); }                                      // this call's buffer
  T* next(int par, bool use2) const { return buf(use2 ? (par ^ 1) : par); }        // the next call's: the other one when the calls overlap

  hipError_t alloc_both_zeroed(size_t n, hipStream_t st) {
    const hipError_t e = first.alloc_zeroed(n, st);
    return e != hipSuccess ? e : second.alloc_zeroed(n, st);
  }
  hipError_t alloc_second() { return second.alloc(first.size()); }                 // unfilled (a buffer every call writes before it reads)
  // The second buffer, zeroed on `st`.  One that comes into being while it is the CURRENT buffer (par != 0: a mode first
  // used after overlapped calls left par at 1) inherits the first `prefix_elems` elements of the first, which is where
  // that mode's last use left its history.
  hipError_t ensure_second(hipStream_t st, int par, size_t prefix_elems) {
    if (second) return hipSuccess;
    hipError_t e = second.alloc_zeroed(first.size(), st);
    if (e == hipSuccess && par != 0 && prefix_elems > 0)
      e = hipMemcpyAsync(second.get(), first.get(), prefix_elems * sizeof(T), hipMemcpyDeviceToDevice, st);
    return e;
  }
};

}  // namespace pysdr
