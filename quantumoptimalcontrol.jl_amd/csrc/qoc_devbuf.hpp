// qoc_devbuf.hpp — the owning buffer behind every device allocation of the library, and the byte ledger the counted ones
// report to (qoc_get_info's info[3]).  Host only; knows nothing of qoc_ctx or of streams: a caller drains whatever may
// still read a buffer before it grows or releases it.
//
// A buffer is either valid (pointer and size as allocated) or empty (null, 0 bytes), after every operation and
// whichever way the allocation went; the ledger is at all times the sum of the live counted buffers that report to it.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <vector>

namespace qoc {

class DevBufBase;

struct DevLedger {
  size_t bytes = 0;               // Σ bytes() of the live counted buffers
  std::vector<DevBufBase*> bufs;  // every buffer made with this ledger, counted or not
  inline void release_all();
};

enum DevCount { kUncounted = 0, kCounted = 1 };

class DevBufBase {
 public:
  DevBufBase() = default;  // an uncounted local: freed at scope exit unless a member adopts it
  // host_flags >= 0: pinned host memory (hipHostMalloc with these flags) instead of device memory
  DevBufBase(DevLedger& ledger, DevCount counted, int host_flags = -1)
      : led_(&ledger), counted_(counted == kCounted), host_flags_(host_flags) {
    ledger.bufs.push_back(this);
  }
  DevBufBase(const DevBufBase&) = delete;
  DevBufBase& operator=(const DevBufBase&) = delete;
  ~DevBufBase() {
    release();
    if (led_) led_->bufs.erase(std::remove(led_->bufs.begin(), led_->bufs.end(), this), led_->bufs.end());
  }

  size_t bytes() const { return n_; }
  template <typename U>
  U* as() const {  // the void buffers' element pointer
    return static_cast<U*>(p_);
  }

  // exactly n bytes, whatever was there (freed first, nothing copied); on failure empty, HIP's last error cleared
  hipError_t alloc(size_t n) {
    release();
    if (!n) return hipSuccess;
    void* p = nullptr;
    const hipError_t e = host_flags_ < 0 ? hipMalloc(&p, n) : hipHostMalloc(&p, n, (unsigned)host_flags_);
    if (e != hipSuccess || !p) {
      (void)hipGetLastError();
      return e != hipSuccess ? e : hipErrorOutOfMemory;
    }
    take(p, n);
    return hipSuccess;
  }
  // at least n bytes: as it is when it already has them, else alloc(n)
  hipError_t grow(size_t n) { return n <= n_ ? hipSuccess : alloc(n); }
  void release() {
    if (!p_) return;
    if (host_flags_ < 0)
      (void)hipFree(p_);
    else
      (void)hipHostFree(p_);
    if (counted_) led_->bytes -= n_;
    p_ = nullptr;
    n_ = 0;
  }
  // takes over what o holds (same kind of memory), releasing what was here; o is left empty
  void adopt(DevBufBase&& o) {
    if (&o == this) return;
    release();
    void* p = o.p_;
    const size_t n = o.n_;
    if (o.counted_ && p) o.led_->bytes -= n;
    o.p_ = nullptr;
    o.n_ = 0;
    if (p) take(p, n);
  }

 protected:
  void take(void* p, size_t n) {
    p_ = p;
    n_ = n;
    if (counted_) led_->bytes += n;
  }
  void* p_ = nullptr;
  size_t n_ = 0;
  DevLedger* led_ = nullptr;
  bool counted_ = false;
  int host_flags_ = -1;
};

inline void DevLedger::release_all() {
  for (DevBufBase* b : bufs) b->release();
}

template <typename T>
class DevBuf : public DevBufBase {
 public:
  using DevBufBase::DevBufBase;
  operator T*() const { return static_cast<T*>(p_); }
};

}  // namespace qoc
