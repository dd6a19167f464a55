// Move-only owners of the host layer's GPU resources: device buffer (with capacity), pinned buffer,
// event, stream.  A handle is empty, owning (released exactly once: on destruction, reset, a new
// allocation or a move-assignment onto it) or borrowed (a caller's pointer or stream: never
// released).  Every release call of the host layer is in this header.
//
// The runtime calls come from the `Api` template parameter, so a host check can substitute a
// counting fake (tests/native/slot_policy_check.cpp defines MPPI_HANDLES_NO_HIP and includes no HIP
// header).  Api's functions return 0 on success and the runtime's error code otherwise.
#pragma once
#include <cstddef>
#include <utility>

#ifndef MPPI_HANDLES_NO_HIP
#include <hip/hip_runtime.h>
#endif

namespace mppi {

// The resource value `H` (a pointer type), released by Rel::release when owned.  Reads like the raw
// pointer it replaces (implicit conversion); only the handle can free it.
template <class H, class Rel>
class Handle {
 public:
  Handle() = default;
  ~Handle() { reset(); }
  Handle(const Handle&) = delete;
  Handle& operator=(const Handle&) = delete;
  Handle(Handle&& o) noexcept : h_(o.h_), owned_(o.owned_) { o.forget(); }
  Handle& operator=(Handle&& o) noexcept {
    if (this != &o) {
      reset();
      h_ = o.h_;
      owned_ = o.owned_;
      o.forget();
    }
    return *this;
  }
  H get() const { return h_; }
  operator H() const { return h_; }
  H operator->() const { return h_; }
  bool owned() const { return owned_; }
  // Release an owned resource (a borrowed one is only dropped); the handle is empty afterwards.
  void reset() {
    if (h_ && owned_) Rel::release(h_);
    forget();
  }
  void adopt(H h) {  // take ownership of h
    reset();
    h_ = h;
    owned_ = h != H{};
  }
  void borrow(H h) {  // refer to a resource someone else releases
    reset();
    h_ = h;
    owned_ = false;
  }

 private:
  void forget() {
    h_ = H{};
    owned_ = false;
  }
  H h_{};
  bool owned_ = false;
};

template <class T, class Api>
struct DeviceRelease {
  static void release(T* p) { Api::dev_free(p); }
};
template <class T, class Api>
struct PinnedRelease {
  static void release(T* p) { Api::pin_free(p); }
};
template <class E, class Api>
struct EventRelease {
  static void release(E e) { Api::event_destroy(e); }
};
template <class S, class Api>
struct StreamRelease {
  static void release(S s) { Api::stream_destroy(s); }
};

// Device buffer of T with its capacity in bytes.
template <class T, class Api>
class DeviceBufT : public Handle<T*, DeviceRelease<T, Api>> {
  using Base = Handle<T*, DeviceRelease<T, Api>>;

 public:
  size_t cap() const { return cap_; }
  // Drop the old buffer (its contents are not kept) and allocate `bytes`.
  int alloc(size_t bytes) {
    reset();
    void* p = nullptr;
    const int e = Api::dev_alloc(&p, bytes);
    if (e) return e;
    Base::adopt(static_cast<T*>(p));
    cap_ = bytes;
    return 0;
  }
  // alloc only when the capacity is short.  A caller whose stream may still read the old buffer
  // synchronises it first (capi::grow).
  int grow(size_t bytes) { return bytes <= cap_ ? 0 : alloc(bytes); }
  void reset() {
    Base::reset();
    cap_ = 0;
  }
  void borrow(T* p) {  // capacity 0: a borrowed buffer is never grown into
    Base::borrow(p);
    cap_ = 0;
  }
  DeviceBufT() = default;
  DeviceBufT(DeviceBufT&& o) noexcept : Base(std::move(o)), cap_(o.cap_) { o.cap_ = 0; }
  DeviceBufT& operator=(DeviceBufT&& o) noexcept {
    if (this != &o) {
      Base::operator=(std::move(o));
      cap_ = o.cap_;
      o.cap_ = 0;
    }
    return *this;
  }

 private:
  size_t cap_ = 0;
};

template <class T, class Api>
class PinnedBufT : public Handle<T*, PinnedRelease<T, Api>> {
 public:
  int alloc(size_t bytes) {
    void* p = nullptr;
    const int e = Api::pin_alloc(&p, bytes);
    if (e) return e;
    this->adopt(static_cast<T*>(p));
    return 0;
  }
};

template <class Api>
class EventT : public Handle<typename Api::event_t, EventRelease<typename Api::event_t, Api>> {
 public:
  int create(unsigned flags = 0) {
    typename Api::event_t e{};
    const int rc = Api::event_create(&e, flags);
    if (rc) return rc;
    this->adopt(e);
    return 0;
  }
};

template <class Api>
class StreamT : public Handle<typename Api::stream_t, StreamRelease<typename Api::stream_t, Api>> {
 public:
  int create(unsigned flags) {
    typename Api::stream_t s{};
    const int rc = Api::stream_create(&s, flags);
    if (rc) return rc;
    this->adopt(s);
    return 0;
  }
  int create(unsigned flags, int priority) {
    typename Api::stream_t s{};
    const int rc = Api::stream_create_prio(&s, flags, priority);
    if (rc) return rc;
    this->adopt(s);
    return 0;
  }
};

#ifndef MPPI_HANDLES_NO_HIP
struct HipApi {
  using event_t = hipEvent_t;
  using stream_t = hipStream_t;
  static int dev_alloc(void** p, size_t bytes) { return (int)hipMalloc(p, bytes); }
  static void dev_free(void* p) { (void)hipFree(p); }
  static int pin_alloc(void** p, size_t bytes) { return (int)hipHostMalloc(p, bytes, hipHostMallocDefault); }
  static void pin_free(void* p) { (void)hipHostFree(p); }
  static int event_create(hipEvent_t* e, unsigned flags) { return (int)hipEventCreateWithFlags(e, flags); }
  static void event_destroy(hipEvent_t e) { (void)hipEventDestroy(e); }
  static int stream_create(hipStream_t* s, unsigned flags) { return (int)hipStreamCreateWithFlags(s, flags); }
  static int stream_create_prio(hipStream_t* s, unsigned flags, int priority) {
    return (int)hipStreamCreateWithPriority(s, flags, priority);
  }
  static void stream_destroy(hipStream_t s) { (void)hipStreamDestroy(s); }
};
template <class T>
using DeviceBuf = DeviceBufT<T, HipApi>;
template <class T>
using PinnedBuf = PinnedBufT<T, HipApi>;
using Event = EventT<HipApi>;
using Stream = StreamT<HipApi>;
#endif

}  // namespace mppi
