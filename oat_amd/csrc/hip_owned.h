// hip_owned.h -- move-only owners of the HIP resources a context holds: a device allocation, a page-locked host block (with its
// device alias where it is mapped) and an event.  A moved-from owner is empty; alloc / create on a full one releases first.
// Names runtime types and functions only and includes no runtime header: the includer does that first (tests/host puts a fake there).
#pragma once
#include <cstddef>
#include <utility>

namespace oatgpu {

template <class T> class DevMem {
    T *p_ = nullptr;
public:
    DevMem() = default;
    DevMem(DevMem &&o) noexcept : p_(std::exchange(o.p_, nullptr)) {}
    DevMem &operator=(DevMem &&o) noexcept { if (this != &o) { reset(); p_ = std::exchange(o.p_, nullptr); } return *this; }
    ~DevMem() { reset(); }
    hipError_t alloc(size_t bytes) { reset(); const hipError_t e = hipMalloc((void **)&p_, bytes); if (e != hipSuccess) p_ = nullptr; return e; }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    T *get() const { return p_; }
    operator T *() const { return p_; }
};

template <class T> class HostMem {
    T *h_ = nullptr, *d_ = nullptr;      // d_: the device alias of a hipHostMallocMapped block
public:
    HostMem() = default;
    HostMem(HostMem &&o) noexcept : h_(std::exchange(o.h_, nullptr)), d_(std::exchange(o.d_, nullptr)) {}
    HostMem &operator=(HostMem &&o) noexcept { if (this != &o) { reset(); h_ = std::exchange(o.h_, nullptr); d_ = std::exchange(o.d_, nullptr); } return *this; }
    ~HostMem() { reset(); }
    hipError_t alloc(size_t bytes, unsigned flags)
    {
        reset();
        hipError_t e = hipHostMalloc((void **)&h_, bytes, flags);
        if (e != hipSuccess) { h_ = nullptr; return e; }
        if (flags & hipHostMallocMapped) e = hipHostGetDevicePointer((void **)&d_, h_, 0);
        if (e != hipSuccess) reset();       // (no alias: the block is of no use)
        return e;
    }
    void reset() { if (h_) (void)hipHostFree(h_); h_ = d_ = nullptr; }
    T *host() const { return h_; }
    T *dev() const { return d_; }
};

class Event {
    hipEvent_t e_ = nullptr;
public:
    Event() = default;
    Event(Event &&o) noexcept : e_(std::exchange(o.e_, nullptr)) {}
    Event &operator=(Event &&o) noexcept { if (this != &o) { reset(); e_ = std::exchange(o.e_, nullptr); } return *this; }
    ~Event() { reset(); }
    hipError_t create(unsigned flags) { reset(); const hipError_t e = hipEventCreateWithFlags(&e_, flags); if (e != hipSuccess) e_ = nullptr; return e; }
    void reset() { if (e_) (void)hipEventDestroy(e_); e_ = nullptr; }
    operator hipEvent_t() const { return e_; }
};

}  // namespace oatgpu
