// host_buffer.h -- who frees what (included by chisel_hip.hip, host side only): a buffer is freed by the object that holds its
// owner, in that object's destructor, and nowhere else.  The views the kernels take (MapView, StereoView, ...) keep raw pointers:
// copies of get().  Move-only; alloc() frees what was held before, and holds nothing after a failure.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <utility>

namespace chisel_hip {

// n elements of device memory (hipMalloc / hipFree)
template <class T>
struct DeviceBuffer {
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p_, o.p_); return *this; }  // (o frees what this held)
    ~DeviceBuffer() { reset(); }
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
    }
    T *get() const { return p_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T *p_ = nullptr;
};

// n elements of page-locked host memory (hipHostMalloc / hipHostFree) that the device addresses too: dev() is get() as the kernels see it
template <class T>
struct PinnedBuffer {
    PinnedBuffer() = default;
    PinnedBuffer(PinnedBuffer &&o) noexcept : p_(o.p_), dev_(o.dev_) { o.p_ = o.dev_ = nullptr; }
    PinnedBuffer &operator=(PinnedBuffer &&o) noexcept { std::swap(p_, o.p_); std::swap(dev_, o.dev_); return *this; }
    ~PinnedBuffer() { reset(); }
    hipError_t alloc(size_t n) {
        reset();
        hipError_t e = hipHostMalloc((void **)&p_, n * sizeof(T), hipHostMallocDefault);
        if (e != hipSuccess) p_ = nullptr;
        else if ((e = hipHostGetDevicePointer((void **)&dev_, p_, 0)) != hipSuccess) reset();
        return e;
    }
    void reset() {
        if (p_) (void)hipHostFree(p_);
        p_ = dev_ = nullptr;
    }
    T *get() const { return p_; }
    T *dev() const { return dev_; }
    explicit operator bool() const { return p_ != nullptr; }

private:
    T *p_ = nullptr, *dev_ = nullptr;
};

}  // namespace chisel_hip
