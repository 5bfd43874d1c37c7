// host_buffer.h -- who frees what (included by chisel_hip.hip, host side only): a buffer is freed by the object that holds its
// owner, in that object's destructor, and nowhere else.  The views the kernels take (MapView, StereoView, ...) keep raw pointers:
// copies of get().  Move-only; alloc() frees what was held before, and holds nothing after a failure.  A DeviceBuffer knows its element
// count (size(): 0 while it holds nothing), so that a buffer grown on demand needs no capacity field beside it.
#pragma once
#include <hip/hip_runtime.h>
#include <assert.h>
#include <stddef.h>
#include <utility>

struct chisel_hip_map;

namespace chisel_hip {

// n elements of device memory (hipMalloc / hipFree)
template <class T>
struct DeviceBuffer {
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p_(o.p_), n_(o.n_) { o.p_ = nullptr; o.n_ = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }  // (o frees what this held)
    ~DeviceBuffer() { reset(); }
    hipError_t alloc(size_t n) {
        reset();
        const hipError_t e = hipMalloc(&p_, n * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else n_ = n;
        return e;
    }
    void reset() {
        if (p_) (void)hipFree(p_);
        p_ = nullptr;
        n_ = 0;
    }
    T *get() const { return p_; }
    size_t size() const { return n_; }  // elements
    explicit operator bool() const { return p_ != nullptr; }

private:
    T *p_ = nullptr;
    size_t n_ = 0;
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

// Pinned 64-bit words that a kernel on `stream` writes -- totals, then a table whose length the call sets -- and the host reads after
// its wait; grown on demand (doubled).
struct PinnedWords {
    hipError_t ensure(size_t need, hipStream_t stream) {
        if (need <= words_) return hipSuccess;
        hipError_t e = hipStreamSynchronize(stream);  // (a scan of an earlier call may still write the block that goes)
        if (e != hipSuccess) return e;
        words_ = 0;
        e = block_.alloc(2 * need);
        if (e == hipSuccess) words_ = 2 * need;
        return e;
    }
    volatile long long *get() const { return block_.get(); }
    long long *dev() const { return block_.dev(); }

private:
    PinnedBuffer<long long> block_;
    size_t words_ = 0;
};

// [n] 64-bit control words of a pass on the device -- zeroed by the call's one memset, added to by its kernels -- and where they
// reach the host.  The two members that need the map (its stream, its progress) are defined in host_totals.h.
struct ControlWords {
    int prepare(chisel_hip_map *m, size_t n);  // allocated once, with the pinned words beside them
    hipError_t zero(hipStream_t stream) { return hipMemsetAsync(ctl_.get(), 0, ctl_.size() * sizeof(unsigned long long), stream); }
    unsigned long long *dev() const { return ctl_.get(); }  // what the views take as ctl
    int report_and_wait(chisel_hip_map *m, volatile long long **words);  // the report kernel and THE WAIT of the call; *words: complete

private:
    DeviceBuffer<unsigned long long> ctl_;
    PinnedWords host_;
};

inline size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// The host arrays of one read-only call, staged through ONE device allocation that lives as long as this object.  The caller hands
// over its own pointers: in() / out() / inout() give an array that is asked for (non-null) a 16-byte-rounded section, begin()
// allocates, points each of them at its section and queues the copies in on `stream`, finish() queues the copies out.  With
// on_device the pointers are the device's already and stay as they are: nothing is allocated, copied or waited for.  Whatever was
// queued is waited for before the buffer dies -- in finish(), also after a failed copy, or else in the destructor.
class Staging {
public:
    Staging(hipStream_t stream, bool on_device) : stream_(stream), on_device_(on_device) {}
    ~Staging() {
        if (queued_) (void)hipStreamSynchronize(stream_);
    }
    template <class T> void in(const T *&p, size_t bytes) { add(p, bytes, true, false); }
    template <class T> void out(T *&p, size_t bytes) { add(p, bytes, false, true); }
    template <class T> void inout(T *&p, size_t bytes) { add(p, bytes, true, true); }
    hipError_t begin() {
        if (n_ == 0) return hipSuccess;
        hipError_t e = buf_.alloc(total_);
        queued_ = e == hipSuccess;
        for (int i = 0; i < n_ && e == hipSuccess; i++) {
            Section &s = sec_[i];
            s.dev = buf_.get() + s.at;
            s.point(s.slot, s.dev);
            if (s.copy_in) e = hipMemcpyAsync(s.dev, s.host, s.bytes, hipMemcpyHostToDevice, stream_);
        }
        return e;
    }
    // `e`: what the launch said; the first error of it, the copies out and the wait
    hipError_t finish(hipError_t e) {
        if (on_device_) return e;
        for (int i = 0; i < n_; i++)
            if (e == hipSuccess && sec_[i].copy_out) e = hipMemcpyAsync(const_cast<void *>(sec_[i].host), sec_[i].dev, sec_[i].bytes, hipMemcpyDeviceToHost, stream_);
        const hipError_t e_sync = hipStreamSynchronize(stream_);
        queued_ = false;
        return e == hipSuccess ? e_sync : e;
    }

private:
    struct Section {
        const void *host;
        size_t bytes, at;
        bool copy_in, copy_out;
        void *slot;                               // the caller's pointer variable ...
        void (*point)(void *slot, unsigned char *dev);  // ... and how to set it
        unsigned char *dev;
    };
    template <class T>
    void add(T *&p, size_t bytes, bool copy_in, bool copy_out) {
        if (on_device_ || !p) return;
        assert(n_ < MAX_SECTIONS);
        sec_[n_++] = Section{p, bytes, total_, copy_in, copy_out, &p, [](void *slot, unsigned char *dev) { *static_cast<T **>(slot) = reinterpret_cast<T *>(dev); }, nullptr};
        total_ += round16(bytes);
    }
    static constexpr int MAX_SECTIONS = 8;
    hipStream_t stream_;
    bool on_device_, queued_ = false;
    Section sec_[MAX_SECTIONS];
    int n_ = 0;
    size_t total_ = 0;
    DeviceBuffer<unsigned char> buf_;
};

}  // namespace chisel_hip
