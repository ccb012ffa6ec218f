// The one owner of device and pinned host memory behind the C ABI: a move-only typed buffer over a small allocator policy.
//   DevBuf<T>  hipMalloc / hipFree                      PinBuf<T>  hipHostMalloc(hipHostMallocDefault) / hipHostFree
// A buffer converts to T* on its own: kernel-argument structs and launchers take raw pointers, and a null pointer is state in many
// places (`!ws->d_sw_items`).  The capacity (in elements) lives in the buffer; reserve() is the grow-only step and keeps no contents.
// Nothing here pools or caches: release() gives the block back, the destructor releases.  Whoever lets a buffer go while a stream may
// still read it synchronises first -- the buffer does not know the streams.
// Every operation returns the project's status (0, or fail()'s 1 with the message set).  The HIP policies count their live
// allocations (aqc_live_buffers).  HIP-free without hipcc: tests/native/devbuf_selftest.cpp supplies a policy of its own.
#pragma once
#include <cstddef>
#include <vector>

namespace aqc {

int fail(const char* fmt, ...) __attribute__((format(printf, 1, 2)));   // sets the thread's error message; returns 1 (aqc_api.cpp)

// Policy: static int allocate(void** p, size_t bytes), int deallocate(void* p), int copy_in(void* dst, const void* host, size_t bytes)
template <class T, class Policy>
class Buf {
    T* p_ = nullptr;
    size_t cap_ = 0;

public:
    Buf() = default;
    Buf(const Buf&) = delete;
    Buf& operator=(const Buf&) = delete;
    Buf(Buf&& o) noexcept : p_(o.p_), cap_(o.cap_) { o.p_ = nullptr; o.cap_ = 0; }
    Buf& operator=(Buf&& o) noexcept {
        if (this != &o) {
            (void)release();
            p_ = o.p_; cap_ = o.cap_;
            o.p_ = nullptr; o.cap_ = 0;
        }
        return *this;
    }
    ~Buf() { (void)release(); }

    int alloc(size_t n) {   // exactly n elements, into an empty buffer
        if (p_) return fail("alloc(%zu) on a buffer that holds %zu elements", n, cap_);
        void* q = nullptr;
        if (Policy::allocate(&q, n * sizeof(T))) return 1;
        p_ = static_cast<T*>(q);
        cap_ = q ? n : 0;
        return 0;
    }
    int reserve(size_t n) {   // grow-only; the contents are not kept
        if (n <= cap_) return 0;
        if (release()) return 1;
        return alloc(n);
    }
    int upload(const std::vector<T>& v, size_t min_count = 1) {   // alloc + synchronous copy (plan tables, job lists)
        if (alloc(v.size() > min_count ? v.size() : min_count)) return 1;
        return v.empty() ? 0 : Policy::copy_in(p_, v.data(), v.size() * sizeof(T));
    }
    int release() {
        T* q = p_;
        p_ = nullptr; cap_ = 0;
        return q ? Policy::deallocate(q) : 0;
    }
    size_t capacity() const { return cap_; }
    explicit operator bool() const { return p_ != nullptr; }
    operator T*() const { return p_; }
};

}  // namespace aqc

#if defined(__HIPCC__)
#include <hip/hip_runtime_api.h>

#include <atomic>

namespace aqc {

inline std::atomic<long long> g_live_device{0}, g_live_pinned{0};   // live allocations of the two policies

struct HipDevice {
    static int allocate(void** p, size_t bytes) {
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) { *p = nullptr; return fail("hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); }
        if (*p) ++g_live_device;
        return 0;
    }
    static int deallocate(void* p) {
        --g_live_device;
        const hipError_t e = hipFree(p);
        return e == hipSuccess ? 0 : fail("hipFree failed: %s", hipGetErrorString(e));
    }
    static int copy_in(void* dst, const void* host, size_t bytes) {
        const hipError_t e = hipMemcpy(dst, host, bytes, hipMemcpyHostToDevice);
        return e == hipSuccess ? 0 : fail("hipMemcpy(%zu bytes, host to device) failed: %s", bytes, hipGetErrorString(e));
    }
};

struct HipPinned {
    static int allocate(void** p, size_t bytes) {
        const hipError_t e = hipHostMalloc(p, bytes, hipHostMallocDefault);
        if (e != hipSuccess) { *p = nullptr; return fail("hipHostMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e)); }
        if (*p) ++g_live_pinned;
        return 0;
    }
    static int deallocate(void* p) {
        --g_live_pinned;
        const hipError_t e = hipHostFree(p);
        return e == hipSuccess ? 0 : fail("hipHostFree failed: %s", hipGetErrorString(e));
    }
    static int copy_in(void* dst, const void* host, size_t bytes) {
        const hipError_t e = hipMemcpy(dst, host, bytes, hipMemcpyHostToHost);
        return e == hipSuccess ? 0 : fail("hipMemcpy(%zu bytes, host to pinned) failed: %s", bytes, hipGetErrorString(e));
    }
};

template <class T> using DevBuf = Buf<T, HipDevice>;
template <class T> using PinBuf = Buf<T, HipPinned>;

}  // namespace aqc
#endif
