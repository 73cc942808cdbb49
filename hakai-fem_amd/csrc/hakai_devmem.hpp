// hakai_devmem.hpp -- what every host translation unit of libhakai_hip.so uses around device memory:
// the HIP error check and hkc::DevBuf, the one owner of device memory. Every device allocation of the
// library is a DevBuf, a member of the state that owns it or a local, so a return on any path frees
// it; this file alone calls the runtime's allocator. A raw device pointer elsewhere is a view of a
// DevBuf that some state owns, and is commented as one.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <vector>

namespace hkc {

int hip_fail(hipError_t e, const char* what);  // hakai_capi.cpp: sets hakai_last_error

// Device arrays the process holds now (hakai_stat "device_buffers"): one per successful alloc, one
// less per free of a held array; a move changes nothing.
inline std::atomic<long long> g_dev_live{0};

// A device array that frees itself: move-only, converts to its pointer at launch sites.
template <class T>
class DevBuf {
  public:
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevBuf& operator=(DevBuf&& o) noexcept {
        if (this != &o) {
            free();
            p_ = o.p_;
            o.p_ = nullptr;
        }
        return *this;
    }
    ~DevBuf() { free(); }
    void free() {
        if (p_) {
            (void)hipFree((void*)p_);
            g_dev_live.fetch_sub(1, std::memory_order_relaxed);
        }
        p_ = nullptr;
    }
    // n elements (at least one), uninitialised; a held array is freed first
    hipError_t alloc(size_t n) {
        free();
        const hipError_t e = hipMalloc((void**)&p_, (n ? n : 1) * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        else g_dev_live.fetch_add(1, std::memory_order_relaxed);
        return e;
    }
    // n elements (at least one), zeroed on stream s
    hipError_t alloc_zero(size_t n, hipStream_t s) {
        const hipError_t e = alloc(n);
        return e != hipSuccess ? e : hipMemsetAsync(p_, 0, (n ? n : 1) * sizeof(T), s);
    }
    hipError_t upload(const std::vector<T>& v, hipStream_t s) {
        const hipError_t e = alloc(v.size());
        if (e != hipSuccess || v.empty()) return e;
        return hipMemcpyAsync(p_, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, s);
    }
    operator T*() const { return p_; }
    T* get() const { return p_; }

  private:
    T* p_ = nullptr;
};

}  // namespace hkc

#define HIPCHK(x)                                              \
    do {                                                       \
        hipError_t _e = (x);                                   \
        if (_e != hipSuccess) return ::hkc::hip_fail(_e, #x);  \
    } while (0)
