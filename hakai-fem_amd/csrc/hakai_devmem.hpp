// hakai_devmem.hpp -- what every host translation unit of libhakai_hip.so uses around device memory:
// the HIP error check, raw allocation helpers and the owning device buffer.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

namespace hkc {

int hip_fail(hipError_t e, const char* what);  // hakai_capi.cpp: sets hakai_last_error

template <class T>
hipError_t dalloc(T** p, size_t n) {
    *p = nullptr;
    if (n == 0) n = 1;
    return hipMalloc((void**)p, n * sizeof(T));
}

template <class T>
void dfree(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

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
        if (p_) (void)hipFree((void*)p_);
        p_ = nullptr;
    }
    // n elements (at least one), uninitialised; a held array is freed first
    hipError_t alloc(size_t n) {
        free();
        const hipError_t e = hipMalloc((void**)&p_, (n ? n : 1) * sizeof(T));
        if (e != hipSuccess) p_ = nullptr;
        return e;
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
