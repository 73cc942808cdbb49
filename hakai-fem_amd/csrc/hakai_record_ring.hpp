// hakai_record_ring.hpp -- hkc::RecordRing, the device ring a history output's kernels write records
// to and the host reads them from (DESIGN.md "Record rings and the ordered tree"). The kernel that
// finishes a record writes slot count % cap and adds one to the count; the host zeroes the count
// (restart) and copies out. Refusals and slot arithmetic: hakai_record_sets.hpp (HIP-free).
#pragma once
#include <cstring>

#include "hakai_devmem.hpp"
#include "hakai_record_sets.hpp"

namespace hkc {

struct RecordRing {
    long long stride = 1, cap = 1;
    size_t W = 0;                        // values of a record
    DevBuf<double> d_ring;               // [cap][1 + W]: step k (as int64), then the values
    DevBuf<unsigned long long> d_count;  // records written since the (re)start

    // (arguments that passed ring_check)
    hipError_t alloc(size_t W_, long long stride_, long long capacity, hipStream_t s) {
        W = W_, stride = stride_, cap = capacity;
        const hipError_t e = d_ring.alloc_zero((size_t)cap * (1 + W), s);
        return e != hipSuccess ? e : d_count.alloc_zero(1, s);
    }
    hipError_t restart(hipStream_t s) { return hipMemsetAsync(d_count, 0, sizeof(unsigned long long), s); }

    int count(hipStream_t s, int64_t* n_written, int64_t* n_held) const {
        unsigned long long n = 0;
        HIPCHK(hipMemcpyAsync(&n, d_count, sizeof n, hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        if (n_written) *n_written = (int64_t)n;
        if (n_held) *n_held = std::min<int64_t>((int64_t)n, cap);
        return 0;
    }

    // Records [first, first + n) into steps [n] and values [n][W] (either may be null).
    int read(hipStream_t s, const char* what, int64_t first, int64_t n, int64_t* steps, double* values) const {
        int64_t nw = 0, nh = 0, s0, n0;
        if (int r = count(s, &nw, &nh)) return r;
        if (int r = read_range_check(what, first, n, nw, nh)) return r;
        if (n == 0 || (!steps && !values)) return 0;
        const size_t R = 1 + W;
        std::vector<double> buf((size_t)n * R);
        ring_runs(first, n, cap, &s0, &n0);
        HIPCHK(hipMemcpyAsync(buf.data(), d_ring + (size_t)s0 * R, (size_t)n0 * R * sizeof(double),
                              hipMemcpyDeviceToHost, s));
        if (n > n0)
            HIPCHK(hipMemcpyAsync(buf.data() + (size_t)n0 * R, d_ring, (size_t)(n - n0) * R * sizeof(double),
                                  hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        for (int64_t i = 0; i < n; ++i) {
            if (steps) std::memcpy(&steps[i], &buf[(size_t)i * R], sizeof(int64_t));
            if (values) std::memcpy(values + (size_t)i * W, &buf[(size_t)i * R + 1], W * sizeof(double));
        }
        return 0;
    }
};

}  // namespace hkc
