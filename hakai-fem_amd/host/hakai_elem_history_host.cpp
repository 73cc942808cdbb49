// hakai_elem_history_host.cpp -- the host helpers of the element-set history (include/hakai_hip.h),
// no GPU and no other part of the library: the CSV writer and the combination of the ranks' partial
// records. Compiled without contraction: hakai_elem_history_combine's sums are plain additions in
// rank order. tests/test_elem_history_cpu.py builds this file alone.
#include <cstdio>
#include <cstring>

#include "../../include/hakai_hip.h"

namespace hkc {
int fail(int code, const char* fmt, ...);
}  // namespace hkc
using hkc::fail;

extern "C" {

int hakai_elem_history_write_csv(const char* path, int32_t n_names, const char* const* set_names, int64_t n,
                                 const int64_t* steps, const double* values, double d_time) {
    static const char* const field[HAKAI_ELEM_HISTORY_FIELDS] = {
        "N_active", "N_deleted", "V",    "V0",   "S_xx", "S_yy", "S_zz",     "S_xy",          "S_yz",      "S_zx",           "E_xx", "E_yy",
        "E_zz",     "E_xy",      "E_yz", "E_zx", "EQ",   "SE",   "PD",       "eqps_max",      "eqps_max_elem", "mises_max", "mises_max_elem",
        "J_min"};
    if (!path || n_names < 1 || n_names > HAKAI_ELEM_HISTORY_MAX_SETS + 1 || !set_names || n < 0 ||
        (n > 0 && (!steps || !values)))
        return fail(HAKAI_ERR_ARG, "elem_history_write_csv: bad arguments");
    FILE* fp = std::fopen(path, "w");
    if (!fp) return fail(HAKAI_ERR_IO, "%s: cannot open for writing", path);
    std::fprintf(fp, "step,time");
    for (int s = 0; s < n_names; ++s)
        for (int f = 0; f < HAKAI_ELEM_HISTORY_FIELDS; ++f) std::fprintf(fp, ",%s_%s", set_names[s], field[f]);
    std::fprintf(fp, "\n");
    const size_t W = (size_t)n_names * HAKAI_ELEM_HISTORY_FIELDS;
    for (int64_t i = 0; i < n; ++i) {
        std::fprintf(fp, "%lld,%.17g", (long long)steps[i], (double)steps[i] * d_time);
        for (size_t j = 0; j < W; ++j) std::fprintf(fp, ",%.17g", values[(size_t)i * W + j]);
        std::fprintf(fp, "\n");
    }
    const bool bad = std::ferror(fp) != 0;
    if (std::fclose(fp) != 0 || bad) return fail(HAKAI_ERR_IO, "%s: write failed", path);
    return 0;
}

int hakai_elem_history_combine(int32_t n_ranks, int32_t n_total, int64_t n, const int64_t* steps,
                               const double* values, int64_t* steps_out, double* values_out) {
    if (n_ranks < 1 || n_total < 1 || n_total > HAKAI_ELEM_HISTORY_MAX_SETS + 1 || n < 0)
        return fail(HAKAI_ERR_ARG, "elem_history_combine: %d ranks, %d sets, %lld records", n_ranks, n_total,
                    (long long)n);
    if (n > 0 && (!steps || !values || !steps_out || !values_out))
        return fail(HAKAI_ERR_ARG, "elem_history_combine: null array");
    for (int r = 1; r < n_ranks; ++r)
        for (int64_t i = 0; i < n; ++i)
            if (steps[(size_t)r * n + i] != steps[i])
                return fail(HAKAI_ERR_STATE, "elem_history_combine: record %lld is step %lld on rank 0 and step %lld on "
                            "rank %d (stride and capacity must be the same on every rank)", (long long)i,
                            (long long)steps[i], (long long)steps[(size_t)r * n + i], r);
    const int F = HAKAI_ELEM_HISTORY_FIELDS;
    const size_t W = (size_t)n * n_total * F;
    for (size_t j = 0; j < W; ++j) {
        const int f = (int)(j % F);
        double x = values[j];
        if (f <= 18) {  // ((p_0 + p_1) + p_2) + ... in rank order, one rounding per addition
            for (int r = 1; r < n_ranks; ++r) x = x + values[(size_t)r * W + j];
        } else if (f == 19 || f == 21) {  // the larger value, the lower id among equals; id 0: no active element
            double id = values[j + 1];
            for (int r = 1; r < n_ranks; ++r) {
                const double ox = values[(size_t)r * W + j], oid = values[(size_t)r * W + j + 1];
                if (oid > 0.0 && (!(id > 0.0) || ox > x || (ox == x && oid < id))) {
                    x = ox;
                    id = oid;
                }
            }
            values_out[j + 1] = id;
        } else if (f == 20 || f == 22) {
            continue;  // (written with its value)
        } else {
            for (int r = 1; r < n_ranks; ++r) {
                const double ox = values[(size_t)r * W + j];
                x = ox < x ? ox : x;
            }
        }
        values_out[j] = x;
    }
    for (int64_t i = 0; i < n; ++i) steps_out[i] = steps[i];
    return 0;
}

}  // extern "C"
