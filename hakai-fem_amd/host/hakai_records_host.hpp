// hakai_records_host.hpp -- what the host helpers of the two history outputs share
// (hakai_history_host.cpp, hakai_elem_history_host.cpp): the CSV writer of records and the refusals in
// front of a combination of the ranks' records. No GPU and no other part of the library; the field
// names and the combination rules stay with their record type.
#pragma once
#include <cstdint>
#include <cstdio>

#include "../../include/hakai_hip.h"

namespace hkc {

int fail(int code, const char* fmt, ...);

// step,time,<set>_<field>,... then one line per record: values [n][n_names][n_fields], %.17g.
inline int write_records_csv(const char* what, const char* path, const char* const* fields, int n_fields, int max_sets,
                             int32_t n_names, const char* const* set_names, int64_t n, const int64_t* steps,
                             const double* values, double d_time) {
    if (!path || n_names < 1 || n_names > max_sets + 1 || !set_names || n < 0 || (n > 0 && (!steps || !values)))
        return fail(HAKAI_ERR_ARG, "%s: bad arguments", what);
    FILE* fp = std::fopen(path, "w");
    if (!fp) return fail(HAKAI_ERR_IO, "%s: cannot open for writing", path);
    std::fprintf(fp, "step,time");
    for (int s = 0; s < n_names; ++s)
        for (int f = 0; f < n_fields; ++f) std::fprintf(fp, ",%s_%s", set_names[s], fields[f]);
    std::fprintf(fp, "\n");
    const size_t W = (size_t)n_names * n_fields;
    for (int64_t i = 0; i < n; ++i) {
        std::fprintf(fp, "%lld,%.17g", (long long)steps[i], (double)steps[i] * d_time);
        for (size_t j = 0; j < W; ++j) std::fprintf(fp, ",%.17g", values[(size_t)i * W + j]);
        std::fprintf(fp, "\n");
    }
    const bool bad = std::ferror(fp) != 0;
    if (std::fclose(fp) != 0 || bad) return fail(HAKAI_ERR_IO, "%s: write failed", path);
    return 0;
}

// In front of a combination of n records of n_ranks ranks (steps [n_ranks][n]): the counts, the arrays
// (null_records: one that n > 0 needs is null; null_always: one that every call needs is), and the
// same steps on every rank.
inline int combine_check(const char* what, int max_sets, int32_t n_ranks, int32_t n_total, int64_t n,
                         const int64_t* steps, bool null_records, bool null_always) {
    if (n_ranks < 1 || n_total < 1 || n_total > max_sets + 1 || n < 0)
        return fail(HAKAI_ERR_ARG, "%s: %d ranks, %d sets, %lld records", what, n_ranks, n_total, (long long)n);
    if (null_always || (n > 0 && null_records)) return fail(HAKAI_ERR_ARG, "%s: null array", what);
    for (int r = 1; r < n_ranks; ++r)
        for (int64_t i = 0; i < n; ++i)
            if (steps[(size_t)r * n + i] != steps[i])
                return fail(HAKAI_ERR_STATE, "%s: record %lld is step %lld on rank 0 and step %lld on rank %d (stride "
                            "and capacity must be the same on every rank)", what, (long long)i, (long long)steps[i],
                            (long long)steps[(size_t)r * n + i], r);
    return 0;
}

}  // namespace hkc
