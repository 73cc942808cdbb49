// hakai_stable_dt_host.cpp -- the host helpers of the stable-time-step diagnostic
// (include/hakai_hip.h), no GPU and no other part of the library: the combination of the ranks'
// results and the CSV writer of the drivers' stable_dt.csv.
#include <cstdio>

#include "../../include/hakai_hip.h"

namespace hkc {
int fail(int code, const char* fmt, ...);
}  // namespace hkc
using hkc::fail;

// (value, element) of b replaces a's when it is smaller, or equal with the lower element id; element
// 0 is "no active element" and never wins.
static void take_min(double& v, int64_t& id, double ov, int64_t oid) {
    if (oid == 0) return;
    if (id == 0 || ov < v || (ov == v && oid < id)) {
        v = ov;
        id = oid;
    }
}

extern "C" {

int hakai_stable_dt_combine(int32_t n_ranks, const hakai_stable_dt_t* parts, hakai_stable_dt_t* out) {
    if (n_ranks < 1 || !parts || !out) return fail(HAKAI_ERR_ARG, "stable_dt_combine: %d ranks or a null pointer", n_ranks);
    hakai_stable_dt_t r;
    r.dt_est = r.dt_safe = __builtin_inf();
    r.element_est = r.element_safe = 0;
    r.n_active = r.n_est_below = r.n_safe_below = 0;
    for (int q = 0; q < n_ranks; ++q) {
        take_min(r.dt_est, r.element_est, parts[q].dt_est, parts[q].element_est);
        take_min(r.dt_safe, r.element_safe, parts[q].dt_safe, parts[q].element_safe);
        r.n_active += parts[q].n_active;
        r.n_est_below += parts[q].n_est_below;
        r.n_safe_below += parts[q].n_safe_below;
    }
    *out = r;
    return 0;
}

int hakai_stable_dt_write_csv(const char* path, int64_t n, const int64_t* steps, const hakai_stable_dt_t* rec,
                              double d_time) {
    if (!path || n < 0 || (n > 0 && (!steps || !rec))) return fail(HAKAI_ERR_ARG, "stable_dt_write_csv: bad arguments");
    FILE* fp = std::fopen(path, "w");
    if (!fp) return fail(HAKAI_ERR_IO, "%s: cannot open for writing", path);
    std::fprintf(fp, "step,time,d_time,dt_est,element_est,dt_safe,element_safe,n_active,n_est_below,n_safe_below\n");
    for (int64_t i = 0; i < n; ++i)
        std::fprintf(fp, "%lld,%.17g,%.17g,%.17g,%lld,%.17g,%lld,%lld,%lld,%lld\n", (long long)steps[i],
                     (double)steps[i] * d_time, d_time, rec[i].dt_est, (long long)rec[i].element_est, rec[i].dt_safe,
                     (long long)rec[i].element_safe, (long long)rec[i].n_active, (long long)rec[i].n_est_below,
                     (long long)rec[i].n_safe_below);
    const bool bad = std::ferror(fp) != 0;
    if (std::fclose(fp) != 0 || bad) return fail(HAKAI_ERR_IO, "%s: write failed", path);
    return 0;
}

}  // extern "C"
