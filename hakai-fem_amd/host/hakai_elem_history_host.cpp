// hakai_elem_history_host.cpp -- the host helpers of the element-set history (include/hakai_hip.h),
// no GPU and no other part of the library: the CSV writer and the combination of the ranks' partial
// records. Compiled without contraction: hakai_elem_history_combine's sums are plain additions in
// rank order. The CSV loop and the refusals in front of the combination are hakai_records_host.hpp's,
// shared with the node-set history. tests/test_elem_history_cpu.py builds this file alone.
#include "../../include/hakai_hip.h"
#include "hakai_records_host.hpp"

extern "C" {

int hakai_elem_history_write_csv(const char* path, int32_t n_names, const char* const* set_names, int64_t n,
                                 const int64_t* steps, const double* values, double d_time) {
    static const char* const field[HAKAI_ELEM_HISTORY_FIELDS] = {
        "N_active", "N_deleted", "V",    "V0",   "S_xx", "S_yy", "S_zz",     "S_xy",          "S_yz",      "S_zx",           "E_xx", "E_yy",
        "E_zz",     "E_xy",      "E_yz", "E_zx", "EQ",   "SE",   "PD",       "eqps_max",      "eqps_max_elem", "mises_max", "mises_max_elem",
        "J_min"};
    return hkc::write_records_csv("elem_history_write_csv", path, field, HAKAI_ELEM_HISTORY_FIELDS,
                                  HAKAI_ELEM_HISTORY_MAX_SETS, n_names, set_names, n, steps, values, d_time);
}

int hakai_elem_history_combine(int32_t n_ranks, int32_t n_total, int64_t n, const int64_t* steps,
                               const double* values, int64_t* steps_out, double* values_out) {
    if (int r = hkc::combine_check("elem_history_combine", HAKAI_ELEM_HISTORY_MAX_SETS, n_ranks, n_total, n, steps,
                                   !steps || !values || !steps_out || !values_out, false))
        return r;
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
