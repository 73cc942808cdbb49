// hakai_record_sets.hpp -- what the history outputs share on the host before any device call
// (DESIGN.md "Record rings and the ordered tree"): the parser of the caller's sets, the refusals of a
// ring's stride and capacity, the arithmetic of a read from the ring. No HIP:
// tools/history_host_check.cpp drives every refusal and every range of small rings on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/hakai_hip.h"

namespace hkc {

int fail(int code, const char* fmt, ...);

// The caller's sets (set_off, 1-based set_ids) as a mask per item: bit s-1 of mask[i - 1] says item i
// is in set s. HAKAI_ERR_ARG names `what` (the calling function) and `item` ("node", "element").
inline int parse_sets(const char* what, const char* item, int max_sets, long long n_items, int32_t n_sets,
                      const int64_t* set_off, const int64_t* set_ids, std::vector<unsigned short>& mask) {
    if (n_sets < 0 || n_sets > max_sets) return fail(HAKAI_ERR_ARG, "%s: %d sets (0..%d)", what, n_sets, max_sets);
    if (n_sets > 0 && !set_off) return fail(HAKAI_ERR_ARG, "%s: null set_off", what);
    mask.assign((size_t)n_items, 0);
    for (int s = 0; s < n_sets; ++s) {
        if (set_off[s] < 0 || set_off[s + 1] < set_off[s] || (set_off[s + 1] > set_off[s] && !set_ids))
            return fail(HAKAI_ERR_ARG, "%s: bad set_off of set %d", what, s + 1);
        for (int64_t i = set_off[s]; i < set_off[s + 1]; ++i) {
            const long long id = set_ids[i];
            if (id < 1 || id > n_items)
                return fail(HAKAI_ERR_ARG, "%s: %s %lld of set %d out of 1..%lld", what, item, id, s + 1, n_items);
            if ((mask[id - 1] >> s) & 1u)
                return fail(HAKAI_ERR_ARG, "%s: %s %lld twice in set %d", what, item, id, s + 1);
            mask[id - 1] |= (unsigned short)(1u << s);
        }
    }
    return 0;
}

// A ring of `capacity` records of 1 + W doubles (the step, then W values), one every `stride` steps.
inline int ring_check(const char* what, int64_t stride, int64_t capacity, int64_t W) {
    if (stride < 1 || capacity < 1)
        return fail(HAKAI_ERR_ARG, "%s: stride %lld, capacity %lld (both >= 1)", what, (long long)stride,
                    (long long)capacity);
    if (capacity > ((int64_t)1 << 40) / (1 + W)) return fail(HAKAI_ERR_ARG, "%s: capacity too large", what);
    return 0;
}

// Records [first, first + n) of n_written, of which the ring still holds the newest n_held.
inline int read_range_check(const char* what, int64_t first, int64_t n, int64_t n_written, int64_t n_held) {
    if (first < 0 || n < 0 || first + n > n_written || (n > 0 && first < n_written - n_held))
        return fail(HAKAI_ERR_ARG, "%s: records [%lld, %lld) of %lld written, the newest %lld held", what,
                    (long long)first, (long long)(first + n), (long long)n_written, (long long)n_held);
    return 0;
}

// Record i is in slot i % cap: n <= cap records from `first` are n0 from slot s0, then n - n0 from slot 0.
inline void ring_runs(int64_t first, int64_t n, int64_t cap, int64_t* s0, int64_t* n0) {
    *s0 = first % cap;
    *n0 = std::min<int64_t>(n, cap - *s0);
}

}  // namespace hkc
