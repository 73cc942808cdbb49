// hakai_conn_plan.hpp -- planner of the connectivity templates: pure host code, no HIP, no context.
// hakai_upload_model plans and uploads the result; tools/conn_plan_check.cpp checks the round trip on
// the CPU (tests/test_conn_templates.py).
#pragma once
#include <cstddef>
#include <vector>

namespace hk {

// ---------------------------------------------------------------------------------------------
// Connectivity templates (tuning "conn_templates"). On an extruded or structured mesh the eight
// node ids of an element are its first node plus the same eight offsets for every element of a
// region. The plan stores, per element, the base node conn[e][0] and the id of its offset pattern,
// packed into one 32-bit record
//     rec[e] = base | pid << base_bits        (base_bits: what the largest base needs)
// and a table pat[P][8] of the distinct patterns, pat[p][k] = conn[e][k] - conn[e][0] (int32, any
// sign; pat[p][0] = 0). Lane k of the element kernel forms its node as
//     (rec[e] & (1 << base_bits) - 1) + pat[8 (rec[e] >> base_bits) + k]
// which is conn[e][k] exactly, padding elements included (they are elements like any other here: all
// eight nodes 0, so a pattern of zeros). The kernel then streams 4 B per element instead of 32; the
// table is read from the caches.
//
// No compressed form -- the kernel runs the plain array -- when the mesh has more than `cap` distinct
// patterns (the table must stay cache resident: kConnPatCap patterns are 8 KB) or when a base and a
// pattern id do not fit 32 bits together. The planner stops at the first pattern past the cap, so an
// unstructured mesh costs a few hundred elements' worth of look-ups at upload and nothing per step.
// ---------------------------------------------------------------------------------------------
constexpr int kConnPatCap = 256;

struct ConnPlan {
    bool ok = false;            // a compressed form exists (else every other member is empty / 0)
    int P = 0;                  // distinct patterns
    int base_bits = 0;          // low bits of a record that hold the base node
    std::vector<unsigned> rec;  // [nEp]
    std::vector<int> pat;       // [8 P]
    long long bytes = 0;        // predicted connectivity bytes the element kernel reads per launch:
                                // 4 nEp + 32 P with a compressed form, 32 nEp with the plain array
};

// conn: [8 nEp] element nodes, 0-based and non-negative, padding elements included.
// Returns plan.ok; plan.bytes is set either way.
bool conn_plan(const int* conn, long long nEp, ConnPlan& plan, int cap = kConnPatCap);

// The node of (e, k) as the kernel forms it.
inline int conn_decode(const ConnPlan& p, long long e, int k) {
    const unsigned r = p.rec[(size_t)e];
    return (int)(r & ((1u << p.base_bits) - 1u)) + p.pat[8 * (size_t)(r >> p.base_bits) + (size_t)k];
}

}  // namespace hk
