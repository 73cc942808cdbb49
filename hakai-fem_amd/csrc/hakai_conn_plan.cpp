// hakai_conn_plan.cpp -- planner of the connectivity templates (hakai_conn_plan.hpp).
#include "hakai_conn_plan.hpp"

#include <array>
#include <map>

namespace hk {

static int bits_for(unsigned v) {  // bits that hold 0..v
    int b = 0;
    while (b < 32 && (v >> b) != 0u) ++b;
    return b;
}

bool conn_plan(const int* conn, long long nEp, ConnPlan& plan, int cap) {
    plan = ConnPlan();
    plan.bytes = 32 * nEp;
    if (nEp <= 0 || cap < 1) return false;
    // pass 1: the distinct patterns in order of first appearance, and the largest base
    std::map<std::array<int, 8>, int> ids;
    std::vector<int> pid((size_t)nEp);
    std::vector<int> pat;
    unsigned max_base = 0;
    for (long long e = 0; e < nEp; ++e) {
        const int* c = conn + 8 * e;
        if (c[0] < 0) return false;
        std::array<int, 8> o;
        for (int k = 0; k < 8; ++k) {
            const long long d = (long long)c[k] - (long long)c[0];  // (both in [0, 2^31): fits int32)
            o[(size_t)k] = (int)d;
        }
        auto it = ids.find(o);
        if (it == ids.end()) {
            if ((int)ids.size() == cap) return false;  // one pattern too many: the plain array
            it = ids.emplace(o, (int)ids.size()).first;
            pat.insert(pat.end(), o.begin(), o.end());
        }
        pid[(size_t)e] = it->second;
        if ((unsigned)c[0] > max_base) max_base = (unsigned)c[0];
    }
    const int P = (int)ids.size();
    const int base_bits = bits_for(max_base);
    if (base_bits + bits_for((unsigned)(P - 1)) > 32) return false;
    // pass 2: the records
    plan.rec.resize((size_t)nEp);
    // (bases are non-negative int32, so base_bits <= 31 and the shifts are defined)
    for (size_t e = 0; e < (size_t)nEp; ++e) {
        const unsigned p = (unsigned)pid[e];
        plan.rec[e] = (unsigned)conn[8 * e] | (p << base_bits);
    }
    plan.pat.swap(pat);
    plan.P = P;
    plan.base_bits = base_bits;
    plan.bytes = 4 * nEp + 32 * (long long)P;
    plan.ok = true;
    return true;
}

}  // namespace hk
