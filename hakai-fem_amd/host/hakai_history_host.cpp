// hakai_history_host.cpp -- the host helpers of history output (include/hakai_hip.h), no GPU and no
// other part of the library: the CSV writer, the drivers' set definition (hakai_run_inp and the
// N-GPU driver hakai.run take their sets from here, so they cannot drift), and the combination of
// the ranks' partial records. Compiled without contraction: hakai_history_combine's sums are plain
// additions in rank order. The CSV loop and the refusals in front of the combination are
// hakai_records_host.hpp's, shared with the element-set history. tools/history_host_check.cpp builds
// this file alone.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_records_host.hpp"

namespace hkc {
void history_driver_sets(const hakai_inp_model_t* M, std::vector<std::string>& names, std::vector<int64_t>& off,
                         std::vector<int64_t>& nodes, std::vector<std::string>& dropped);
}  // namespace hkc
using hkc::fail;

// HAKAI_HISTORY=<stride>: the sets of the drivers' history output -- "all" (set 0), one per
// instance, then one per *Boundary group (the nodes of its dofs), HAKAI_HISTORY_MAX_SETS in all.
void hkc::history_driver_sets(const hakai_inp_model_t* M, std::vector<std::string>& names, std::vector<int64_t>& off,
                              std::vector<int64_t>& nodes, std::vector<std::string>& dropped) {
    names.assign(1, "all");
    off.assign(1, 0);
    nodes.clear();
    dropped.clear();
    auto add = [&](const std::string& name, const std::vector<int64_t>& ns) {
        if ((int)names.size() > HAKAI_HISTORY_MAX_SETS) {
            dropped.push_back(name);
            return;
        }
        names.push_back(name);
        nodes.insert(nodes.end(), ns.begin(), ns.end());
        off.push_back((int64_t)nodes.size());
    };
    for (int i = 0; i < M->n_instance; ++i) {
        const int64_t n0 = M->instance_node_offset[i];
        const int64_t n1 = i + 1 < M->n_instance ? M->instance_node_offset[i + 1] : M->nNode;
        std::vector<int64_t> ns;
        for (int64_t n = n0; n < n1; ++n) ns.push_back(n + 1);
        add("inst" + std::to_string(i + 1), ns);
    }
    for (int g = 0; g < M->bc.n_groups; ++g) {
        std::vector<int64_t> ns;
        for (int64_t en = M->bc.entry_off[g]; en < M->bc.entry_off[g + 1]; ++en)
            for (int64_t d = M->bc.dof_off[en]; d < M->bc.dof_off[en + 1]; ++d) ns.push_back((M->bc.dofs[d] - 1) / 3 + 1);
        std::sort(ns.begin(), ns.end());
        ns.erase(std::unique(ns.begin(), ns.end()), ns.end());
        add("bc" + std::to_string(g + 1), ns);
    }
}

extern "C" {

int hakai_history_write_csv(const char* path, int32_t n_names, const char* const* set_names, int64_t n,
                            const int64_t* steps, const double* values, double d_time) {
    static const char* const field[HAKAI_HISTORY_FIELDS] = {"F_int_x", "F_int_y", "F_int_z", "F_ext_x", "F_ext_y", "F_ext_z",
                                                            "P_x",     "P_y",     "P_z",     "KE",      "W_int",   "W_ext",
                                                            "W_bc",    "U_x",     "U_y",     "U_z"};
    return hkc::write_records_csv("history_write_csv", path, field, HAKAI_HISTORY_FIELDS, HAKAI_HISTORY_MAX_SETS, n_names,
                                  set_names, n, steps, values, d_time);
}

int hakai_inp_history_sets(const hakai_inp_model_t* model, int32_t* n_sets, int64_t* set_off, int64_t* set_nodes,
                           int64_t nodes_cap, char* names, int64_t names_cap, int32_t* n_dropped) {
    if (!model || !n_sets || !set_off) return fail(HAKAI_ERR_ARG, "inp_history_sets: null");
    std::vector<std::string> nm, dropped;
    std::vector<int64_t> off, nodes;
    hkc::history_driver_sets(model, nm, off, nodes, dropped);
    std::string text;
    for (const std::string& s : nm) text += s + "\n";
    for (const std::string& s : dropped) text += s + "\n";
    if (set_nodes && nodes_cap < (int64_t)nodes.size())
        return fail(HAKAI_ERR_ARG, "inp_history_sets: %lld nodes, room for %lld", (long long)nodes.size(),
                    (long long)nodes_cap);
    if (names && names_cap < (int64_t)text.size() + 1)
        return fail(HAKAI_ERR_ARG, "inp_history_sets: %lld bytes of names, room for %lld", (long long)text.size() + 1,
                    (long long)names_cap);
    *n_sets = (int32_t)nm.size() - 1;
    if (n_dropped) *n_dropped = (int32_t)dropped.size();
    std::copy(off.begin(), off.end(), set_off);
    if (set_nodes) std::copy(nodes.begin(), nodes.end(), set_nodes);
    if (names) std::memcpy(names, text.c_str(), text.size() + 1);
    return 0;
}

int hakai_history_combine(int32_t n_ranks, int32_t n_total, int64_t n, const int64_t* steps, const double* values,
                          const double* ke_seed, int64_t* steps_out, double* values_out, double* ke_seed_out) {
    if (int r = hkc::combine_check("history_combine", HAKAI_HISTORY_MAX_SETS, n_ranks, n_total, n, steps,
                                   !steps || !values || !steps_out || !values_out, !ke_seed || !ke_seed_out))
        return r;
    // ((p_0 + p_1) + p_2) + ... in rank order, one rounding per addition (no contraction in this file)
    const size_t W = (size_t)n * n_total * HAKAI_HISTORY_FIELDS;
    for (size_t j = 0; j < W; ++j) {
        double x = values[j];
        for (int r = 1; r < n_ranks; ++r) x = x + values[(size_t)r * W + j];
        values_out[j] = x;
    }
    for (int s = 0; s < n_total; ++s) {
        double x = ke_seed[s];
        for (int r = 1; r < n_ranks; ++r) x = x + ke_seed[(size_t)r * n_total + s];
        ke_seed_out[s] = x;
    }
    for (int64_t i = 0; i < n; ++i) steps_out[i] = steps[i];
    return 0;
}

}  // extern "C"
