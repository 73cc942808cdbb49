// hakai_loads_plan.hpp -- planner of the external loads (hakai_set_loads): pure host code, no HIP,
// no context. It validates a hakai_loads_t against the mesh and builds what k_loads (hakai_loads.hip)
// gathers per node: the concentrated entries of each node in list order, and a CSR node -> (pressure
// entry, corner) in ascending order of the press_* index -- the order of the node's sum.
// tests/test_loads_cpu.py compiles the same file into a stand-alone program.
#pragma once
#include <string>
#include <vector>

#include "../../include/hakai_hip.h"

namespace hk {

struct LoadsPlan {
    // amplitude tables, 0-based offsets
    std::vector<int> amp_n, amp_off;
    std::vector<double> amp_t, amp_v;
    // concentrated entries grouped by node (counting sort: list order kept within a node)
    std::vector<int> cl_ptr;      // [nN+1]; empty without concentrated loads
    std::vector<int> cl_comp;     // component 0..2
    std::vector<int> cl_amp;      // table or -1
    std::vector<double> cl_val;
    // gravity
    std::vector<double> g_acc;    // [3 n_grav]
    std::vector<int> g_amp;
    // pressure: entry tables, then the per-node CSR of (entry, corner) pairs
    std::vector<int> pr_elem;     // 0-based element
    std::vector<int> pr_code;     // loads_face_code of the entry's face
    std::vector<int> pr_amp;
    std::vector<double> pr_val;
    std::vector<int> pr_ptr;      // [nN+1]; empty without pressure
    std::vector<int> pr_ent;      // 4 * entry + corner
};

// 0, or HAKAI_ERR_ARG with the reason in err; plan is complete only on 0.
// conn: [8 nE] element nodes, 0-based.
int loads_plan(const hakai_loads_t& L, long long nN, long long nE, const int* conn, LoadsPlan& plan,
               std::string& err);

}  // namespace hk
