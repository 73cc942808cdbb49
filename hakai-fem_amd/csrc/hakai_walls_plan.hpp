// hakai_walls_plan.hpp -- planner of the rigid walls (hakai_set_walls): pure host code, no HIP, no
// context. It validates a hakai_walls_t against the mesh, normalises the normals (once, on the host:
// hakai_walls_node.hpp walls_normalise) and builds what k_loads (hakai_loads.hip) reads: the wall
// table, the walls' amplitude tables and one 32-bit membership mask per node.
// tests/test_walls_cpu.py compiles the same file into a stand-alone program.
#pragma once
#include <string>
#include <vector>

#include "../../include/hakai_hip.h"

namespace hk {

struct WallsPlan {
    // amplitude tables, 0-based offsets
    std::vector<int> amp_n, amp_off;
    std::vector<double> amp_t, amp_v;
    int n_wall = 0;
    std::vector<double> tab;     // [kWallRow n_wall] rows of hakai_walls_node.hpp (n normalised)
    std::vector<int> amp;        // [n_wall] table or -1
    // bit w of mask[n]: node n is in wall w's list (a wall without a list sets its bit everywhere).
    // Empty when every wall takes every node: the kernel then reads no mask stream.
    std::vector<unsigned> mask;  // [nN] or empty
};

// 0, or HAKAI_ERR_ARG with the reason in err; plan is complete only on 0.
int walls_plan(const hakai_walls_t& W, long long nN, WallsPlan& plan, std::string& err);

}  // namespace hk
