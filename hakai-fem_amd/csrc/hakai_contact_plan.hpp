// hakai_contact_plan.hpp -- planner of the contact model: pure host code, no HIP, no context.
// hakai_contact.hip contact_setup fills ContactInput and uploads the plan; tools/contact_plan_check.cpp
// compares it with the oracle's own lists on the CPU (tests/test_contact_plan.py).
//
// Reference: v2/HAKAI_j.jl (v2 = HAKAI-v0.0.2/Julia)
//   setup            :244-421   pairs (instance_pair, cp_index), CT lists, element sizes
//   get_element_face :1944-1992, get_surface_triangle :1996-2164, add_surface_triangle :2167-2245
//   surface update   :766-804   (after element deletion)
#pragma once
#include <cstdint>
#include <string>
#include <vector>

namespace hkc {

// ---------------------------------------------------------------------------------------------
// The contact lists the reference grows at run time (appending newly exposed faces when an element
// is deleted) are enumerated ONCE: every triangle / contact node that can ever appear is an entry
// that carries the elements whose deletion adds it ("adders"). An entry is live at step t iff it was
// in the initial list (orig = 1, triangle adder = -1) or one of its adders was deleted before t.
// Surfaces follow the reference's quirks: in a run of equal face keys an odd run
// keeps its last face, unless that is the very last face of the instance; a deletion exposes, for
// each face of the deleted element, the first face of another element with the same key. A pair
// (i instance, j instance) holds the i side's nodes (contact points), the j side's triangles and
// their nodes; the point side grows with every deletion in its instance, the triangle side only
// when the two instances differ (:766-804).
// Node entries of a pair side are one segment; segments whose live node sets are equal at every
// step (same instance, face filter and adders) share bounding boxes (Seg::dup / alias). Live lists
// are rebuilt per region (one per segment, one for all triangles) in tiles of kTile entries, and
// the element -> entry CSRs list what a deletion exposes.
// With an ownership block (multi-GPU, owner-computed search) the plan is that of the GLOBAL mesh
// restricted to the rank's entries: the node entries of the nodes it owns (owner = the rank of the
// node's lowest incident element) with local node ids, and the triangles of its own elements with
// local node and element ids; adders stay global.
// ---------------------------------------------------------------------------------------------

// Layouts shared with the device (hakai_contact.hip, hakai_contact_xr.hip).
struct PairParam {
    double young, kc, Cr, ddiv;
    int self;
    int hash_off, hash_size;
    int pad;
};
struct Seg {
    int start, end, pair, side;  // side 0: i-nodes, 1: j-nodes
    int region;
    int dup;       // 1: the same live node set as an earlier segment, whose boxes also fill this one's
    int alias[2];  // bbox offsets (12 pair + 6 side) of up to two such duplicates, -1 if none
};
static_assert(sizeof(Seg) == 32, "Seg: two 16-B vectors");
struct Tile {
    int list, start, end, region;
};
constexpr int kTile = 2048;  // entries per live-list tile

// multi-GPU: the entries this rank keeps
struct ContactOwnership {
    int rank = 0, nranks = 1;
    const int64_t* rank_elem_off = nullptr;  // [nranks+1] ascending element ranges
    const std::vector<int>* g2l = nullptr;   // [nN] local node or -1, validated by the caller
};

// Everything the planner reads.
struct ContactInput {
    long long nN = 0, nE = 0;
    const std::vector<double>* coord = nullptr;  // 3nN
    const std::vector<int>* conn = nullptr;      // 8nE, 0-based
    const std::vector<int>* mat = nullptr;       // nE, 0-based
    const std::vector<double>* young = nullptr;  // per material
    int contact_flag = 1;                        // 1 or 2 (2: self pairs too)
    const int64_t* element_instance = nullptr;   // [nE] 1-based contiguous blocks, null = one instance
    int n_cp = 0;                                // *Contact Pair surfaces (0: all exterior)
    const int32_t* cp_instance = nullptr;        // [n_cp][2] 1-based
    const int64_t* cp_elem_off = nullptr;        // [2 n_cp + 1]
    const int64_t* cp_elems = nullptr;           // instance-local, 1-based
    double kc_o = 1.0, kc_s = 1.0, Cr_o = 0.0, Cr_s = 0.0;  // :2255-2259
    const ContactOwnership* own = nullptr;
};

struct NodeEntries {  // all pairs concatenated
    std::vector<int> pair, node, orig, aptr{0}, add;
};

struct ContactPlan {
    std::vector<PairParam> par;
    int htot = 0;                        // hash buckets over all pairs
    NodeEntries ni, nj;                  // i side (contact points), j side (triangle nodes)
    std::vector<int> tri_pair, tri_nodes, tri_ele, tri_adder;
    std::vector<Seg> seg;
    std::vector<Tile> tiles;
    std::vector<int> reg_first;          // [nreg+1] first tile of each region
    std::vector<int> reg;                // [nreg][2] (base, live count = 0)
    std::vector<int> pair_reg;           // [npairs][2] region of (pair, side), -1 if none
    std::vector<int> reg_list;           // [nreg] list of each region (0 i-nodes, 1 j-nodes, 2 triangles)
    int tri_reg = 0;
    std::vector<int> el_ni_ptr, el_ni, el_nj_ptr, el_nj, el_tri_ptr, el_tri;  // element -> entries it exposes
    std::vector<int> pair_inst;          // [npairs][2] 1-based instances
    std::vector<long long> pair_counts;  // [npairs][3] initial #nodes_i, #triangles, #nodes_j (of every rank)
    double min_size = 0, max_size = 0, d_lim = 0;
    std::vector<long long> ni_per_rank;  // with ownership: i-node entries each rank keeps
};

// Builds the plan of a mesh with at least one element. Returns the message of an argument error
// (the plan is then unusable), or an empty string.
std::string contact_plan(const ContactInput& in, ContactPlan& P);

}  // namespace hkc
