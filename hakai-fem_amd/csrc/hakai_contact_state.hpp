// hakai_contact_state.hpp -- the contact search state (hkc::Contact), the records its hash grid
// holds, and what crosses between the two translation units of the contact search:
// hakai_contact.hip (the one-GPU step, setup, the C entry points) and hakai_contact_xr.hip (the
// owner-computed multi-GPU search, hkc::Xrank). Its device arrays are DevBufs (hakai_devmem.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "hakai_contact_plan.hpp"
#include "hakai_internal.hpp"

namespace hkc {

struct Xrank;  // multi-GPU state (hakai_contact_xr.hip)
namespace ck {
struct TriRec;  // hakai_contact_dev.hpp
struct StepIn;
}  // namespace ck

// A hash-bucket entry: the i-node's cell, node id and position (coord + u of this step, the value
// the triangle test would gather: the same expression, so the same bits), written by the binning
// straight into the bucket list, so the triangle search reads one 64-B record per entry and has no
// dependent gather of the node's position behind it. next: the bucket's next entry (-1 = end).
struct alignas(16) BEnt {
    long long m[3];
    int node, pad;
    double p[3];
    long long next;
};
static_assert(sizeof(BEnt) == 64, "BEnt: four 16-B vectors");

// What an event's force needs from its i-node besides the position: the velocity (d_disp / d_time
// of the previous step, :628, or the initial velocity) and the mass the damping term reads
// (diag_M[i] with the node id i, :2592). Formed by the binning (same expressions, same bits) and
// kept beside the bucket list, so the search loads it only for an event.
struct alignas(16) BVel {
    double v[3], mq;
};
// A binned i-node as it travels between ranks (multi-GPU, A2 -> A3); pad of BEnt = the pair.
struct alignas(16) BRec {
    BEnt e;
    BVel w;
};
static_assert(sizeof(BRec) == 96, "BRec: six 16-B vectors");

struct Contact {
    // node / element space of the kernels: the context's own (one GPU) or the global mirror
    long long nN = 0, nE = 0;
    Xrank* xr = nullptr;             // multi-GPU (hakai_set_contact_global), else null
    int npairs = 0;
    std::vector<PairParam> h_par;
    DevBuf<PairParam> d_par;
    // i-side (contact points) and j-side (triangle nodes) node entries, all pairs concatenated
    int n_ni = 0, n_nj = 0;
    DevBuf<int> d_ni_pair, d_ni_node, d_ni_orig, d_ni_aptr, d_ni_add;
    DevBuf<int> d_nj_pair, d_nj_node, d_nj_orig, d_nj_aptr, d_nj_add;
    int nseg = 0;
    DevBuf<Seg> d_seg;  // [nseg] node-entry segment (start, end, pair, side, region)
    // triangles
    int n_tri = 0;
    DevBuf<int> d_tri_pair, d_tri_nodes, d_tri_ele, d_tri_adder;
    // live lists (rebuilt on steps where the surface may have changed)
    int ntile = 0, nreg = 0;
    DevBuf<Tile> d_tiles;           // [ntile]
    DevBuf<int> d_tile_cnt, d_tile_off;  // [ntile], [ntile+1]
    DevBuf<int> d_reg_first;        // [nreg+1] first tile of each region
    DevBuf<int> d_reg;              // [nreg][2] (base, live count)
    DevBuf<int> d_pair_reg;         // [npairs][2] region of (pair, side)
    int tri_reg = 0;
    std::vector<int> reg_list_h;    // [nreg] list of each region (0 i-nodes, 1 j-nodes, 2 triangles)
    // element -> entries its deletion exposes (CSR), and the deleted-element list of a step
    DevBuf<int> d_el_tri_ptr, d_el_tri, d_el_ni_ptr, d_el_ni;
    DevBuf<int> d_el_nj_ptr, d_el_nj, d_dlist;
    DevBuf<int> d_ni_live, d_nj_live, d_tri_live;
    bool force_rebuild = true;
    bool always_rebuild = false;    // tuning/testing: full rebuild every step (no incremental update)
    long long last_t = -1;
    // launch grids sized at setup from the contact model (small decks: few blocks, so the ~20
    // per-step kernels are not dominated by dispatching idle workgroups); every loop is grid-stride
    int g_seg = 256, g_ev = 1024, g_tri = 4096, g_node = 256, g_del = 1024, g_reset = 64;
    int g_box = 32;  // bounding boxes: blocks per segment (each block ends in 6 atomics on the pair's
                     // 6 bounds, so fewer, longer blocks: ~4 entries per thread, one unrolled pass)
    // hash grid over i-nodes
    int htot = 0;
    // bucket heads: (search sequence << 32 | first entry); a head of an older sequence is an empty
    // bucket, so the table is never cleared (chained buckets: no count, scan or fill pass)
    DevBuf<unsigned long long> d_head;  // [htot]
    DevBuf<BEnt> d_blist;           // [blist_cap] bucket lists
    DevBuf<BVel> d_bvel;            // [blist_cap] beside them
    long long blist_cap = 0;
    DevBuf<unsigned long long> d_bbox;  // [npairs][12] ordered-integer encoded doubles
    // small decks (set at setup; tuning "contact_fuse_small"): fused single-workgroup phases
    bool small = false;
    int fuse_small = 1;
    int fuse_binfilter = 1;  // tuning "contact_fuse_binfilter": binning and prefilter in one launch

    // events and per-node gather over the touched nodes
    long long cap = 0;
    DevBuf<unsigned int> d_ctl;     // kCtl control words (events, max events, dirty, touched counts)
    DevBuf<unsigned int> d_evs;     // [kEvShards][kShardStride] event counters (one per shard)
    DevBuf<int> d_ev_nodes;         // [cap][4]
    DevBuf<double> d_ev_f;          // [cap][3]
    DevBuf<int> d_cnt;              // [nN] terms per node (zero between steps)
    DevBuf<int> d_tpos;             // [nN] position of a touched node in its list
    DevBuf<int> d_touched[2];       // ping-pong lists of nodes with contact force
    int tsel = 0;
    long long tcap = 0;
    DevBuf<int> d_toff;             // [tcap] start of each touched node's term range
    DevBuf<int> d_tcnt;             // [tcap] its length
    DevBuf<ck::TriRec> d_cand;      // [cand_cap] the triangles passing the prefilter, in
                                    // kCandShards shards of cshard_cap records
    long long cand_cap = 0, cshard_cap = 0;
    DevBuf<unsigned int> d_ccnt;    // [kCandShards * kShardStride] candidate count of each shard (word
                                    // 0) and item count (word kItemWord)
    DevBuf<uint2> d_item;           // [kCandShards][kItemsPerCand * cshard_cap] (candidate slot, cell << 27 |
                                    // bucket): the cells of a candidate's neighbourhood that its sphere reaches
    DevBuf<double> d_terms;         // [4 cap][3]
    DevBuf<double> d_fext;          // [nN][3] external force (hakai_ctx::d_fext points here)
    // velocity before the first step (initial condition / uploaded), v2/HAKAI_j.jl:233-239
    DevBuf<double> d_velo0;
    bool use_velo0 = true;
    double min_size = 0, max_size = 0, d_lim = 0;
    double myu = 0.25, kc_o = 1.0, kc_s = 1.0, Cr_o = 0.0, Cr_s = 0.0;  // :2255-2259
    std::vector<int> pair_inst;  // [npairs][2] (1-based instances), for hakai_contact_info
    std::vector<long long> pair_counts;  // [npairs][3] initial #nodes_i, #triangles, #nodes_j
};

// ---- hakai_contact.hip, launched by the multi-GPU phases too (each kernel is defined once) ----
int contact_setup(hakai_ctx* c, const ContactInput& in, ContactPlan& P);
ck::StepIn step_in(hakai_ctx* c, double t, double d_time);  // the one-GPU arrays
// host state at the start of step t (touched-list flip, last step); true: full live-list rebuild
bool step_begin(Contact* C, int t);
// k_ct_reset onto the box array bbox (multi-GPU: g2l, and the bin block header it zeroes)
void launch_reset(hakai_ctx* c, unsigned long long* bbox, bool rebuild, const int* del_any, int t, const int* g2l,
                  int* zero_hdr);
// live lists for step t from the deletion steps del_step: the full rebuild, the append of the
// entries the listed deletions expose
void live_rebuild(hakai_ctx* c, const int* del_step, int t);
void live_append(hakai_ctx* c, const int* del_step, int t);
void launch_boxes(hakai_ctx* c, const ck::StepIn& in, unsigned long long* bbox);  // k_ct_bbox
unsigned filter_grid(const Contact* C);
void tri_prefilter(hakai_ctx* c, const ck::StepIn& in, const unsigned long long* bbox);
void tri_search(hakai_ctx* c, const ck::StepIn& in);
void launch_alloc(hakai_ctx* c);                  // k_ct_alloc
void launch_sum(hakai_ctx* c, const int* g2l);    // k_ct_sum

// ---- hakai_contact_xr.hip (every one with c->contact->xr set) ----
int xr_a1(hakai_ctx* c, double t, double d_time);  // phases of a step, hakai_internal.hpp contact_phase
int xr_a2(hakai_ctx* c, double d_time);
int xr_a3(hakai_ctx* c, double d_time);
int xr_state_reset(hakai_ctx* c);
void xr_after_overflow(hakai_ctx* c);
int xr_tuning(hakai_ctx* c, const char* key, long long value);  // the contact_exchange_* keys
void xr_event_cap(Contact* C);                    // the event buffer changed: clamp the event blocks
int xr_check(hakai_ctx* c);
int xr_stats(hakai_ctx* c, long long* binned, long long* bytes, long long* rec_bytes);
void xr_destroy(Contact* C);

}  // namespace hkc
