// hakai_contact.hip -- all-exterior instance-vs-instance contact on gfx950.
//
// Reference: v2/HAKAI_j.jl (v2 = HAKAI-v0.0.2/Julia)
//   surface update   :766-804   (after element deletion; setup and the surface functions:
//                               hakai_contact_plan.hpp, where the contact model is planned)
//   cal_contact_force:2248-2706 (CPU path; the CUDA.jl path :2899-3157 deliberately differs, §9 Q14)
//   accumulation     :435, :511-538  (Float128 per thread, rounded once into external_force)
//
// Design (MI355X-first, same results):
//   * The contact lists the reference grows at run time (appending newly exposed faces when an
//     element is deleted) are enumerated ONCE on the host: every triangle / contact node that can
//     ever appear carries the elements whose deletion adds it. On the device an entry is live at
//     step t iff it was in the initial list or one of its adders was deleted before t (del_step).
//     Same sets as the reference at every step, no host round trip, no reallocation.
//   * The reference's candidate filter |cell(j0) - cell(i)| <= 1 per axis (cells of size
//     1.1*elementMaxSize, 0.6 for self-contact) becomes a hash grid over the i-nodes: a triangle
//     visits the distinct buckets of the 27 neighbouring cells and applies the exact same integer
//     test, so the candidate set is identical and the work is O(contact nodes), not O(T x N).
//   * Every contact event computes the reference's FP64 expressions verbatim (no contraction).
//     Forces are gathered per node and summed in double-double, then rounded once: the reference
//     sums in Float128 and rounds once, so both are the correctly rounded sum up to a 2^-106
//     relative window (order-independent, no atomics on doubles).
//
// This file: the one-GPU step (live lists, boxes, hash grid, prefilter, triangle search, event
// gather, the fused small-deck phases), contact_setup, and the C entry points. The owner-computed
// multi-GPU search is hakai_contact_xr.hip; it launches some of this file's kernels through the
// functions hakai_contact_state.hpp declares. Device code both files call: hakai_contact_dev.hpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "hakai_contact_dev.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace {

using namespace hkc::ck;
using hkc::Contact;
using hkc::PairParam;
using hkc::Seg;
using hkc::Tile;
using hkc::kTile;
using hkc::BEnt;
using hkc::BRec;
using hkc::BVel;


__device__ __forceinline__ bool live(int orig, const int* aptr, const int* add, int k, const int* del_step, int t) {
    if (orig) return true;
    for (int a = aptr[k]; a < aptr[k + 1]; ++a) {
        const int s = del_step[add[a]];  // -1: deleted before an upload_state
        if (s != 0 && s < t) return true;
    }
    return false;
}

// Step prologue: pair boxes to (+inf, -inf), event counter to 0, full rebuild if the host forces
// it, incremental update if an element was deleted in the previous step (del_any == t-1), and
// the contact forces of the previous step's touched nodes back to 0 (external_force is otherwise
// never rewritten).
// The per-step kernels below are bodies over (workgroup bid of nb): the __global__ wrappers pass
// blockIdx.x / gridDim.x, and the fused small-deck kernels (one workgroup, "Small decks") run
// several bodies back to back with a workgroup barrier between them.
// (multi-GPU: the touched nodes are global ids of this rank's nodes, g2l maps them into fext)
__device__ __forceinline__ void reset_body(int bid, int nb, unsigned long long* bbox, int npairs, unsigned int* ctl,
                                           unsigned int* evs, unsigned int* ccnt, int force, const int* del_any,
                                           int t, const double* t_rd, const int* touched_prev, int tsel,
                                           double* fext, const int* g2l = nullptr, int* zero_hdr = nullptr) {
    if (t_rd) t = (int)*t_rd + 1;  // graph mode: step number from the device counter
    const int i = bid * blockDim.x + threadIdx.x;
    if (zero_hdr && i < 2) zero_hdr[i] = 0;  // multi-GPU: this step's bin block (count, overflow)
    if (i < kEvShards) evs[i * kShardStride] = 0;
    if (i < kCandShards)
        ccnt[i * kShardStride] = ccnt[i * kShardStride + kTestWord] = ccnt[i * kShardStride + kItemWord] = 0;
    for (int q = i; q < box_words(npairs); q += nb * blockDim.x) bbox[q] = box_max(q) ? 0ULL : ~0ULL;
    if (i == 0) {
        ctl[kEv] = 0;
        ctl[kDirty] = force ? 1u : 0u;
        ctl[kDel] = (!force && del_any && *del_any == t - 1) ? 1u : 0u;
        ctl[kNdel] = 0;
        ctl[kNcand] = 0;
        ctl[kCandOver] = 0;
        ctl[kTerms] = 0;
        ctl[kTouched + tsel] = 0;
        ctl[kSeq] = ctl[kSeq] + 1u;  // this step's bucket-head stamp (never 0: the heads start at 0)
    }
    const int np = (int)ld_ctl(&ctl[kTouched + 1 - tsel]);
    for (int q = i; q < np; q += nb * blockDim.x) {
        const long long n = g2l ? g2l[touched_prev[q]] : touched_prev[q];  // (multi-GPU: only local nodes)
        fext[3 * n] = 0.0;
        fext[3 * n + 1] = 0.0;
        fext[3 * n + 2] = 0.0;
    }
}

__global__ void k_ct_reset(unsigned long long* bbox, int npairs, unsigned int* ctl, unsigned int* evs,
                           unsigned int* ccnt, int force, const int* del_any, int t, const double* t_rd,
                           const int* touched_prev, int tsel, double* fext, const int* g2l, int* zero_hdr) {
    reset_body(blockIdx.x, gridDim.x, bbox, npairs, ctl, evs, ccnt, force, del_any, t, t_rd, touched_prev, tsel,
               fext, g2l, zero_hdr);
}

// ---- live lists -----------------------------------------------------------------------------
// Every node entry / triangle that can ever appear is enumerated at setup (most of them are
// interior and only become live if elements are deleted). The live ones are kept in index lists,
// one region per pair side's node segment (at the segment's own offset, capacity = segment size)
// and one for all triangles; reg[2r] = region base, reg[2r+1] = live count. Like the reference's
// c_nodes / c_triangles they only grow (:766-804): a deletion appends the entries it exposes
// (k_ct_append); triangles of deleted elements stay listed and are skipped at use (:2374-2377).
// A full rebuild (setup, state upload/reset, a probe, a non-consecutive step) scans everything
// in tiles of kTile entries that never straddle a region. Lists: 0 i-nodes, 1 j-nodes, 2 triangles.
constexpr int kTilePer = 8;
static_assert(kTile == kB * kTilePer, "a tile is one block's pass");

struct LiveIn {
    const int *ni_orig, *ni_aptr, *ni_add, *nj_orig, *nj_aptr, *nj_add, *tri_ele, *tri_adder, *flag, *del_step;
    int t;
};

__device__ __forceinline__ bool is_live(const LiveIn& L, int list, int k) {
    if (list == 0) return live(L.ni_orig[k], L.ni_aptr, L.ni_add, k, L.del_step, L.t);
    if (list == 1) return live(L.nj_orig[k], L.nj_aptr, L.nj_add, k, L.del_step, L.t);
    const int ad = L.tri_adder[k];
    if (ad < 0) return true;
    const int st = L.del_step[ad];
    return st != 0 && st < L.t;  // face exposed by a deletion in an earlier step
}

// block-wide exclusive scan of one int per thread (blockDim.x <= 1024 threads, s_w[blockDim.x/64]);
// returns this thread's exclusive prefix, total = the block's sum
__device__ __forceinline__ int block_excl_scan(int v, int* s_w, int& total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int x = v;
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (lane == 63) s_w[w] = x;
    __syncthreads();
    int base = 0, tot = 0;
    const int nw = (int)blockDim.x >> 6;
    for (int q = 0; q < nw; ++q) {
        base += q < w ? s_w[q] : 0;
        tot += s_w[q];
    }
    __syncthreads();
    total = tot;
    return base + x - v;
}

__global__ __launch_bounds__(kB) void k_ct_live_count(const unsigned int* ctl, LiveIn L, const Tile* tiles,
                                                      int ntile, int* tile_cnt) {
    if (ctl[kDirty] == 0) return;
    __shared__ int s_w[kB / 64];
    for (int b = blockIdx.x; b < ntile; b += gridDim.x) {
        const Tile tl = tiles[b];
        int n = 0;
        for (int q = 0; q < kTilePer; ++q) {
            const int k = tl.start + (int)threadIdx.x + kB * q;
            if (k < tl.end && is_live(L, tl.list, k)) ++n;
        }
        int tot;
        block_excl_scan(n, s_w, tot);
        if (threadIdx.x == 0) tile_cnt[b] = tot;
    }
}

// one block: exclusive scan of the tile counts (tile_off[0..ntile]); region r = tiles
// [reg_first[r], reg_first[r+1]) -> reg[2r+1] = its live count
__global__ __launch_bounds__(kB) void k_ct_live_scan(const unsigned int* ctl, int ntile, const int* tile_cnt,
                                                     int* tile_off, int nreg, const int* reg_first, int* reg) {
    if (ctl[kDirty] == 0) return;
    __shared__ int s_w[kB / 64];
    int carry = 0;
    constexpr int PER = 16;
    for (int c0 = 0; c0 < ntile; c0 += kB * PER) {
        const int b = c0 + (int)threadIdx.x * PER;
        int v[PER], sum = 0;
        for (int q = 0; q < PER; ++q) {
            v[q] = b + q < ntile ? tile_cnt[b + q] : 0;
            sum += v[q];
        }
        int tot;
        int run = carry + block_excl_scan(sum, s_w, tot);
        for (int q = 0; q < PER; ++q) {
            if (b + q < ntile) tile_off[b + q] = run;
            run += v[q];
        }
        carry += tot;
    }
    if (threadIdx.x == 0) tile_off[ntile] = carry;
    __syncthreads();  // this block's global stores are visible to its own threads after the barrier
    for (int r = threadIdx.x; r < nreg; r += kB) reg[2 * r + 1] = tile_off[reg_first[r + 1]] - tile_off[reg_first[r]];
}

__global__ __launch_bounds__(kB) void k_ct_live_write(const unsigned int* ctl, LiveIn L, const Tile* tiles,
                                                      int ntile, const int* tile_off, const int* reg_first,
                                                      const int* reg, int* out_ni, int* out_nj, int* out_tri) {
    if (ctl[kDirty] == 0) return;
    __shared__ int s_w[kB / 64];
    for (int b = blockIdx.x; b < ntile; b += gridDim.x) {
        const Tile tl = tiles[b];
        const int k0 = tl.start + (int)threadIdx.x * kTilePer;
        unsigned m = 0;
        int n = 0;
        for (int q = 0; q < kTilePer; ++q) {
            const int k = k0 + q;
            if (k < tl.end && is_live(L, tl.list, k)) {
                m |= 1u << q;
                ++n;
            }
        }
        int tot;
        int o = block_excl_scan(n, s_w, tot) + reg[2 * tl.region] + tile_off[b] - tile_off[reg_first[tl.region]];
        int* out = tl.list == 0 ? out_ni : (tl.list == 1 ? out_nj : out_tri);
        for (int q = 0; q < kTilePer; ++q)
            if (m >> q & 1) out[o++] = k0 + q;
    }
}

// incremental update, part 1: the elements deleted in the previous step (int4 sweep of del_step)
__device__ __forceinline__ void find_del_body(int bid, int nb, unsigned int* ctl, const int* del_step, int nE, int t,
                                              const double* t_rd, int* dlist) {
    if (ld_ctl(&ctl[kDel]) == 0) return;
    if (t_rd) t = (int)*t_rd + 1;
    const int n4 = nE >> 2;
    const int4* d4 = reinterpret_cast<const int4*>(del_step);
    for (int v = bid * blockDim.x + threadIdx.x; v < n4; v += nb * blockDim.x) {
        const int4 d = d4[v];
        if (d.x == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = 4 * v;
        if (d.y == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = 4 * v + 1;
        if (d.z == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = 4 * v + 2;
        if (d.w == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = 4 * v + 3;
    }
    if (bid == 0 && (int)threadIdx.x < nE - 4 * n4) {
        const int e = 4 * n4 + (int)threadIdx.x;
        if (del_step[e] == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = e;
    }
}

__global__ void k_ct_find_del(unsigned int* ctl, const int* del_step, int nE, int t, const double* t_rd, int* dlist) {
    find_del_body(blockIdx.x, gridDim.x, ctl, del_step, nE, t, t_rd, dlist);
}

// a node entry becomes live with the first deletion among its adders; of several adders deleted in
// the same step, the lowest element id appends it
__device__ __forceinline__ bool newly_live(const int* orig, const int* aptr, const int* add, int k, int e,
                                           const int* del_step, int t) {
    if (orig[k]) return false;
    for (int a = aptr[k]; a < aptr[k + 1]; ++a) {
        const int ad = add[a], st = del_step[ad];
        if (st != 0 && st < t - 1) return false;  // live before (st = -1: deleted before an upload)
        if (st == t - 1 && ad < e) return false;
    }
    return true;
}

struct AppendIn {
    const int *el_tri_ptr, *el_tri, *el_ni_ptr, *el_ni, *el_nj_ptr, *el_nj;
    const int *ni_orig, *ni_aptr, *ni_add, *ni_pair, *nj_orig, *nj_aptr, *nj_add, *nj_pair;
    const int* pair_reg;  // [npairs][2] region of (pair, side), -1 if none
    int tri_reg;
};

// incremental update, part 2: one block per deleted element, one thread per entry its deletion
// exposes (triangles, then i-node entries, then j-node entries)
// (lanes lt of lsz per deleted element: a workgroup, or a wave of a one-workgroup kernel)
__device__ __forceinline__ void append_body(int bid, int nb, unsigned int* ctl, const int* dlist, const AppendIn& A,
                                            const int* del_step, int t, const double* t_rd, int* reg, int* ni_live,
                                            int* nj_live, int* tri_live, int lt, int lsz) {
    if (ld_ctl(&ctl[kDel]) == 0) return;
    if (t_rd) t = (int)*t_rd + 1;
    const int nd = (int)ld_ctl(&ctl[kNdel]);
    for (int q = bid; q < nd; q += nb) {
        const int e = dlist[q];
        const int t0 = A.el_tri_ptr[e], nt = A.el_tri_ptr[e + 1] - t0;
        const int i0 = A.el_ni_ptr[e], ni = A.el_ni_ptr[e + 1] - i0;
        const int j0 = A.el_nj_ptr[e], nj = A.el_nj_ptr[e + 1] - j0;
        for (int x = lt; x < nt + ni + nj; x += lsz) {
            if (x < nt) {  // unique adder per triangle
                tri_live[atomicAdd(&reg[2 * A.tri_reg + 1], 1)] = A.el_tri[t0 + x];
            } else if (x < nt + ni) {
                const int k = A.el_ni[i0 + x - nt];
                if (!newly_live(A.ni_orig, A.ni_aptr, A.ni_add, k, e, del_step, t)) continue;
                const int r = A.pair_reg[2 * A.ni_pair[k]];
                ni_live[reg[2 * r] + atomicAdd(&reg[2 * r + 1], 1)] = k;
            } else {
                const int k = A.el_nj[j0 + x - nt - ni];
                if (!newly_live(A.nj_orig, A.nj_aptr, A.nj_add, k, e, del_step, t)) continue;
                const int r = A.pair_reg[2 * A.nj_pair[k] + 1];
                nj_live[reg[2 * r] + atomicAdd(&reg[2 * r + 1], 1)] = k;
            }
        }
    }
}

__global__ void k_ct_append(unsigned int* ctl, const int* dlist, AppendIn A, const int* del_step, int t,
                            const double* t_rd, int* reg, int* ni_live, int* nj_live, int* tri_live) {
    append_body(blockIdx.x, gridDim.x, ctl, dlist, A, del_step, t, t_rd, reg, ni_live, nj_live, tri_live,
                (int)threadIdx.x, (int)blockDim.x);
}

// bounding boxes of the live node lists per pair (:2281-2299). Segment = the live node entries of
// one pair side. kSegBlocks blocks per segment reduce in registers, then across the block
// (shuffles + LDS), then issue ONE atomic per bound.
constexpr int kSegBlocks = 256;


// segment vb / sb, part vb % sb
__device__ __forceinline__ void bbox_body(int vb, int sb, const StepIn& s, const Seg* segs, const int* reg,
                                          const int* ni_live, const int* nj_live, const int* ni_node,
                                          const int* nj_node, unsigned long long* bbox) {
    const Seg sg = segs[vb / sb];
    if (sg.dup) return;  // another segment's blocks fill its boxes
    const int sub = vb % sb;
    const bool side_i = sg.side == 0;
    const int* node = side_i ? ni_node : nj_node;
    const int* lst = (side_i ? ni_live : nj_live) + reg[2 * sg.region];
    const int cnt = reg[2 * sg.region + 1];
    const int bd = (int)blockDim.x;
    unsigned long long mn[3] = {~0ULL, ~0ULL, ~0ULL}, mx[3] = {0ULL, 0ULL, 0ULL};
#pragma unroll 4
    for (int q = sub * bd + (int)threadIdx.x; q < cnt; q += sb * bd) {  // iterations overlap their loads
        double p[3];
        pos(s, node[lst[q]], p);
        for (int d = 0; d < 3; ++d) {
            const unsigned long long e = enc(p[d]);
            mn[d] = umin64(mn[d], e);
            mx[d] = umax64(mx[d], e);
        }
    }
    for (int off = 32; off > 0; off >>= 1)
        for (int d = 0; d < 3; ++d) {
            mn[d] = umin64(mn[d], __shfl_xor(mn[d], off));
            mx[d] = umax64(mx[d], __shfl_xor(mx[d], off));
        }
    __shared__ unsigned long long red[16][6];
    const int w = threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0)
        for (int d = 0; d < 3; ++d) {
            red[w][d] = mn[d];
            red[w][3 + d] = mx[d];
        }
    __syncthreads();
    if (threadIdx.x < 6) {
        const int q = threadIdx.x;
        unsigned long long v = red[0][q];
        for (int ww = 1; ww < bd / 64; ++ww) v = q < 3 ? umin64(v, red[ww][q]) : umax64(v, red[ww][q]);
        for (int a = -1; a < 2; ++a) {  // own slot, then the duplicates'
            const int off = a < 0 ? 12 * sg.pair + (side_i ? 0 : 6) : sg.alias[a];
            if (off < 0) continue;
            unsigned long long* bb = bbox + off;
            if (q < 3) {
                if (v != ~0ULL) atomicMin(&bb[q], v);
            } else if (v != 0ULL) {
                atomicMax(&bb[q], v);
            }
        }
    }
}

__global__ __launch_bounds__(kB) void k_ct_bbox(StepIn s, const Seg* segs, const int* reg, const int* ni_live,
                                                const int* nj_live, const int* ni_node, const int* nj_node,
                                                unsigned long long* bbox, int sb) {
    bbox_body(blockIdx.x, sb, s, segs, reg, ni_live, nj_live, ni_node, nj_node, bbox);
}

// cells of the live i-nodes inside the pair's range box (:2333-2346) -> the hash grid, each binned
// node at its live-list position in the bucket list. vb = virtual block (segment vb / sb, part
// vb % sb); a launch of nseg * sb workgroups has one each.
__device__ __forceinline__ void bin_body(int vb, const StepIn& s, const Seg* segs, const int* reg, const int* ni_live,
                                         const int* ni_pair, const int* ni_node, const PairParam* par,
                                         const unsigned long long* bbox, const unsigned int* ctl,
                                         unsigned long long* head, BEnt* blist, BVel* bvel, int sb) {
#pragma clang fp contract(off)
    const Seg sg = segs[vb / sb];
    if (sg.side != 0) return;
    const int base = reg[2 * sg.region], n = reg[2 * sg.region + 1];
    const int bd = (int)blockDim.x;
    const unsigned seq = ctl[kSeq];
    for (int q = (vb % sb) * bd + (int)threadIdx.x; q < n; q += sb * bd) {
        const int k = ni_live[base + q];
        const int pr = ni_pair[k];
        const Range r = pair_range(bbox + 12 * pr);
        const int nd = ni_node[k];
        const PairParam pp = par[pr];  // loaded with the box, not behind the range test
        double p[3];
        pos(s, nd, p);
        if (r.empty || p[0] < r.mn[0] || p[1] < r.mn[1] || p[2] < r.mn[2] || p[0] > r.mx[0] || p[1] > r.mx[1] ||
            p[2] > r.mx[2])  // the candidate test of :2514-2519, applied before binning
            continue;
        BRec e;
        bin_rec(s, r, pp, pr, nd, p, e);
        const int b = pp.hash_off + (int)(hash3(e.e.m[0], e.e.m[1], e.e.m[2]) & (unsigned)(pp.hash_size - 1));
        bucket_push(head, b, seq, base + q, e.e, e.w, blist, bvel);  // coalesced by live position
    }
}

__global__ __launch_bounds__(kB) void k_ct_bin(StepIn s, const Seg* segs, const int* reg, const int* ni_live,
                                               const int* ni_pair, const int* ni_node, const PairParam* par,
                                               const unsigned long long* bbox, const unsigned int* ctl,
                                               unsigned long long* head, BEnt* blist, BVel* bvel, int sb) {
    bin_body(blockIdx.x, s, segs, reg, ni_live, ni_pair, ni_node, par, bbox, ctl, head, blist, bvel, sb);
}

__global__ __launch_bounds__(kB) void k_ct_tri_filter(StepIn s, const int* tri_cnt, const int* tri_live,
                                                      const int* tri_pair, const int* tri_nodes, const int* tri_ele,
                                                      const PairParam* par, const unsigned long long* bbox,
                                                      unsigned int* ccnt, TriRec* cand, long long cshard_cap,
                                                      uint2* item) {
    tri_filter_body(blockIdx.x, gridDim.x, s, tri_cnt, tri_live, tri_pair, tri_nodes, tri_ele, par, bbox, ccnt, cand,
                    cshard_cap, item);
}

// events of one thread, kept in registers and appended with one atomic per wave (a same-address
// atomic per event serialised the kernel); more than kEvLocal go out one by one
constexpr int kEvLocal = 4;
struct EvBuf {
    int n, j0, j1, j2;
    int i[kEvLocal];
    double f[kEvLocal][3];
};

__device__ __forceinline__ void ev_write(int* ev_nodes, double* ev_f, long long e, int i, int j0, int j1, int j2,
                                         double fx, double fy, double fz) {
    int* en = ev_nodes + 4 * e;
    en[0] = i;
    en[1] = j0;
    en[2] = j1;
    en[3] = j2;
    double* ef = ev_f + 3 * e;
    ef[0] = fx;
    ef[1] = fy;
    ef[2] = fz;
}

// one bucket entry: its four 16-B vectors are issued together and pinned (the asm), so the
// compiler cannot split the record into per-field loads sunk behind the tests that use them --
// that made every entry a chain of four dependent round trips
__device__ __forceinline__ BEnt ld_bent(const BEnt* e) {
    const uint4* q = reinterpret_cast<const uint4*>(e);
    const uint4 w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
    asm volatile("" ::"v"(w0.x), "v"(w1.x), "v"(w2.x), "v"(w3.x));
    BEnt r;
    r.m[0] = ll2(w0.x, w0.y);
    r.m[1] = ll2(w0.z, w0.w);
    r.m[2] = ll2(w1.x, w1.y);
    r.node = (int)w1.z;
    r.pad = (int)w1.w;
    r.p[0] = __longlong_as_double(ll2(w2.x, w2.y));
    r.p[1] = __longlong_as_double(ll2(w2.z, w2.w));
    r.p[2] = __longlong_as_double(ll2(w3.x, w3.y));
    r.next = ll2(w3.z, w3.w);
    return r;
}

// one (candidate triangle, neighbour cell) pair: the rest of the loop body at :2371-2698 for the
// i-nodes of cell mj (one of the 27 around the triangle's first node), found in hash bucket b.
template <bool EXACT_CELL>
__device__ __forceinline__ void tri_cell(const StepIn& s, const TriRec* __restrict__ rec, const long long mj[3],
                                         int b, unsigned seq, const PairParam* par, const unsigned long long* head,
                                         const BEnt* __restrict__ blist, const BVel* __restrict__ bvel, double d_lim,
                                         double myu, unsigned int* evn, long long cap, int* ev_nodes, double* ev_f,
                                         EvBuf& eb) {
#pragma clang fp contract(off)
    const int pr = rec->pr;
    const unsigned long long h = head[b];
    const int first = (unsigned)(h >> 32) == seq ? (int)(unsigned)h : -1;  // an older stamp: empty
    // self contact: the triangle's element's own nodes are skipped (:2496-2507); loaded once
    const bool self = rec->self;
    int own8[8];
    if (self) {
        const int* cn = s.conn + 8 * (long long)rec->eleid;
#pragma unroll
        for (int a = 0; a < 8; ++a) own8[a] = gid(s, cn[a]);
    }
    // the point-independent part of the test, held in registers for the whole bucket
    const double c0 = rec->c[0], c1 = rec->c[1], c2 = rec->c[2], Rmax = rec->Rmax;
    const double q00 = rec->q0[0], q01 = rec->q0[1], q02 = rec->q0[2], vdet = rec->vdet;
    double im[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) im[k] = rec->im[k];
    int nxt = -1;
    for (int sl = first; sl >= 0; sl = nxt) {
        const BEnt be = ld_bent(blist + sl);
        nxt = (int)be.next;
        const int i = be.node;
        // branch-free cell and self tests: no load waits behind a branch. EXACT_CELL (search items):
        // only the bucket's entries of this very cell (other cells' entries are found through their
        // own item, if their cell is searched at all); else (32 lanes per candidate, each bucket
        // visited once) every entry of the 27-neighbourhood of the first-node cell mj
        bool skip = EXACT_CELL
                        ? ((int)(mj[0] != be.m[0]) | (int)(mj[1] != be.m[1]) | (int)(mj[2] != be.m[2])) != 0
                        : ((int)(llabs(mj[0] - be.m[0]) > 1) | (int)(llabs(mj[1] - be.m[1]) > 1) |
                           (int)(llabs(mj[2] - be.m[2]) > 1)) != 0;
        if (self) {
#pragma unroll
            for (int a = 0; a < 8; ++a) skip |= (i == own8[a]);
        }
        if (skip) continue;
        const double p[3] = {be.p[0], be.p[1], be.p[2]};
        const double dpc = my3norm(p[0] - c0, p[1] - c1, p[2] - c2);
        if (dpc >= Rmax) continue;
        const double bx = p[0] - q00, by = p[1] - q01, bz = p[2] - q02;
        const double x1 = (im[0] * bx + im[1] * by + im[2] * bz) / vdet;
        const double x2 = (im[3] * bx + im[4] * by + im[5] * bz) / vdet;
        const double d = (im[6] * bx + im[7] * by + im[8] * bz) / vdet;
        if (!(0.0 <= x1 && 0.0 <= x2 && x1 + x2 <= 1.0 && d > 0.0 && d <= d_lim)) continue;
        const int j0 = rec->j0, j1 = rec->j1, j2 = rec->j2;
        const double nx = rec->n[0], ny = rec->n[1], nz = rec->n[2], kk = rec->kk;
        // velo = d_disp / d_time of the previous step (:628), the IC before step 1: formed by the
        // binning (i) and the prefilter (j0)
        const BVel w = bvel[sl];
        const double vx = w.v[0] - rec->vj[0], vy = w.v[1] - rec->vj[1], vz = w.v[2] - rec->vj[2];
        const double mag_v = my3norm(vx, vy, vz);
        double vex = 0.0, vey = 0.0, vez = 0.0;
        if (mag_v > 0.0) {
            vex = vx / mag_v;
            vey = vy / mag_v;
            vez = vz / mag_v;
        }
        const double F = kk * d;
        double fx = F * nx, fy = F * ny, fz = F * nz;
        // damping: diag_M[i] indexes the dof vector with a node id (:2592)
        const double Cd = 2 * sqrt(w.mq * kk) * par[pr].Cr;
        const double fc_x = -Cd * vx, fc_y = -Cd * vy, fc_z = -Cd * vz;
        const double dot_ve_n = vex * nx + vey * ny + vez * nz;
        const double vsx = vex - dot_ve_n * nx, vsy = vey - dot_ve_n * ny, vsz = vez - dot_ve_n * nz;
        const double fric_x = -myu * F * vsx, fric_y = -myu * F * vsy, fric_z = -myu * F * vsz;
        fx += fric_x + fc_x;
        fy += fric_y + fc_y;
        fz += fric_z + fc_z;
        if (eb.n < kEvLocal) {
            eb.j0 = j0;
            eb.j1 = j1;
            eb.j2 = j2;
#pragma unroll
            for (int u = 0; u < kEvLocal; ++u)
                if (u == eb.n) {
                    eb.i[u] = i;
                    eb.f[u][0] = fx;
                    eb.f[u][1] = fy;
                    eb.f[u][2] = fz;
                }
            ++eb.n;
        } else {  // evn: this wave's shard counter, cap: the shard's capacity, ev_*: the shard's slots
            const unsigned e = atomicAdd(evn, 1u);
            if ((long long)e < cap) ev_write(ev_nodes, ev_f, e, i, j0, j1, j2, fx, fy, fz);
        }
    }
}

// the wave's buffered events -> its event shard, one atomic per wave (every lane calls it)
__device__ __forceinline__ void ev_flush(const EvBuf& eb, int lane, unsigned int* evn, long long shard_cap,
                                         int* sh_nodes, double* sh_f) {
    const int c = eb.n < kEvLocal ? eb.n : kEvLocal;
    int x = c;  // wave inclusive scan of the buffered counts
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    if (__builtin_amdgcn_readlane(x, 63) == 0) return;  // wave-uniform: no events
    unsigned base = 0;
    if (lane == 63) base = atomicAdd(evn, (unsigned)x);
    base = __shfl(base, 63) + (unsigned)(x - c);
#pragma unroll
    for (int u = 0; u < kEvLocal; ++u)
        if (u < c && (long long)(base + u) < shard_cap)
            ev_write(sh_nodes, sh_f, base + u, eb.i[u], eb.j0, eb.j1, eb.j2, eb.f[u][0], eb.f[u][1], eb.f[u][2]);
}

// one lane per search item (candidate triangle, cell): the prefilter listed only the cells its
// sphere reaches, so no lane is idle and no bucket needs deduplicating (each item takes its own
// cell's entries)
__device__ __forceinline__ void tri_body(const StepIn& s, unsigned int* ctl, const unsigned int* ccnt,
                                         const TriRec* cand, long long cshard_cap, const uint2* item,
                                         const PairParam* par, const unsigned long long* head, const BEnt* blist,
                                         const BVel* bvel, double d_lim, double myu, unsigned int* evs,
                                         long long shard_cap, int* ev_nodes, double* ev_f) {
    __shared__ unsigned s_cpre[kCandShards + 4], s_ipre[kCandShards + 4];
    (void)shard_scan(ccnt, cshard_cap, s_cpre);
    const long long icap = kItemsPerCand * cshard_cap;
    const long long n = shard_scan(ccnt + kItemWord, icap, s_ipre);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // totals for the stats, the overflow check and the poison
        ctl[kNcand] = s_cpre[kCandShards + 2];
        atomicMax(&ctl[kNcandMax], s_cpre[kCandShards + 2]);
        atomicMax(&ctl[kCandShardMax], s_cpre[kCandShards + 3]);
        atomicMax(&ctl[kItemShardMax], s_ipre[kCandShards + 3]);  // search items: own buffer, own report
        ctl[kCandOver] = s_cpre[kCandShards + 1] | s_ipre[kCandShards + 1];
    }
    const int lane = (int)(threadIdx.x & 63);
    const unsigned seq = ctl[kSeq];
    const int shard = (int)(((blockIdx.x * blockDim.x + threadIdx.x) >> 6) % kEvShards);
    unsigned int* evn = evs + shard * kShardStride;
    int* sh_nodes = ev_nodes + 4 * (long long)shard * shard_cap;
    double* sh_f = ev_f + 3 * (long long)shard * shard_cap;
    for (long long q0 = blockIdx.x * (long long)blockDim.x; q0 < n; q0 += (long long)gridDim.x * blockDim.x) {
        const long long q = q0 + threadIdx.x;  // wave-uniform trip count (the append below is wave-wide)
        EvBuf eb;
        eb.n = 0;
        eb.j0 = eb.j1 = eb.j2 = 0;
        if (q < n) {
            const uint2 it = item[shard_slot(s_ipre, icap, q)];
            const TriRec* rec = cand + it.x;
            const int dc = (int)(it.y >> 27);
            const long long cell[3] = {rec->mj[0] + (dc % 3 - 1), rec->mj[1] + ((dc / 3) % 3 - 1),
                                       rec->mj[2] + (dc / 9 - 1)};
            tri_cell<true>(s, rec, cell, (int)(it.y & ((1u << 27) - 1u)), seq, par, head, blist, bvel, d_lim, myu,
                           evn, shard_cap, sh_nodes, sh_f, eb);
        }
        ev_flush(eb, lane, evn, shard_cap, sh_nodes, sh_f);
    }
}

__global__ __launch_bounds__(128) void k_ct_tri(StepIn s, unsigned int* ctl, const unsigned int* ccnt,
                                                const TriRec* cand, long long cshard_cap, const uint2* item,
                                                const PairParam* par, const unsigned long long* head,
                                                const BEnt* blist, const BVel* bvel, double d_lim, double myu,
                                                unsigned int* evs, long long shard_cap, int* ev_nodes, double* ev_f) {
    tri_body(s, ctl, ccnt, cand, cshard_cap, item, par, head, blist, bvel, d_lim, myu, evs, shard_cap, ev_nodes, ev_f);
}

// Small decks: 32 lanes per candidate triangle (27 cells used), lane c takes cell c (dz, dy, dx in the
// reference's loop order); a cell whose bucket a lower cell of the same triangle maps to is
// skipped, so every bucket is visited once (buckets compared across lanes, readlane). No search
// items: at a few hundred candidates the prefilter's item pass costs more than idle lanes do.
__global__ __launch_bounds__(128) void k_ct_tri32(StepIn s, unsigned int* ctl, const unsigned int* ccnt,
                                                  const TriRec* cand, long long cshard_cap, const PairParam* par,
                                                  const unsigned long long* head, const BEnt* blist, const BVel* bvel,
                                                  double d_lim, double myu, unsigned int* evs, long long shard_cap,
                                                  int* ev_nodes, double* ev_f) {
    __shared__ unsigned s_cpre[kCandShards + 4];
    const long long n = 32LL * shard_scan(ccnt, cshard_cap, s_cpre);
    if (blockIdx.x == 0 && threadIdx.x == 0) {  // totals for the stats, the overflow check and the poison
        ctl[kNcand] = s_cpre[kCandShards + 2];
        atomicMax(&ctl[kNcandMax], s_cpre[kCandShards + 2]);
        atomicMax(&ctl[kCandShardMax], s_cpre[kCandShards + 3]);
        ctl[kCandOver] = s_cpre[kCandShards + 1];
    }
    const int lane = (int)(threadIdx.x & 63);
    const unsigned seq = ctl[kSeq];
    const int shard = (int)(((blockIdx.x * blockDim.x + threadIdx.x) >> 6) % kEvShards);
    unsigned int* evn = evs + shard * kShardStride;
    int* sh_nodes = ev_nodes + 4 * (long long)shard * shard_cap;
    double* sh_f = ev_f + 3 * (long long)shard * shard_cap;
    for (long long q0 = blockIdx.x * (long long)blockDim.x; q0 < n; q0 += (long long)gridDim.x * blockDim.x) {
        const long long q = q0 + threadIdx.x;  // wave-uniform trip count (the append below is wave-wide)
        EvBuf eb;
        eb.n = 0;
        eb.j0 = eb.j1 = eb.j2 = 0;
        const int cell = (int)(q & 31);
        const bool valid = q < n && cell < 27;
        const TriRec* rec = cand + (valid ? shard_slot(s_cpre, cshard_cap, q >> 5) : 0);
        long long mj[3] = {0, 0, 0};
        unsigned hb = 0x80000000u | (unsigned)lane;  // never equal to a real bucket (< 2^31)
        int hoff = 0;
        if (valid) {
            hoff = rec->hoff;
            mj[0] = rec->mj[0];
            mj[1] = rec->mj[1];
            mj[2] = rec->mj[2];
            hb = hash3(mj[0] + (cell % 3 - 1), mj[1] + ((cell / 3) % 3 - 1), mj[2] + (cell / 9 - 1)) &
                 (unsigned)rec->hmask;
        }
        bool dup = false;
        const int half = lane & 32;
#pragma unroll
        for (int c2 = 0; c2 < 26; ++c2) {
            const unsigned lo = (unsigned)__builtin_amdgcn_readlane((int)hb, c2);
            const unsigned hi = (unsigned)__builtin_amdgcn_readlane((int)hb, 32 + c2);
            dup |= c2 < cell && (half ? hi : lo) == hb;
        }
        if (valid && !dup)
            tri_cell<false>(s, rec, mj, hoff + (int)hb, seq, par, head, blist, bvel, d_lim, myu, evn, shard_cap,
                            sh_nodes, sh_f, eb);
        ev_flush(eb, lane, evn, shard_cap, sh_nodes, sh_f);
    }
}



// Per-node gather of the event terms over the nodes that received one ("touched", a compact list
// instead of a pass over all nN nodes): count -> per-node term ranges by a wave-aggregated bump
// allocator (ranges are disjoint; their order is irrelevant) -> scatter -> sum.
// Block 0 also poisons the step when a buffer overflowed in it (events beyond a shard, candidate
// triangles beyond their buffer, a truncated multi-GPU mirror block): the nodal, BC, element and
// interface kernels of this and later steps of the call then write nothing (hakai_device.hpp,
// poisoned), so the state stays the last good step's and hakai_step reports the overflow.
__device__ __forceinline__ void count_body(int bid, int nb, unsigned int* ctl, const unsigned int* evs,
                                           long long shard_cap, const int* ev_nodes, int* cnt, int* touched,
                                           int* tpos, int tsel, int* poison, int t, const double* t_rd) {
    __shared__ unsigned s_pre[kEvShards + 4];
    const long long n = 4 * shard_prefix(bid, ctl, evs, shard_cap, s_pre);
    if (bid == 0 && threadIdx.x == 0) {
        const bool over = ctl[kCandOver] != 0 || s_pre[kEvShards + 1];
        if (over && poison[0] == 0) {
            poison[1] = t_rd ? (int)*t_rd + 1 : t;
            poison[0] = 1;
        }
    }
    __shared__ unsigned s_app[2];
    for (long long e0 = bid * (long long)blockDim.x; e0 < n; e0 += (long long)nb * blockDim.x) {
        const long long e = e0 + threadIdx.x;
        int node = -1;
        bool first = false;
        if (e < n) {
            node = ev_nodes[4 * shard_slot(s_pre, shard_cap, e >> 2) + (e & 3)];
            first = atomicAdd(&cnt[node], 1) == 0;
        }
        const unsigned q = block_append(&ctl[kTouched + tsel], first, s_app);
        if (first) {
            touched[q] = node;
            tpos[node] = (int)q;
        }
    }
}

__global__ void k_ct_count(unsigned int* ctl, const unsigned int* evs, long long shard_cap, const int* ev_nodes,
                           int* cnt, int* touched, int* tpos, int tsel, int* poison, int t, const double* t_rd) {
    count_body(blockIdx.x, gridDim.x, ctl, evs, shard_cap, ev_nodes, cnt, touched, tpos, tsel, poison, t, t_rd);
}

__device__ __forceinline__ void alloc_body(int bid, int nb, unsigned int* ctl, int tsel, const int* touched,
                                           const int* cnt, int* toff, int* tcnt) {
    const int nt = (int)ld_ctl(&ctl[kTouched + tsel]);
    const int lane = (int)(threadIdx.x & 63);
    for (int q0 = bid * blockDim.x; q0 < nt; q0 += nb * blockDim.x) {
        const int q = q0 + (int)threadIdx.x;
        const int c = q < nt ? cnt[touched[q]] : 0;
        int x = c;  // wave inclusive scan
        for (int o = 1; o < 64; o <<= 1) {
            const int y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        unsigned base = 0;
        if (lane == 63) base = atomicAdd(&ctl[kTerms], (unsigned)x);
        base = __shfl(base, 63);
        if (q < nt) {
            toff[q] = (int)base + x - c;
            tcnt[q] = c;
        }
    }
}

__global__ void k_ct_alloc(unsigned int* ctl, int tsel, const int* touched, const int* cnt, int* toff, int* tcnt) {
    alloc_body(blockIdx.x, gridDim.x, ctl, tsel, touched, cnt, toff, tcnt);
}

__device__ __forceinline__ void scatter_body(int bid, int nb, unsigned int* ctl, const unsigned int* evs,
                                             long long shard_cap, const int* ev_nodes, const double* ev_f,
                                             const int* toff, const int* tpos, int* cnt, double* terms) {
#pragma clang fp contract(off)
    __shared__ unsigned s_pre[kEvShards + 4];
    const long long n = 4 * shard_prefix(bid, ctl, evs, shard_cap, s_pre);
    for (long long e = bid * (long long)blockDim.x + threadIdx.x; e < n; e += (long long)nb * blockDim.x) {
        const long long ev = shard_slot(s_pre, shard_cap, e >> 2);
        const int role = (int)(e & 3);
        const int node = ev_nodes[4 * ev + role];
        const int slot = toff[tpos[node]] + atomicSub(&cnt[node], 1) - 1;  // leaves cnt zeroed
        const double* f = ev_f + 3 * ev;
        double* o = terms + 3 * (long long)slot;
        term_write(o, role, f);
    }
}

__global__ void k_ct_scatter(unsigned int* ctl, const unsigned int* evs, long long shard_cap, const int* ev_nodes,
                             const double* ev_f, const int* toff, const int* tpos, int* cnt, double* terms) {
    scatter_body(blockIdx.x, gridDim.x, ctl, evs, shard_cap, ev_nodes, ev_f, toff, tpos, cnt, terms);
}

// external_force = 0.0 + (sum of the node's terms), summed in double-double and rounded once
__device__ __forceinline__ void sum_body(int bid, int nb, const unsigned int* ctl, int tsel, const int* touched,
                                         const int* toff, const int* tcnt, const double* terms, double* fext,
                                         const int* g2l = nullptr) {
#pragma clang fp contract(off)
    const int nt = (int)ld_ctl(&ctl[kTouched + tsel]);
    for (int q = bid * blockDim.x + threadIdx.x; q < nt; q += nb * blockDim.x) {
        const long long n = g2l ? g2l[touched[q]] : touched[q];
        const int a = toff[q], b = a + tcnt[q];
        for (int c = 0; c < 3; ++c) {
            double s = 0.0, e = 0.0;
            for (int i = a; i < b; ++i) {
                const double x = terms[3 * (long long)i + c];
                const double t = s + x;  // TwoSum
                const double bp = t - s;
                const double err = (s - (t - bp)) + (x - bp);
                s = t;
                e += err;
            }
            fext[3 * n + c] = s + e;
        }
    }
}

__global__ void k_ct_sum(unsigned int* ctl, int tsel, const int* touched, const int* toff, const int* tcnt,
                         const double* terms, double* fext, const int* g2l) {
    sum_body(blockIdx.x, gridDim.x, ctl, tsel, touched, toff, tcnt, terms, fext, g2l);
    // multi-GPU: the next step's touched list starts empty (its steps run no k_ct_reset)
    if (g2l && blockIdx.x == 0 && threadIdx.x == 0) ctl[kTouched + 1 - tsel] = 0;
}

// ---- small decks: fused single-workgroup phases ------------------------------------------------
// The reference's own decks have a few thousand contact entries and tens of events per step, so
// the ~13 launches of a contact step (each >= ~2.4 us from a graph, tools/barrier_probe.hip) cost
// more than their work. For models small at setup (Contact::small) the step runs the prologue
// (reset, deletion scan, surface append) and the event gather (count, alloc, scatter, sum) each as
// ONE 1024-thread workgroup, the bodies separated by workgroup barriers; the binning and the
// triangle prefilter share one launch. Same bodies, same results.
constexpr int kSmallThreads = 1024;

__global__ __launch_bounds__(kSmallThreads) void k_ct_prologue1(
    unsigned long long* bbox, int npairs, unsigned int* ctl, unsigned int* evs, unsigned int* ccnt, const int* del_any,
    int t, const double* t_rd, const int* touched_prev, int tsel, double* fext, const int* del_step, int nE,
    int* dlist, AppendIn A, int* reg, int* ni_live, int* nj_live, int* tri_live, int with_lists) {
    reset_body(0, 1, bbox, npairs, ctl, evs, ccnt, 0, del_any, t, t_rd, touched_prev, tsel, fext);
    if (!with_lists) return;
    __syncthreads();
    find_del_body(0, 1, ctl, del_step, nE, t, t_rd, dlist);
    __syncthreads();
    append_body(0, 1, ctl, dlist, A, del_step, t, t_rd, reg, ni_live, nj_live, tri_live, (int)threadIdx.x,
                (int)blockDim.x);
}

__global__ __launch_bounds__(kSmallThreads) void k_ct_gather1(unsigned int* ctl, const unsigned int* evs,
                                                              long long shard_cap, const int* ev_nodes,
                                                              const double* ev_f, int* cnt, int* touched, int* tpos,
                                                              int tsel, int* poison, int t,
                                                              const double* t_rd, int* toff, int* tcnt,
                                                              double* terms, double* fext) {
    count_body(0, 1, ctl, evs, shard_cap, ev_nodes, cnt, touched, tpos, tsel, poison, t, t_rd);
    __syncthreads();
    alloc_body(0, 1, ctl, tsel, touched, cnt, toff, tcnt);
    __syncthreads();
    scatter_body(0, 1, ctl, evs, shard_cap, ev_nodes, ev_f, toff, tpos, cnt, terms);
    __syncthreads();
    sum_body(0, 1, ctl, tsel, touched, toff, tcnt, terms, fext);
}

// binning (workgroups [0, nbin)) and the triangle prefilter (the rest) in one launch: both need
// only the pair boxes
__global__ __launch_bounds__(kB) void k_ct_binfilter(StepIn s, const Seg* segs, const int* reg, const int* ni_live,
                                                     const int* ni_pair, const int* ni_node, const PairParam* par,
                                                     const unsigned long long* bbox, const unsigned int* ctl,
                                                     unsigned long long* head, BEnt* blist, BVel* bvel,
                                                     int sb, int nbin, const int* tri_cnt,
                                                     const int* tri_live, const int* tri_pair, const int* tri_nodes,
                                                     const int* tri_ele, unsigned int* ccnt, TriRec* cand,
                                                     long long cshard_cap, uint2* item) {
    if ((int)blockIdx.x < nbin)
        bin_body(blockIdx.x, s, segs, reg, ni_live, ni_pair, ni_node, par, bbox, ctl, head, blist, bvel, sb);
    else
        tri_filter_body(blockIdx.x - nbin, gridDim.x - nbin, s, tri_cnt, tri_live, tri_pair, tri_nodes, tri_ele, par,
                        bbox, ccnt, cand, cshard_cap, item);
}

}  // namespace

namespace hkc {

void contact_destroy(hakai_ctx* c) {
    Contact* C = c->contact;
    if (!C) return;
    (void)hipStreamSynchronize(c->stream);
    if (C->xr) xr_destroy(C);
    delete C;  // every buffer frees itself
    c->contact = nullptr;
    c->d_fext = nullptr;
}

int contact_state_reset(hakai_ctx* c, const double* velo0_host) {
    Contact* C = c->contact;
    if (!C) return 0;
    C->use_velo0 = true;
    C->force_rebuild = true;
    if (velo0_host)
        HIPCHK(hipMemcpyAsync(C->d_velo0, velo0_host, 3 * (size_t)c->nN * sizeof(double), hipMemcpyHostToDevice,
                              c->stream));
    return C->xr ? xr_state_reset(c) : 0;
}

static int search(hakai_ctx* c, const StepIn& in, bool fused);

// prefilter grid: one live triangle per thread
unsigned filter_grid(const Contact* C) {
    return (unsigned)std::max(1, std::min((C->n_tri + kB - 1) / kB, kFilterBlocks));
}

// the triangle prefilter against the (combined) pair boxes bbox, as its own launch
void tri_prefilter(hakai_ctx* c, const StepIn& in, const unsigned long long* bbox) {
    Contact* C = c->contact;
    hipLaunchKernelGGL(k_ct_tri_filter, dim3(filter_grid(C)), dim3(kB), 0, c->stream, in, C->d_reg + 2 * C->tri_reg + 1,
                       C->d_tri_live, C->d_tri_pair, C->d_tri_nodes, C->d_tri_ele, C->d_par, bbox, C->d_ccnt,
                       C->d_cand, C->cshard_cap, C->small ? nullptr : C->d_item);
}

// the step's input arrays of one GPU (multi-GPU: the exchange file replaces mass, l2g, del_step)
StepIn step_in(hakai_ctx* c, double t, double d_time) {
    Contact* C = c->contact;
    StepIn in;
    in.coord = c->d_coord;
    in.u = c->d_u[c->sv.cur];
    in.u_pre = c->d_u[1 - c->sv.cur];
    in.flag = c->d_flag;
    in.conn = c->d_conn;
    in.mass = c->d_mass;
    in.l2g = nullptr;
    in.del_step = c->d_del_step;
    in.velo0 = C->use_velo0 ? C->d_velo0 : nullptr;
    in.d_time = d_time;
    in.t = (int)t;
    return in;
}

static AppendIn append_in(const Contact* C) {
    AppendIn A;
    A.el_tri_ptr = C->d_el_tri_ptr; A.el_tri = C->d_el_tri;
    A.el_ni_ptr = C->d_el_ni_ptr; A.el_ni = C->d_el_ni; A.el_nj_ptr = C->d_el_nj_ptr; A.el_nj = C->d_el_nj;
    A.ni_orig = C->d_ni_orig; A.ni_aptr = C->d_ni_aptr; A.ni_add = C->d_ni_add; A.ni_pair = C->d_ni_pair;
    A.nj_orig = C->d_nj_orig; A.nj_aptr = C->d_nj_aptr; A.nj_add = C->d_nj_add; A.nj_pair = C->d_nj_pair;
    A.pair_reg = C->d_pair_reg;
    A.tri_reg = C->tri_reg;
    return A;
}

static LiveIn live_in(const hakai_ctx* c, const int* del_step, int t) {
    const Contact* C = c->contact;
    LiveIn L;
    L.ni_orig = C->d_ni_orig; L.ni_aptr = C->d_ni_aptr; L.ni_add = C->d_ni_add;
    L.nj_orig = C->d_nj_orig; L.nj_aptr = C->d_nj_aptr; L.nj_add = C->d_nj_add;
    L.tri_ele = C->d_tri_ele; L.tri_adder = C->d_tri_adder;
    L.flag = c->d_flag; L.del_step = del_step; L.t = t;
    return L;
}

bool step_begin(Contact* C, int t) {
    if ((long long)t != C->last_t + 1 || C->always_rebuild) C->force_rebuild = true;
    const bool rebuild = C->force_rebuild;
    C->tsel = 1 - C->tsel;
    C->force_rebuild = false;
    C->last_t = t;
    return rebuild;
}

void launch_reset(hakai_ctx* c, unsigned long long* bbox, bool rebuild, const int* del_any, int t, const int* g2l,
                  int* zero_hdr) {
    Contact* C = c->contact;
    hipLaunchKernelGGL(k_ct_reset, dim3(C->g_reset), dim3(kB), 0, c->stream, bbox, C->npairs, C->d_ctl, C->d_evs,
                       C->d_ccnt, rebuild ? 1 : 0, del_any, t, c->gr.trd, C->d_touched[1 - C->tsel], C->tsel, c->d_fext,
                       g2l, zero_hdr);
}

// full rebuild (forced steps only: the host knows them, so the kernels are not even launched
// otherwise)
void live_rebuild(hakai_ctx* c, const int* del_step, int t) {
    Contact* C = c->contact;
    if (C->ntile == 0) return;
    hipStream_t s = c->stream;
    const LiveIn L = live_in(c, del_step, t);
    const Tile* tl = C->d_tiles;
    const unsigned gt = (unsigned)std::min(C->ntile, 2048);
    hipLaunchKernelGGL(k_ct_live_count, dim3(gt), dim3(kB), 0, s, C->d_ctl, L, tl, C->ntile, C->d_tile_cnt);
    hipLaunchKernelGGL(k_ct_live_scan, dim3(1), dim3(kB), 0, s, C->d_ctl, C->ntile, C->d_tile_cnt, C->d_tile_off,
                       C->nreg, C->d_reg_first, C->d_reg);
    hipLaunchKernelGGL(k_ct_live_write, dim3(gt), dim3(kB), 0, s, C->d_ctl, L, tl, C->ntile, C->d_tile_off,
                       C->d_reg_first, C->d_reg, C->d_ni_live, C->d_nj_live, C->d_tri_live);
}

// incremental update (steps after a deletion): the entries the listed deletions expose
void live_append(hakai_ctx* c, const int* del_step, int t) {
    Contact* C = c->contact;
    if (C->ntile == 0) return;
    hipLaunchKernelGGL(k_ct_append, dim3(256), dim3(64), 0, c->stream, C->d_ctl, C->d_dlist, append_in(C), del_step, t,
                       c->gr.trd, C->d_reg, C->d_ni_live, C->d_nj_live, C->d_tri_live);
}

void launch_boxes(hakai_ctx* c, const StepIn& in, unsigned long long* bbox) {
    Contact* C = c->contact;
    if (C->nseg > 0)
        hipLaunchKernelGGL(k_ct_bbox, dim3(C->nseg * C->g_box), dim3(kB), 0, c->stream, in, C->d_seg, C->d_reg,
                           C->d_ni_live, C->d_nj_live, C->d_ni_node, C->d_nj_node, bbox, C->g_box);
}

void launch_alloc(hakai_ctx* c) {
    Contact* C = c->contact;
    hipLaunchKernelGGL(k_ct_alloc, dim3(C->g_node), dim3(kB), 0, c->stream, C->d_ctl, C->tsel, C->d_touched[C->tsel],
                       C->d_cnt, C->d_toff, C->d_tcnt);
}

void launch_sum(hakai_ctx* c, const int* g2l) {
    Contact* C = c->contact;
    hipLaunchKernelGGL(k_ct_sum, dim3(C->g_node), dim3(kB), 0, c->stream, C->d_ctl, C->tsel, C->d_touched[C->tsel],
                       C->d_toff, C->d_tcnt, C->d_terms, c->d_fext, g2l);
}

// One GPU: a step's whole contact work (:500-560): step prologue, live-list update, pair boxes,
// then the search and the event gather into external_force.
static int step_start(hakai_ctx* c, double t, double d_time) {
    Contact* C = c->contact;
    hipStream_t s = c->stream;
    const StepIn in = step_in(c, t, d_time);
    const int* del_step = c->d_del_step;
    const int* del_any = c->d_del_step + c->nEp + 1;
    const bool rebuild = step_begin(C, in.t);
    // small decks: reset + deletion scan + surface append in one workgroup (not on full-rebuild
    // steps, whose live-list rebuild sits between the reset and the scan)
    const bool fused = C->small && C->fuse_small;
    if (fused && !rebuild) {
        hipLaunchKernelGGL(k_ct_prologue1, dim3(1), dim3(kSmallThreads), 0, s, C->d_bbox, C->npairs, C->d_ctl, C->d_evs,
                           C->d_ccnt, del_any, in.t, c->gr.trd, C->d_touched[1 - C->tsel], C->tsel, c->d_fext, del_step,
                           (int)C->nE, C->d_dlist, append_in(C), C->d_reg, C->d_ni_live, C->d_nj_live, C->d_tri_live,
                           C->ntile > 0 ? 1 : 0);
    } else {
        launch_reset(c, C->d_bbox, rebuild, del_any, in.t, nullptr, nullptr);
        if (rebuild) live_rebuild(c, del_step, in.t);
        if (C->ntile > 0)
            hipLaunchKernelGGL(k_ct_find_del, dim3(C->g_del), dim3(kB), 0, s, C->d_ctl, del_step, (int)C->nE, in.t,
                               c->gr.trd, C->d_dlist);
        live_append(c, del_step, in.t);
    }
    launch_boxes(c, in, C->d_bbox);
    HIPCHK(hipGetLastError());
    return search(c, in, fused);
}

// binning, bucket scan and fill, triangle prefilter and search, and (one GPU) the event gather
// into external_force
static int search(hakai_ctx* c, const StepIn& in, bool fused) {
    Contact* C = c->contact;
    hipStream_t s = c->stream;
    const int tsel = C->tsel;
    const unsigned gfilt = filter_grid(C);
    // the binning and the triangle prefilter in one launch (both need only the boxes; their
    // workgroups run side by side): small decks, and larger ones unless tuned off
    const bool fused_mid = (fused || C->fuse_binfilter) && C->nseg > 0 && C->n_tri > 0;
    const Seg* sg = C->d_seg;
    if (C->nseg > 0) {
        if (fused_mid) {
            const int nbin = C->nseg * C->g_seg;
            hipLaunchKernelGGL(k_ct_binfilter, dim3((unsigned)nbin + gfilt), dim3(kB), 0, s, in, sg, C->d_reg,
                               C->d_ni_live, C->d_ni_pair, C->d_ni_node, C->d_par, C->d_bbox, C->d_ctl, C->d_head,
                               C->d_blist, C->d_bvel, C->g_seg, nbin, C->d_reg + 2 * C->tri_reg + 1, C->d_tri_live,
                               C->d_tri_pair, C->d_tri_nodes, C->d_tri_ele, C->d_ccnt, C->d_cand,
                               C->cshard_cap, C->small ? nullptr : C->d_item);
        } else {
            hipLaunchKernelGGL(k_ct_bin, dim3(C->nseg * C->g_seg), dim3(kB), 0, s, in, sg, C->d_reg, C->d_ni_live,
                               C->d_ni_pair, C->d_ni_node, C->d_par, C->d_bbox, C->d_ctl, C->d_head, C->d_blist,
                               C->d_bvel, C->g_seg);
        }
    }
    if (C->n_tri > 0) {
        if (!fused_mid) tri_prefilter(c, in, C->d_bbox);
        tri_search(c, in);
    }
    const unsigned ge = (unsigned)C->g_ev;
    if (fused) {  // small decks: count, alloc, scatter and sum in one workgroup
        hipLaunchKernelGGL(k_ct_gather1, dim3(1), dim3(kSmallThreads), 0, s, C->d_ctl, C->d_evs, C->cap / kEvShards,
                           C->d_ev_nodes, C->d_ev_f, C->d_cnt, C->d_touched[tsel], C->d_tpos, tsel, c->d_poison,
                           in.t, c->gr.trd, C->d_toff, C->d_tcnt, C->d_terms, c->d_fext);
        HIPCHK(hipGetLastError());
        C->use_velo0 = false;
        return 0;
    }
    hipLaunchKernelGGL(k_ct_count, dim3(ge), dim3(kB), 0, s, C->d_ctl, C->d_evs, C->cap / kEvShards, C->d_ev_nodes,
                       C->d_cnt, C->d_touched[tsel], C->d_tpos, tsel, c->d_poison, in.t, c->gr.trd);
    launch_alloc(c);
    hipLaunchKernelGGL(k_ct_scatter, dim3(ge), dim3(kB), 0, s, C->d_ctl, C->d_evs, C->cap / kEvShards, C->d_ev_nodes,
                       C->d_ev_f, C->d_toff, C->d_tpos, C->d_cnt, C->d_terms);
    launch_sum(c, nullptr);
    HIPCHK(hipGetLastError());
    C->use_velo0 = false;
    return 0;
}

void tri_search(hakai_ctx* c, const StepIn& in) {
    Contact* C = c->contact;
    if (C->small) {
        hipLaunchKernelGGL(k_ct_tri32, dim3(C->g_tri), dim3(128), 0, c->stream, in, C->d_ctl, C->d_ccnt,
                           C->d_cand, C->cshard_cap, C->d_par, C->d_head, C->d_blist, C->d_bvel,
                           C->d_lim, C->myu, C->d_evs, C->cap / kEvShards, C->d_ev_nodes, C->d_ev_f);
        return;
    }
    hipLaunchKernelGGL(k_ct_tri, dim3(C->g_tri), dim3(128), 0, c->stream, in, C->d_ctl, C->d_ccnt,
                       C->d_cand, C->cshard_cap, C->d_item, C->d_par, C->d_head, C->d_blist, C->d_bvel, C->d_lim,
                       C->myu, C->d_evs, C->cap / kEvShards, C->d_ev_nodes, C->d_ev_f);
}

int contact_phase(hakai_ctx* c, int part, double t, double d_time) {
    Contact* C = c->contact;
    if (!C) return 0;
    if (part == 1) return C->xr ? xr_a1(c, t, d_time) : step_start(c, t, d_time);
    if (!C->xr) return 0;
    return part == 2 ? xr_a2(c, d_time) : xr_a3(c, d_time);
}

int contact_step(hakai_ctx* c, double t, double d_time) {
    if (c->contact && c->contact->xr)
        return fail(HAKAI_ERR_STATE, "contact force probe on a multi-GPU rank: step the group instead");
    return contact_phase(c, 1, t, d_time);
}

bool contact_multi(const hakai_ctx* c) { return c->contact && c->contact->xr; }

// Graph mode (hakai_step): a step may be captured when its contact work is the same launch sequence
// every step -- one GPU, no full rebuild, no initial velocity, consecutive step numbers.
// contact_step's host state then changes only by the tsel flip and last_t, which
// contact_graph_advance replays for a cached graph's two steps.
bool contact_graph_ok(const hakai_ctx* c, double t) {
    const Contact* C = c->contact;
    if (!C) return true;
    return !C->xr && !C->force_rebuild && !C->always_rebuild && !C->use_velo0 && (long long)t == C->last_t + 1;
}

// hakai_step found a poisoned step: the device state is the last good step's. Rebuild the live
// lists at the next step; velo of the first step is the initial one only if no step survived.
// Multi-GPU: if an exchange capacity overflowed (the same on every rank: they read the same
// headers), grow it past every count of the failed step and pack every deletion step again, so the
// step can run again from there (contact_exchange_retry).
void contact_after_overflow(hakai_ctx* c, long long steps_since_reset) {
    Contact* C = c->contact;
    if (!C) return;
    C->force_rebuild = true;
    C->use_velo0 = steps_since_reset == 0;
    C->last_t = -1;
    if (C->xr) xr_after_overflow(c);
}

void contact_graph_advance(hakai_ctx* c, double t_last) {
    Contact* C = c->contact;
    if (!C) return;
    C->last_t = (long long)t_last;  // two steps: tsel flipped twice
}

// candidate buffer of about `total` records in kCandShards shards. A shard holds at least what
// its prefilter blocks can append in one pass over the triangles (kB per block), so a deck whose
// triangles fit one pass of the grid cannot overflow a shard -- as the unsharded n_tri-sized
// buffer could not.
static void size_cand(Contact* C, long long total) {
    const long long blocks = std::max<long long>(1, std::min<long long>((C->n_tri + kB - 1) / kB, kFilterBlocks));
    const long long one_pass = (blocks + kCandShards - 1) / kCandShards * kB;
    C->cshard_cap = std::max<long long>((total + kCandShards - 1) / kCandShards, one_pass);
    C->cand_cap = C->cshard_cap * kCandShards;
}

int contact_tuning(hakai_ctx* c, const char* key, long long value) {
    Contact* C = c->contact;
    if (!C) return fail(HAKAI_ERR_STATE, "%s before set_contact", key);
    if (!std::strcmp(key, "contact_fuse_binfilter")) {
        if (value != 0 && value != 1) return fail(HAKAI_ERR_ARG, "contact_fuse_binfilter must be 0 or 1");
        C->fuse_binfilter = (int)value;
        graph_invalidate(c);
        return 0;
    }
    if (!std::strcmp(key, "contact_fuse_small")) {  // small decks: fused single-workgroup phases
        if (value != 0 && value != 1) return fail(HAKAI_ERR_ARG, "contact_fuse_small must be 0 or 1");
        C->fuse_small = (int)value;
        graph_invalidate(c);
        return 0;
    }
    if (!std::strcmp(key, "contact_candidate_cap")) {
        if (value < 1 || value > (1LL << 31) - 1) return fail(HAKAI_ERR_ARG, "contact_candidate_cap out of range");
        HIPCHK(hipStreamSynchronize(c->stream));
        C->d_cand.free();
        C->d_item.free();
        size_cand(C, value);
        HIPCHK(C->d_cand.alloc((size_t)C->cand_cap));
        HIPCHK(C->d_item.alloc((size_t)kItemsPerCand * C->cand_cap));
        HIPCHK(hipMemsetAsync(C->d_ctl + kNcandMax, 0, 3 * sizeof(unsigned int), c->stream));  // + shard max, over
        HIPCHK(hipMemsetAsync(C->d_ctl + kItemShardMax, 0, sizeof(unsigned int), c->stream));
        return 0;
    }
    if (!std::strcmp(key, "contact_exchange_deletions") || !std::strcmp(key, "contact_exchange_bins") ||
        !std::strcmp(key, "contact_exchange_events")) {
        if (!C->xr) return fail(HAKAI_ERR_STATE, "%s without hakai_set_contact_global", key);
        return xr_tuning(c, key, value);
    }
    if (!std::strcmp(key, "contact_full_rebuild")) {
        if (value != 0 && value != 1) return fail(HAKAI_ERR_ARG, "contact_full_rebuild must be 0 or 1");
        C->always_rebuild = value != 0;
        return 0;
    }
    if (!std::strcmp(key, "contact_event_cap")) {
        if (value < 1 || value > (1LL << 30)) return fail(HAKAI_ERR_ARG, "contact_event_cap out of range");
        HIPCHK(hipStreamSynchronize(c->stream));
        C->d_ev_nodes.free();
        C->d_ev_f.free();
        C->d_terms.free();
        C->d_touched[0].free();
        C->d_touched[1].free();
        C->d_toff.free();
        C->d_tcnt.free();
        C->cap = (value + kEvShards - 1) / kEvShards * kEvShards;
        C->tcap = std::min<long long>(C->nN, 4 * C->cap);
        if (C->xr) xr_event_cap(C);
        HIPCHK(C->d_ev_nodes.alloc(4 * (size_t)C->cap));
        HIPCHK(C->d_ev_f.alloc(3 * (size_t)C->cap));
        HIPCHK(C->d_terms.alloc(12 * (size_t)C->cap));
        HIPCHK(C->d_touched[0].alloc((size_t)C->tcap));
        HIPCHK(C->d_touched[1].alloc((size_t)C->tcap));
        HIPCHK(C->d_toff.alloc((size_t)C->tcap));
        HIPCHK(C->d_tcnt.alloc((size_t)C->tcap));
        // the previous step's touched list is gone: clear external_force and its count
        HIPCHK(hipMemsetAsync(c->d_fext, 0, 3 * (size_t)c->nN * sizeof(double), c->stream));
        HIPCHK(hipMemsetAsync(C->d_ctl + kTouched, 0, 2 * sizeof(unsigned int), c->stream));
        HIPCHK(hipMemsetAsync(C->d_ctl + kEvMax, 0, sizeof(unsigned int), c->stream));
        HIPCHK(hipMemsetAsync(C->d_ctl + kEvShardMax, 0, sizeof(unsigned int), c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return 0;
    }
    return fail(HAKAI_ERR_ARG, "unknown tuning key '%s'", key);
}

int contact_check(hakai_ctx* c) {
    Contact* C = c->contact;
    if (!C) return 0;
    unsigned int mx = 0, mc[3] = {0, 0, 0};
    HIPCHK(hipMemcpyAsync(&mx, C->d_ctl + kEvMax, sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(mc, C->d_ctl + kNcandMax, 3 * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if ((long long)mc[kCandShardMax - kNcandMax] > C->cshard_cap)
        return fail(HAKAI_ERR_STATE, "contact: %u candidate triangles in one step (%u in one of %d shards) exceed the "
                    "buffer (%lld); raise hakai_set_tuning(\"contact_candidate_cap\")", mc[0],
                    mc[kCandShardMax - kNcandMax], kCandShards, C->cand_cap);
    unsigned int mi = 0;  // search items (one per candidate and reachable cell, <= 27 per candidate)
    HIPCHK(hipMemcpy(&mi, C->d_ctl + kItemShardMax, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if ((long long)mi > kItemsPerCand * C->cshard_cap)
        return fail(HAKAI_ERR_STATE, "contact: %u search items in one of %d shards exceed the item buffer (%lld per "
                    "shard, %d per candidate slot); raise hakai_set_tuning(\"contact_candidate_cap\"), which also "
                    "grows the item buffer", mi, kCandShards, (long long)kItemsPerCand * C->cshard_cap, kItemsPerCand);
    if (C->xr)
        if (int rc = xr_check(c)) return rc;
    unsigned int ms = 0;
    HIPCHK(hipMemcpy(&ms, C->d_ctl + kEvShardMax, sizeof(unsigned int), hipMemcpyDeviceToHost));
    if ((long long)ms > C->cap / kEvShards)
        return fail(HAKAI_ERR_STATE, "contact: %u events in one step (%u in one of %d shards) exceed the buffer "
                    "(%lld); raise hakai_set_tuning(\"contact_event_cap\")", mx, ms, kEvShards, C->cap);
    int pz = 0;
    HIPCHK(hipMemcpy(&pz, c->d_poison, sizeof(int), hipMemcpyDeviceToHost));
    if (pz)  // multi-GPU search: another rank's buffers overflowed
        return fail(HAKAI_ERR_STATE, "contact: a contact buffer of another rank overflowed; raise "
                    "hakai_set_tuning(\"contact_event_cap\" / \"contact_candidate_cap\") on every rank");
    return 0;
}

// what depends on the kernels' constants: buffer capacities and launch grids (see Contact::g_*)
static void size_for_kernels(Contact* C, const hkc::ContactPlan& P) {
    long long ci0 = 0, ct0 = 0, maxseg = 1;  // initial contact points and live triangles, longest segment
    for (int p = 0; p < C->npairs; ++p) {
        ci0 += C->pair_counts[3 * p];
        ct0 += C->pair_counts[3 * p + 1];
    }
    for (const Seg& sg : P.seg) maxseg = std::max<long long>(maxseg, sg.end - sg.start);
    // fused small-deck phases: one 1024-thread workgroup scans the deletion steps, the bucket table
    // and the i-node entries a few times at most
    C->small = C->nE <= (1 << 16) && C->n_ni <= (1 << 16) && C->htot <= (1 << 15);
    // event buffer: 8 events per initial contact point (overflow is detected and reported)
    C->cap = std::max<long long>(1 << 16, 8LL * ci0);
    C->cap = (C->cap + kEvShards - 1) / kEvShards * kEvShards;
    C->tcap = std::min<long long>(C->nN, 4 * C->cap);
    size_cand(C, std::min<long long>(std::max<long long>(C->n_tri, 1), std::max<long long>(1 << 16, 4 * ct0)));
    // launch grids: large models keep the full grids
    auto clampi = [](long long v, long long lo, long long hi) { return (int)std::max(lo, std::min(hi, v)); };
    C->g_seg = clampi((maxseg + kB - 1) / kB, 1, kSegBlocks);
    C->g_box = clampi((maxseg + 4 * kB - 1) / (4 * kB), 1, 128);  // ~4 entries per thread: one unrolled pass
    C->g_ev = clampi((4 * ci0 + kB - 1) / kB, 16, 1024);
    // >= 64 waves (every event shard); one pass over 16 search items (reachable cells) per live
    // triangle up to the 4096-block cap -- small self-contact decks keep half their triangles
    C->g_tri = clampi(((C->small ? 32 : 16) * ct0 + 127) / 128, 32, 4096);  // (small: 32 lanes per candidate)
    C->g_node = clampi((2 * ci0 + kB - 1) / kB, 4, 256);
    C->g_del = clampi((C->nE / 4 + kB - 1) / kB, 1, 1024);
    C->g_reset =
        clampi((std::max<long long>(std::max<long long>(kEvShards, 12LL * C->npairs), 2 * ci0) + kB - 1) / kB, 1, 64);
}

// builds c->contact on the mesh of `in` (the context's own, or the global one with the entries this
// rank keeps): plan (hakai_contact_plan.hpp), sizes, upload, buffers; c->contact was destroyed by the caller
int contact_setup(hakai_ctx* c, const hkc::ContactInput& in, hkc::ContactPlan& P) {
    if (in.nE == 0) return 0;
    const std::string err = hkc::contact_plan(in, P);
    if (!err.empty()) return fail(HAKAI_ERR_ARG, "%s", err.c_str());
    auto* C = new hkc::Contact();
    C->kc_o = in.kc_o, C->kc_s = in.kc_s, C->Cr_o = in.Cr_o, C->Cr_s = in.Cr_s;  // what the plan's pairs hold
    C->nN = in.nN, C->nE = in.nE, C->npairs = (int)P.par.size(), C->h_par = P.par, C->htot = P.htot;
    C->n_ni = (int)P.ni.node.size(), C->n_nj = (int)P.nj.node.size(), C->n_tri = (int)P.tri_ele.size();
    C->nseg = (int)P.seg.size(), C->ntile = (int)P.tiles.size(), C->nreg = (int)P.reg_list.size();
    C->tri_reg = P.tri_reg, C->reg_list_h = P.reg_list, C->pair_inst = P.pair_inst, C->pair_counts = P.pair_counts;
    C->min_size = P.min_size, C->max_size = P.max_size, C->d_lim = P.d_lim;
    size_for_kernels(C, P);
    hipStream_t s = c->stream;
    const hipError_t ups[] = {
        C->d_par.upload(P.par, s), C->d_seg.upload(P.seg, s),
        C->d_ni_pair.upload(P.ni.pair, s), C->d_ni_node.upload(P.ni.node, s), C->d_ni_orig.upload(P.ni.orig, s),
        C->d_ni_aptr.upload(P.ni.aptr, s), C->d_ni_add.upload(P.ni.add, s),
        C->d_nj_pair.upload(P.nj.pair, s), C->d_nj_node.upload(P.nj.node, s), C->d_nj_orig.upload(P.nj.orig, s),
        C->d_nj_aptr.upload(P.nj.aptr, s), C->d_nj_add.upload(P.nj.add, s),
        C->d_tri_pair.upload(P.tri_pair, s), C->d_tri_nodes.upload(P.tri_nodes, s),
        C->d_tri_ele.upload(P.tri_ele, s), C->d_tri_adder.upload(P.tri_adder, s),
        C->d_reg_first.upload(P.reg_first, s), C->d_reg.upload(P.reg, s), C->d_pair_reg.upload(P.pair_reg, s),
        C->d_el_ni_ptr.upload(P.el_ni_ptr, s), C->d_el_ni.upload(P.el_ni, s),
        C->d_el_nj_ptr.upload(P.el_nj_ptr, s), C->d_el_nj.upload(P.el_nj, s),
        C->d_el_tri_ptr.upload(P.el_tri_ptr, s), C->d_el_tri.upload(P.el_tri, s), C->d_tiles.upload(P.tiles, s)};
    int rc = 0;
    for (hipError_t e : ups)
        if (e != hipSuccess) rc = hip_fail(e, "contact_setup: upload");
    c->contact = C;
    if (rc) {
        hkc::contact_destroy(c);
        return rc;
    }
    HIPCHK(C->d_head.alloc((size_t)C->htot));
    HIPCHK(hipMemsetAsync(C->d_head, 0, (size_t)C->htot * sizeof(unsigned long long), s));  // stamp 0: empty
    C->blist_cap = std::max(C->n_ni, 1);  // (multi-GPU: sized for every rank's records, xr_buffers)
    HIPCHK(C->d_blist.alloc((size_t)C->blist_cap));
    HIPCHK(C->d_bvel.alloc((size_t)C->blist_cap));
    HIPCHK(C->d_tile_cnt.alloc((size_t)C->ntile));
    HIPCHK(C->d_tile_off.alloc((size_t)C->ntile + 1));
    HIPCHK(C->d_dlist.alloc((size_t)C->nE));
    HIPCHK(C->d_ni_live.alloc((size_t)C->n_ni));
    HIPCHK(C->d_nj_live.alloc((size_t)C->n_nj));
    HIPCHK(C->d_tri_live.alloc((size_t)C->n_tri));
    HIPCHK(C->d_bbox.alloc((size_t)box_words(C->npairs)));
    HIPCHK(C->d_ctl.alloc((size_t)kCtl));
    HIPCHK(C->d_evs.alloc((size_t)kEvShards * kShardStride));
    HIPCHK(hipMemsetAsync(C->d_evs, 0, (size_t)kEvShards * kShardStride * sizeof(unsigned int), s));
    HIPCHK(C->d_ev_nodes.alloc(4 * (size_t)C->cap));
    HIPCHK(C->d_ev_f.alloc(3 * (size_t)C->cap));
    HIPCHK(C->d_cnt.alloc((size_t)C->nN + 1));
    HIPCHK(C->d_tpos.alloc((size_t)C->nN + 1));
    HIPCHK(C->d_touched[0].alloc((size_t)C->tcap));
    HIPCHK(C->d_touched[1].alloc((size_t)C->tcap));
    HIPCHK(C->d_toff.alloc((size_t)C->tcap));
    HIPCHK(C->d_tcnt.alloc((size_t)C->tcap));
    HIPCHK(C->d_ccnt.alloc((size_t)kCandShards * kShardStride));
    HIPCHK(C->d_cand.alloc((size_t)C->cand_cap));
    HIPCHK(C->d_item.alloc((size_t)kItemsPerCand * C->cand_cap));
    if (C->htot >= (1 << 27)) return fail(HAKAI_ERR_ARG, "contact: %d hash buckets (search items hold 27 bits)", C->htot);
    HIPCHK(C->d_terms.alloc(12 * (size_t)C->cap));
    HIPCHK(C->d_velo0.alloc(3 * (size_t)c->nN));
    HIPCHK(C->d_fext.alloc(3 * (size_t)c->nN));
    c->d_fext = C->d_fext;
    HIPCHK(hipMemsetAsync(C->d_cnt, 0, ((size_t)C->nN + 1) * sizeof(int), s));
    HIPCHK(hipMemsetAsync(C->d_ctl, 0, kCtl * sizeof(unsigned int), s));
    HIPCHK(hipMemsetAsync(c->d_fext, 0, 3 * (size_t)c->nN * sizeof(double), s));
    C->force_rebuild = true;
    // velocity before the first step: the state's (IC / uploaded) velocity (local nodes)
    if (!c->h_velo0.empty())
        HIPCHK(hipMemcpyAsync(C->d_velo0, c->h_velo0.data(), 3 * (size_t)c->nN * sizeof(double), hipMemcpyHostToDevice, s));
    else
        HIPCHK(hipMemsetAsync(C->d_velo0, 0, 3 * (size_t)c->nN * sizeof(double), s));
    C->use_velo0 = c->sv.steps_done == 0 || !c->h_velo0.empty();
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // namespace hkc

extern "C" {

int hakai_set_contact(hakai_ctx* c, int32_t contact_flag, const int64_t* element_instance) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    return hakai_set_contact_cp(c, contact_flag, element_instance, 0, nullptr, nullptr, nullptr);
}

int hakai_set_contact_cp(hakai_ctx* c, int32_t contact_flag, const int64_t* element_instance, int32_t n_cp,
                         const int32_t* cp_instance, const int64_t* cp_elem_off, const int64_t* cp_elems) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (n_cp < 0 || (n_cp > 0 && (!cp_instance || !cp_elem_off || !cp_elems)))
        return fail(HAKAI_ERR_ARG, "set_contact_cp: bad contact-pair arrays");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "set_contact before upload_model");
    HIPCHK(hipSetDevice(c->device));
    hkc::contact_destroy(c);
    if (contact_flag < 1) return 0;
    if (contact_flag > 2) return fail(HAKAI_ERR_ARG, "contact_flag %d (0, 1 or 2)", contact_flag);
    if (c->comm)
        return fail(HAKAI_ERR_STATE, "contact on a rank of a multi-GPU group: use hakai_set_contact_global");
    hkc::ContactInput in;
    in.nN = c->nN, in.nE = c->nE, in.coord = &c->h_coord, in.conn = &c->h_conn, in.mat = &c->h_mat;
    in.young = &c->h_young, in.contact_flag = contact_flag, in.element_instance = element_instance;
    in.n_cp = n_cp, in.cp_instance = cp_instance, in.cp_elem_off = cp_elem_off, in.cp_elems = cp_elems;
    hkc::ContactPlan plan;
    return hkc::contact_setup(c, in, plan);
}

int hakai_set_contact_params(hakai_ctx* c, double myu, double kc_o, double kc_s, double Cr_o, double Cr_s) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    hkc::Contact* C = c->contact;
    if (!C) return fail(HAKAI_ERR_STATE, "set_contact_params before set_contact");
    C->myu = myu;
    C->kc_o = kc_o;
    C->kc_s = kc_s;
    C->Cr_o = Cr_o;
    C->Cr_s = Cr_s;
    for (auto& p : C->h_par) {
        p.kc = p.self ? kc_s : kc_o;
        p.Cr = p.self ? Cr_s : Cr_o;
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(C->d_par, C->h_par.data(), C->h_par.size() * sizeof(PairParam), hipMemcpyHostToDevice,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int hakai_contact_info(hakai_ctx* c, int32_t* n_pairs, int64_t* info, int32_t cap, double* sizes) {
    if (!c || !n_pairs) return fail(HAKAI_ERR_ARG, "null");
    hkc::Contact* C = c->contact;
    *n_pairs = C ? C->npairs : 0;
    if (!C) return 0;
    for (int p = 0; p < C->npairs && p < cap; ++p) {
        info[5 * p + 0] = C->pair_inst[2 * p];
        info[5 * p + 1] = C->pair_inst[2 * p + 1];
        info[5 * p + 2] = C->pair_counts[3 * p];
        info[5 * p + 3] = C->pair_counts[3 * p + 1];
        info[5 * p + 4] = C->pair_counts[3 * p + 2];
    }
    if (sizes) {
        sizes[0] = C->min_size;
        sizes[1] = C->max_size;
    }
    return 0;
}

int hakai_contact_stats(hakai_ctx* c, int64_t* stats, int32_t cap) {
    if (!c || (!stats && cap > 0)) return fail(HAKAI_ERR_ARG, "null");
    hkc::Contact* C = c->contact;
    if (!C) return fail(HAKAI_ERR_STATE, "contact_stats before set_contact");
    HIPCHK(hipSetDevice(c->device));
    std::vector<unsigned int> ctl(kCtl);
    std::vector<int> reg(2 * (size_t)C->nreg);
    HIPCHK(hipMemcpyAsync(ctl.data(), C->d_ctl, kCtl * sizeof(unsigned int), hipMemcpyDeviceToHost, c->stream));
    if (C->nreg)
        HIPCHK(hipMemcpyAsync(reg.data(), C->d_reg, reg.size() * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    long long live[3] = {0, 0, 0};
    const int64_t v[7] = {ctl[kEv], ctl[kEvMax], ctl[kNcand], ctl[kTouched + C->tsel], 0, 0, 0};
    for (int r = 0; r < C->nreg; ++r) live[C->reg_list_h[r]] += reg[2 * r + 1];
    for (int k = 0; k < cap && k < 7; ++k) stats[k] = k < 4 ? v[k] : live[k == 4 ? 2 : k - 5];
    long long rec_bytes = 0;
    if (cap > 7) {  // multi-GPU: contact-zone i-nodes all ranks binned in the last step; the bytes this
                    // rank's exchanges receive per step (the other ranks' blocks at their capacities)
                    // and the bytes of the records in them (headers + the last step's gathered counts)
        long long binned = 0, bytes = 0;
        if (C->xr)
            if (int rc = hkc::xr_stats(c, &binned, &bytes, &rec_bytes)) return rc;
        stats[7] = binned;
        if (cap > 8) stats[8] = bytes;
    }
    if (cap > 9) stats[9] = C->htot;  // hash-grid buckets over all pairs
    if (cap > 10) {  // live triangles the prefilter tested in full (those with a non-empty range box)
        std::vector<unsigned int> cc((size_t)kCandShards * kShardStride);
        HIPCHK(hipMemcpy(cc.data(), C->d_ccnt, cc.size() * sizeof(unsigned int), hipMemcpyDeviceToHost));
        long long nt = 0;
        for (int q = 0; q < kCandShards; ++q) nt += cc[(size_t)q * kShardStride + kTestWord];
        stats[10] = nt;
    }
    if (cap > 11) stats[11] = rec_bytes;
    return 0;
}

int hakai_contact_force(hakai_ctx* c, double t, double d_time, double* external_force) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c || !external_force) return fail(HAKAI_ERR_ARG, "null");
    if (!c->contact) return fail(HAKAI_ERR_STATE, "contact_force before set_contact");
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "contact_force before reset/upload_state");
    HIPCHK(hipSetDevice(c->device));
    const bool keep = c->contact->use_velo0;
    c->contact->force_rebuild = true;  // live lists for this t; and again for the next real step
    int rc = hkc::contact_step(c, t, d_time);
    c->contact->use_velo0 = keep;  // a probe, not a step
    c->contact->force_rebuild = true;
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(external_force, c->d_fext, 3 * (size_t)c->nN * sizeof(double), hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipMemsetAsync(c->d_poison, 0, 2 * sizeof(int), c->stream));  // a probe changes no state
    HIPCHK(hipStreamSynchronize(c->stream));
    return hkc::contact_check(c);
}

}  // extern "C"
