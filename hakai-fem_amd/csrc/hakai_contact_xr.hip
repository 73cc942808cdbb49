// hakai_contact_xr.hip -- the owner-computed multi-GPU contact search (hkc::Xrank): exchange blocks
// and their capacities, the in-process and RCCL gathers, the exchange kernels, phases A1/A2/A3/B of
// a step, and the retry after an overflow. The one-GPU step and the kernels both share are in
// hakai_contact.hip (reached through hakai_contact_state.hpp); device helpers: hakai_contact_dev.hpp.
// Compiled without FP contraction: k_xr_bin forms positions and records with the reference's
// expressions.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstring>
#include <vector>

#include "hakai_contact_dev.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace hkc {

// Multi-GPU contact (hakai_set_contact_global, §8f-3): owner-computed search. Every rank sets up
// the contact model of the GLOBAL mesh (the same host enumeration, so the same entries, pairs and
// hash tables on every rank) and keeps the entries it owns: the triangles of its own elements and
// the node entries of the nodes it owns (owner = the rank of the node's lowest incident element),
// with local node ids, so every position, velocity and element flag the search reads is local. Per
// step (hkc::Xrank, "exchange" kernels below):
//   A1  the previous step's deletions of every rank (global element, step) are all-gathered into a
//       global deletion-step array (live lists: an entry's adders may sit on a neighbour rank);
//       live-list update of the own entries; pair boxes over the own live node entries;
//   A2  the partial boxes are combined (an all-reduce of min/max words, exact); the own live
//       i-nodes inside the pair's range box are binned into compact 96-B records (cell, global
//       node, position, velocity, the mass the damping term reads);
//   A3  the records of every rank are gathered into one hash grid (count, scan, fill), and each
//       rank tests its own candidate triangles (the reference's triangle-parallel loop :2370,
//       per-thread force columns :2386) against every binned i-node: the same candidate set and the
//       same FP64 expressions as one GPU;
//   B   the events of all ranks are all-gathered and every rank forms the same order-independent
//       double-double sums (:2653-2667, :511-517), then takes its own nodes' forces.
// So N ranks are bit-identical to one, and nothing of the model's surface travels per step: only
// deletions, the boxes, the binned contact-zone nodes and the events. Blocks are double-buffered by
// step parity; an in-process group reads its peers' blocks directly (after a stream wait on their
// "packed" events), RCCL all-gathers them. Block capacities (RCCL collectives need host-known
// sizes) are the same on every rank and grow between steps from the counts every rank gathered
// two steps earlier; a burst beyond a capacity poisons that step on every rank, and hakai_step
// grows the capacity and runs the step again (contact_exchange_retry).
// Exchange blocks of every rank: rank q's block at p[q] (RCCL receive buffer or in-process peer)
constexpr int kMaxXRanks = 64;
struct XBlk {
    const char* p[kMaxXRanks];
    int cap[kMaxXRanks];  // records rank q's block holds
    int off[kMaxXRanks];  // prefix of cap: rank q's first slot in arrays over every rank's records
};

struct Xrank {
    int rank = 0, nranks = 1;
    long long E0 = 0, nEloc = 0, nN_g = 0, nE_g = 0;
    int maxEloc = 1;                  // the largest rank's element count (full deletion blocks)
    DevBuf<long long> d_eoff;         // [nranks+1] element ranges
    DevBuf<int> d_l2g;                // [nN local] global node id
    DevBuf<int> d_g2l;                // [nN_g] local node id or -1
    DevBuf<double> g_mass;            // [nN_g] lumped node mass (diag_M[i] with a node id i, :2592)
    DevBuf<int> g_del;                // [nE_g + 2] deletion step; [nE_g + 1] last step with any deletion
    DevBuf<int> d_last_del;           // [nEloc] local deletion steps at the last pack
    // exchange blocks: int4 header (count, overflow, last deletion step, full) + records
    static constexpr int kNx = 3;     // 0 deletions, 1 binned i-nodes, 2 events
    DevBuf<char> d_send[kNx][2];
    size_t send_bytes[kNx] = {0, 0, 0};
    DevBuf<char> d_recv[kNx];         // RCCL: [nranks] blocks
    size_t recv_bytes[kNx] = {0, 0, 0};
    // records per block: capq[x][q] for rank q's block, computed alike on every rank from the
    // gathered counts (so every rank knows every block's size); cap[x] = their maximum
    long long cap[kNx] = {0, 0, 0};
    std::vector<long long> capq[kNx];
    std::vector<int> hist[kNx];       // [q][kHist] recent gathered counts of each rank (the headroom window)
    int hist_pos = 0;
    static constexpr int kHist = 16;
    long long cap_max[kNx] = {0, 0, 0};
    long long cap_floor[kNx] = {1024, 256, 256};  // smallest capacity (tuning contact_exchange_*)
    hipEvent_t ev_sent[kNx][2] = {{nullptr, nullptr}, {nullptr, nullptr}, {nullptr, nullptr}};
    bool full_del = true;             // the next deletion block carries every local deletion step
    // partial pair boxes of this rank, by parity (in-process peers read them), and the combined boxes
    DevBuf<unsigned long long> d_box[2];
    DevBuf<unsigned long long> d_boxg;
    hipEvent_t ev_box[2] = {nullptr, nullptr};
    DevBuf<int> d_xctl;               // [0] exchange overflow bits of the current call (1 del, 2 bins, 4 events);
                                      // [4 ..] the step's gathered counts [kNx][nranks], then their
                                      // maxima since the last overflow growth [kNx][nranks]
    bool retry = false;               // the last poisoned call overflowed an exchange, now grown
    int* h_cnt = nullptr;             // pinned, device-mapped [4][kNx][nranks] gathered counts, written by
    int* d_hcnt = nullptr;            // the kernels that read the blocks (d_hcnt: device view), read two steps later
    hipEvent_t ev_cnt[4] = {nullptr, nullptr, nullptr, nullptr};
    long long seq = 0;                // steps since the last state reset: block parity, count ring
    long long cnt_seq = 0;            // count-ring entries written
    int sl_a = 0;                     // count-ring slot of the current step
    int t_a = 0;                      // step of the current phase A
    long long phase_a = 0;            // phase-A3 calls (equal on the ranks of a lockstep group)
    int par_a = 0;                    // parity of the blocks of the current step

    // the count-ring slot of the current step, as the kernels that read the blocks see it
    int* hcnt_slot() const { return d_hcnt + (size_t)sl_a * kNx * nranks; }

    // (the buffers free themselves after this body)
    ~Xrank() {
        (void)hipDeviceSynchronize();  // in-process peers may still read this rank's blocks
        for (auto& par : ev_sent)
            for (auto& e : par)
                if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_box)
            if (e) (void)hipEventDestroy(e);
        for (auto& e : ev_cnt)
            if (e) (void)hipEventDestroy(e);
        if (h_cnt) (void)hipHostFree(h_cnt);
    }
};
}  // namespace hkc

namespace {

using namespace hkc::ck;
using hkc::Contact;
using hkc::PairParam;
using hkc::Seg;
using hkc::BEnt;
using hkc::BRec;
using hkc::BVel;
using hkc::Xrank;

// ---- multi-GPU exchange (hkc::Xrank) --------------------------------------------------------
// Every exchanged block is an int4 header -- (count, overflow, last deletion step, full) -- and its
// records. Rank q's block is read through XBlk.p[q]: the RCCL-gathered receive buffer, or the
// in-process peer's own send buffer (no copy).
using hkc::kMaxXRanks;
using hkc::XBlk;
__device__ __forceinline__ int xhdr(const char* blk, int w) {
    return __hip_atomic_load(reinterpret_cast<const int*>(blk) + w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
constexpr size_t kXHdr = 16;
constexpr int kNxCount = hkc::Xrank::kNx;

// every rank's block header (count, overflow, last deletion step, full) -> LDS, one lane per rank:
// the loads of all ranks in flight together, not a dependent chain on one thread
__device__ __forceinline__ void load_hdrs(const XBlk& xb, int nr, int4* s_h) {
    const int q = (int)threadIdx.x;
    if (q < nr) {
        const char* b = xb.p[q];
        s_h[q] = make_int4(xhdr(b, 0), xhdr(b, 1), xhdr(b, 2), xhdr(b, 3));
    }
    __syncthreads();
}

struct EvRec {
    int n[4];     // i, j0, j1, j2 (global node ids)
    double f[3];  // force on i (the triangle nodes get -f/3 each)
};

// this rank's events of the step, shard order -> its block; overflow = events beyond a shard or
// candidates beyond their buffer (poisons the step on every rank, k_ct_count_g)
__global__ void k_ev_pack(unsigned int* ctl, const unsigned int* evs, long long shard_cap, const int* ev_nodes,
                          const double* ev_f, char* blk, long long cap) {
    __shared__ unsigned s_pre[kEvShards + 4];
    const long long n = shard_prefix(blockIdx.x, ctl, evs, shard_cap, s_pre);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        const bool over = ctl[kCandOver] != 0 || s_pre[kEvShards + 1];
        int* h = reinterpret_cast<int*>(blk);
        h[0] = (int)n;
        h[1] = over ? 1 : 0;
    }
    EvRec* out = reinterpret_cast<EvRec*>(blk + kXHdr);
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n && e < cap;
         e += (long long)gridDim.x * blockDim.x) {
        const long long sl = shard_slot(s_pre, shard_cap, e);
        EvRec r;
        for (int k = 0; k < 4; ++k) r.n[k] = ev_nodes[4 * sl + k];
        for (int k = 0; k < 3; ++k) r.f[k] = ev_f[3 * sl + k];
        out[e] = r;
    }
}

// rank prefix of the blocks' record counts in LDS (each clamped to the block capacity); block 0
// publishes the event total
__device__ __forceinline__ long long rank_prefix(unsigned int* ctl, const int4* s_h, int nr, long long* s_off,
                                                 const int* cap, bool publish) {
    if (threadIdx.x == 0) {
        long long run = 0;
        for (int q = 0; q < nr; ++q) {
            s_off[q] = run;
            run += min(s_h[q].x, cap[q]);
        }
        s_off[nr] = run;
        if (publish && blockIdx.x == 0) {
            ctl[kEv] = (unsigned)run;
            atomicMax(&ctl[kEvMax], (unsigned)run);
        }
    }
    __syncthreads();
    return s_off[nr];
}

__device__ __forceinline__ int rank_of_rec(const long long* s_off, int nr, long long E) {
    int q = 0;
    while (q + 1 < nr && s_off[q + 1] <= E) ++q;
    return q;
}

__device__ __forceinline__ const EvRec* rank_ev(const XBlk& xb, const long long* s_off, int nr, long long E) {
    const int q = rank_of_rec(s_off, nr, E);
    return reinterpret_cast<const EvRec*>(xb.p[q] + kXHdr) + (E - s_off[q]);
}

// any rank's block over its capacity or flagged: poison step pstep on every rank (all read the same
// headers); xctl records which exchange (bit) for the retry
__device__ __forceinline__ void x_overflow_check(const int4* s_h, int nr, const int* cap, int* poison, int pstep,
                                                 int* xctl, int bit) {
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        bool local = false, over = false;  // a rank's own buffers overflowed / the exchange block
        for (int q = 0; q < nr; ++q) {
            local |= s_h[q].y != 0;
            over |= s_h[q].x > cap[q];
        }
        if (over) atomicOr(xctl, bit);
        if (over || local) poison_from(poison, pstep);
    }
}

// the gathered record counts of exchange x (a full deletion block counts 0): the step's (read back
// for the capacities two steps later) and their maxima (the growth after an overflow). Recorded by
// the kernel that consumes the blocks, so no pointer to a peer's block outlives its step.
__device__ __forceinline__ void x_counts(const int4* s_h, int nr, int x, int* xctl, int* hc) {
    const int q = (int)threadIdx.x;
    if (blockIdx.x == 0 && blockIdx.y == 0 && q < nr) {
        const int v = (x == 0 && s_h[q].w) ? 0 : s_h[q].x;
        xctl[4 + x * nr + q] = v;
        atomicMax(&xctl[4 + (kNxCount + x) * nr + q], v);
        hc[x * nr + q] = v;  // host-mapped ring slot of the step (no copy launch)
    }
}

// every rank's events; only the terms of this rank's nodes (g2l >= 0) are counted and summed
// (also the reset's share of phase B: the previous step's touched nodes' forces back to 0 -- the
// nodal update of that step has read them -- and the term counter)
__global__ void k_ct_count_g(unsigned int* ctl, XBlk xb, int nr, const int* g2l, int* cnt, int* touched,
                             int* tpos, int tsel, int* poison, int pstep, int* xctl, int* hc, const int* touched_prev,
                             double* fext) {
    __shared__ long long s_off[kMaxXRanks + 1];
    __shared__ unsigned s_app[2];
    __shared__ int4 s_h[kMaxXRanks];
    {
        const int np = (int)ld_ctl(&ctl[kTouched + 1 - tsel]);
        for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < np; q += gridDim.x * blockDim.x) {
            const long long l = g2l[touched_prev[q]];
            fext[3 * l] = 0.0;
            fext[3 * l + 1] = 0.0;
            fext[3 * l + 2] = 0.0;
        }
        if (blockIdx.x == 0 && threadIdx.x == 0) ctl[kTerms] = 0;
    }
    load_hdrs(xb, nr, s_h);
    x_overflow_check(s_h, nr, xb.cap, poison, pstep, xctl, 4);
    x_counts(s_h, nr, 2, xctl, hc);
    const long long n = 4 * rank_prefix(ctl, s_h, nr, s_off, xb.cap, true);
    for (long long e0 = blockIdx.x * (long long)blockDim.x; e0 < n; e0 += (long long)gridDim.x * blockDim.x) {
        const long long e = e0 + threadIdx.x;
        int node = -1;
        bool first = false;
        if (e < n) {
            node = rank_ev(xb, s_off, nr, e >> 2)->n[e & 3];
            first = g2l[node] >= 0 && atomicAdd(&cnt[node], 1) == 0;
        }
        const unsigned q = block_append(&ctl[kTouched + tsel], first, s_app);
        if (first) {
            touched[q] = node;
            tpos[node] = (int)q;
        }
    }
}

__global__ void k_ct_scatter_g(XBlk xb, int nr, const int* g2l, unsigned int* ctl, const int* toff,
                               const int* tpos, int* cnt, double* terms) {
#pragma clang fp contract(off)
    __shared__ long long s_off[kMaxXRanks + 1];
    __shared__ int4 s_h[kMaxXRanks];
    load_hdrs(xb, nr, s_h);
    const long long n = 4 * rank_prefix(ctl, s_h, nr, s_off, xb.cap, false);
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < n;
         e += (long long)gridDim.x * blockDim.x) {
        const EvRec* r = rank_ev(xb, s_off, nr, e >> 2);
        const int role = (int)(e & 3);
        const int node = r->n[role];
        if (g2l[node] < 0) continue;
        const int slot = toff[tpos[node]] + atomicSub(&cnt[node], 1) - 1;  // leaves cnt zeroed
        double* o = terms + 3 * (long long)slot;
        term_write(o, role, r->f);
    }
}

// deletions of this rank since the last pack -> its block (global element, step); full: every local
// deletion step (after a state reset / upload / overflow); the header carries the rank's last
// deletion step
// (count of this block: zeroed by the pack of the other parity, which also zeroes the other
// block's for the next pack -- every rank has read that one by now; a step without a deletion
// packs nothing)
__global__ void k_xr_dpack(const int* del_step, const int* del_any, int nEloc, long long E0, int* last_del, char* blk,
                           char* other, long long cap, int full, int t) {
    int* h = reinterpret_cast<int*>(blk);
    int* pl = reinterpret_cast<int*>(blk + kXHdr);
    if (blockIdx.x == 0 && threadIdx.x == 0) reinterpret_cast<int*>(other)[0] = 0;
    const bool none = !full && *del_any != t;  // block-uniform
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; !none && e < nEloc; e += gridDim.x * blockDim.x) {
        const int d = del_step[e];
        if (full) {
            pl[e] = d;
        } else if (d != last_del[e]) {
            const int k = atomicAdd(&h[0], 1);
            if (k < cap) {
                pl[2 * k] = (int)(E0 + e);
                pl[2 * k + 1] = d;
            }
        }
        last_del[e] = d;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        h[2] = *del_any;
        h[3] = full;
    }
}

// every rank's deletion block -> the global deletion steps; block 0 also the global last deletion
// step and the overflow check (a list beyond its capacity poisons the step; it is packed again,
// full, for the retry)
// The incremental blocks also hold exactly the elements deleted in the previous step: they go to
// the deletion list of the live-list update (k_ct_find_del's job on one GPU), and block 0 sets the
// update flag (after k_ct_reset, which clears the list). A full block comes with a full rebuild
// of the live lists on every rank (state reset, upload, overflow retry), which needs no list.
__global__ void k_xr_dunpack(XBlk xb, int nr, const long long* e_off, int* g_del, long long nE_g,
                             int* poison, int t, int* xctl, int* hc, unsigned int* ctl, int* dlist) {
    const int q = (int)blockIdx.y;
    const char* b = xb.p[q];
    const int* pl = reinterpret_cast<const int*>(b + kXHdr);
    __shared__ int4 s_h[kMaxXRanks];
    load_hdrs(xb, nr, s_h);
    x_counts(s_h, nr, 0, xctl, hc);
    if (s_h[q].w) {
        const long long e0 = e_off[q], ne = e_off[q + 1] - e0;
        for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < ne; k += (long long)gridDim.x * blockDim.x)
            g_del[e0 + k] = pl[k];
    } else {
        const long long n = min(s_h[q].x, xb.cap[q]);
        for (long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x; k < n;
             k += (long long)gridDim.x * blockDim.x) {
            const int e = pl[2 * k], d = pl[2 * k + 1];
            g_del[e] = d;
            if (d == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = e;
        }
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
        int mx = 0;
        bool over = false;
        for (int r = 0; r < nr; ++r) {
            mx = max(mx, s_h[r].z);
            over |= !s_h[r].w && s_h[r].x > xb.cap[r];
        }
        g_del[nE_g + 1] = mx;
        ctl[kDel] = (ctl[kDirty] == 0 && mx == t - 1) ? 1u : 0u;
        if (over) {
            atomicOr(xctl, 1);
            poison_from(poison, t);
        }
    }
}

// A1 of a step without a full rebuild (multi-GPU), ONE 1024-thread workgroup: k_ct_reset's share of
// the phase (event and candidate counters, this step's partial box words and bin block header, the
// bucket-head sequence), and every rank's deletion records into the global deletion steps and the
// deletion list; k_ct_append follows with a full grid (in this workgroup, a wave per deleted
// element, the append took 35-63 µs on C4's deletion steps against 15-18 µs for the grid). A rank's
// block that is full (a peer out of step) is unpacked too. The previous step's touched forces and the term counter are
// phase B's (k_ct_count_g), the touched counter the previous k_ct_sum's.
__global__ __launch_bounds__(1024) void k_xr_front(XBlk xb, int nr, const long long* e_off, int* g_del,
                                                   long long nE_g, int* poison, int t, int* xctl, int* hc,
                                                   unsigned int* ctl, int* dlist, unsigned long long* bbox,
                                                   int npairs, unsigned int* evs, unsigned int* ccnt, int* zero_hdr) {
    __shared__ int4 s_h[kMaxXRanks];
    load_hdrs(xb, nr, s_h);
    x_counts(s_h, nr, 0, xctl, hc);
    const int tid = (int)threadIdx.x, bd = (int)blockDim.x;
    if (tid < kEvShards) evs[tid * kShardStride] = 0;
    if (tid < kCandShards)
        ccnt[tid * kShardStride] = ccnt[tid * kShardStride + kTestWord] = ccnt[tid * kShardStride + kItemWord] = 0;
    for (int q = tid; q < box_words(npairs); q += bd) bbox[q] = box_max(q) ? 0ULL : ~0ULL;
    if (tid < 2) zero_hdr[tid] = 0;
    if (tid == 0) {
        int mx = 0;
        bool over = false;
        for (int r = 0; r < nr; ++r) {
            mx = max(mx, s_h[r].z);
            over |= !s_h[r].w && s_h[r].x > xb.cap[r];
        }
        g_del[nE_g + 1] = mx;
        ctl[kEv] = 0;
        ctl[kDirty] = 0;
        ctl[kNdel] = 0;
        ctl[kNcand] = 0;
        ctl[kCandOver] = 0;
        ctl[kSeq] = ctl[kSeq] + 1u;
        ctl[kDel] = mx == t - 1 ? 1u : 0u;
        if (over) {
            atomicOr(xctl, 1);
            poison_from(poison, t);
        }
        __threadfence();  // (the counters before the other waves' atomics and agent-scope loads)
    }
    __syncthreads();
    for (int q = 0; q < nr; ++q) {
        const int* pl = reinterpret_cast<const int*>(xb.p[q] + kXHdr);
        if (s_h[q].w) {
            const long long e0 = e_off[q], ne = e_off[q + 1] - e0;
            for (long long k = tid; k < ne; k += bd) g_del[e0 + k] = pl[k];
        } else {
            const long long n = min(s_h[q].x, xb.cap[q]);
            for (long long k = tid; k < n; k += bd) {
                const int e = pl[2 * k], d = pl[2 * k + 1];
                g_del[e] = d;
                if (d == t - 1) dlist[atomicAdd(&ctl[kNdel], 1u)] = e;
            }
        }
    }
}

// pair boxes of all ranks: min of the min words, max of the max words (exact, order-free). RCCL
// all-reduces with MIN: the max words travel complemented (k_xr_boxflip before and after).
__global__ void k_xr_boxflip(unsigned long long* bb, int npairs) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q < box_words(npairs) && box_max(q)) bb[q] = ~bb[q];
}
struct XBox {
    const unsigned long long* p[kMaxXRanks];
};
__global__ void k_xr_boxcomb(XBox xb, int nr, int npairs, unsigned long long* out) {
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= box_words(npairs)) return;
    const bool mx = box_max(q);
    unsigned long long v = xb.p[0][q];
    for (int r = 1; r < nr; ++r) {
        const unsigned long long w = xb.p[r][q];
        v = mx ? umax64(v, w) : umin64(v, w);
    }
    out[q] = v;
}

// A2: the pair boxes of every rank combined (each workgroup in LDS; workgroup 0 also stores them
// for the triangle prefilter of A3), then this rank's live i-nodes inside their pair's range box ->
// compact records in its block. xb: the in-process peers' partial boxes (nxb = nranks), or the
// RCCL all-reduced one (nxb = 1, max words complemented: flip). npairs > kLdsPairs: k_xr_boxcomb
// combined them into boxg before (nxb = 0).
constexpr int kLdsPairs = 64;
__global__ __launch_bounds__(kB) void k_xr_bin(StepIn s, const Seg* segs, int nseg, const int* reg,
                                               const int* ni_live, const int* ni_pair, const int* ni_node,
                                               const PairParam* par, XBox xb, int nxb, int flip, int npairs,
                                               unsigned long long* boxg, char* blk, long long cap, int sb) {
#pragma clang fp contract(off)
    __shared__ unsigned s_app[2];
    __shared__ alignas(16) unsigned long long s_bb[12 * kLdsPairs + 1];
    const unsigned long long* bbox = boxg;
    if (nxb > 0) {
        for (int q = (int)threadIdx.x; q < box_words(npairs); q += kB) {
            const bool mx = box_max(q);
            unsigned long long v = xb.p[0][q];
            for (int r = 1; r < nxb; ++r) {
                const unsigned long long w = xb.p[r][q];
                v = mx ? umax64(v, w) : umin64(v, w);
            }
            if (flip && mx) v = ~v;
            s_bb[q] = v;
            if (blockIdx.x == 0) boxg[q] = v;
        }
        __syncthreads();
        bbox = s_bb;
    }
    if ((int)blockIdx.x / sb >= nseg) return;  // (nseg = 0: one workgroup, the boxes only)
    const Seg sg = segs[blockIdx.x / sb];
    if (sg.side != 0) return;  // block-uniform
    const int base = reg[2 * sg.region], n = reg[2 * sg.region + 1];
    unsigned int* cnt = reinterpret_cast<unsigned int*>(blk);
    BRec* out = reinterpret_cast<BRec*>(blk + kXHdr);
    for (int q0 = (blockIdx.x % sb) * kB; q0 < n; q0 += sb * kB) {  // block-uniform trip count
        const int q = q0 + (int)threadIdx.x;
        bool in = false;
        int nd = 0, pr = 0;
        double p[3] = {0.0, 0.0, 0.0};
        Range r;
        r.empty = true;
        if (q < n) {
            const int k = ni_live[base + q];
            pr = ni_pair[k];
            r = pair_range(bbox + 12 * pr);
            nd = ni_node[k];
            pos(s, nd, p);
            in = !(r.empty || p[0] < r.mn[0] || p[1] < r.mn[1] || p[2] < r.mn[2] || p[0] > r.mx[0] ||
                   p[1] > r.mx[1] || p[2] > r.mx[2]);  // the candidate test of :2514-2519
        }
        const unsigned slot = block_append(cnt, in, s_app);
        if (in && (long long)slot < cap) {
            BRec e;
            bin_rec(s, r, par[pr], pr, nd, p, e);
            out[slot] = e;
        }
    }
}

// A3: every gathered record (rank q's record k at slot xb.off[q] + k of the bucket list) pushed onto
// its bucket's chain; xctl bit 2 and the poison when a rank binned more than its block holds
// (workgroup bx of gbx over rank q's block)
__device__ __forceinline__ void insert_body(int bx, int gbx, int q, const XBlk& xb, int nr,
                                            const PairParam* par, const unsigned int* ctl, unsigned long long* head,
                                            BEnt* blist, BVel* bvel, int* poison, int pstep, int* xctl, int* hc) {
    __shared__ int4 s_h[kMaxXRanks];
    load_hdrs(xb, nr, s_h);
    x_overflow_check(s_h, nr, xb.cap, poison, pstep, xctl, 2);
    x_counts(s_h, nr, 1, xctl, hc);
    const long long n = min(s_h[q].x, xb.cap[q]);
    const unsigned seq = ctl[kSeq];
    const uint4* rec = reinterpret_cast<const uint4*>(xb.p[q] + kXHdr);  // 6 x 16 B per record
    for (long long k = bx * (long long)blockDim.x + threadIdx.x; k < n; k += (long long)gbx * blockDim.x) {
        // the record moves as six 16-B vectors (a by-value BRec became a 96-B private array in LDS)
        uint4 w[6];
#pragma unroll
        for (int v = 0; v < 6; ++v) w[v] = rec[6 * k + v];
        const PairParam& pp = par[(int)w[1].w];  // BEnt: m[3] = w0.xy w0.zw w1.xy, node w1.z, pad w1.w
        const int b = pp.hash_off + (int)(hash3(ll2(w[0].x, w[0].y), ll2(w[0].z, w[0].w), ll2(w[1].x, w[1].y)) &
                                          (unsigned)(pp.hash_size - 1));
        const int slot = xb.off[q] + (int)k;
        const unsigned long long old = atomicExch(&head[b], ((unsigned long long)seq << 32) | (unsigned)slot);
        const long long nx = (unsigned)(old >> 32) == seq ? (long long)(unsigned)old : -1LL;
        w[3].z = (unsigned)(unsigned long long)nx;  // BEnt::next, the last 8 B
        w[3].w = (unsigned)((unsigned long long)nx >> 32);
        uint4* be = reinterpret_cast<uint4*>(blist + slot);
        uint4* bv = reinterpret_cast<uint4*>(bvel + slot);
#pragma unroll
        for (int v = 0; v < 4; ++v) be[v] = w[v];
        bv[0] = w[4];
        bv[1] = w[5];
    }
}

__global__ void k_xr_insert(XBlk xb, int nr, const PairParam* par, const unsigned int* ctl,
                            unsigned long long* head, BEnt* blist, BVel* bvel, int* poison, int pstep, int* xctl,
                            int* hc) {
    insert_body(blockIdx.x, gridDim.x, blockIdx.y, xb, nr, par, ctl, head, blist, bvel, poison, pstep, xctl, hc);
}

// A3 with the triangle prefilter in the same launch (workgroups [0, gb * nr) insert, the rest
// filter: independent work, side by side)
__global__ __launch_bounds__(kB) void k_xr_insfilter(XBlk xb, int nr, const PairParam* par,
                                                     const unsigned int* ctl, unsigned long long* head, BEnt* blist,
                                                     BVel* bvel, int* poison, int pstep, int* xctl, int* hc, int gb,
                                                     StepIn s, const int* tri_cnt, const int* tri_live,
                                                     const int* tri_pair, const int* tri_nodes, const int* tri_ele,
                                                     const unsigned long long* bbox, unsigned int* ccnt, TriRec* cand,
                                                     long long cshard_cap, uint2* item) {
    const int ni = gb * nr;
    if ((int)blockIdx.x < ni)
        insert_body(blockIdx.x % gb, gb, blockIdx.x / gb, xb, nr, par, ctl, head, blist, bvel, poison, pstep,
                    xctl, hc);
    else
        tri_filter_body(blockIdx.x - ni, gridDim.x - ni, s, tri_cnt, tri_live, tri_pair, tri_nodes, tri_ele, par, bbox,
                        ccnt, cand, cshard_cap, item);
}

}  // namespace

namespace hkc {

// ---- multi-GPU exchange (Xrank) ------------------------------------------------------------------
static size_t xr_rec_bytes(int x) { return x == 0 ? 8 : (x == 1 ? sizeof(BRec) : sizeof(EvRec)); }
// block bytes of rank q's block of exchange x at its capacity (deletions, full: room for every local
// deletion step of the largest rank)
static size_t xr_blkq(const Xrank* X, int x, int q, bool full = false) {
    size_t b = kXHdr + xr_rec_bytes(x) * (size_t)X->capq[x][q];
    if (x == 0 && full) b = kXHdr + 4 * (size_t)X->maxEloc;
    return (b + 15) / 16 * 16;
}
static size_t xr_alloc_blk(const Xrank* X, int x, int q) {
    return x == 0 ? std::max(xr_blkq(X, 0, q, false), xr_blkq(X, 0, q, true)) : xr_blkq(X, x, q);
}
// every rank's block bytes and their offsets in the receive buffer
static size_t xr_layout(const Xrank* X, int x, bool full, size_t* bytes, size_t* off) {
    size_t run = 0;
    for (int q = 0; q < X->nranks; ++q) {
        bytes[q] = xr_blkq(X, x, q, full);
        off[q] = run;
        run += bytes[q];
    }
    return run;
}
// records of the largest block / of all blocks of exchange x
static void xr_cap_sums(Xrank* X, int x) {
    long long mx = 0;
    for (long long v : X->capq[x]) mx = std::max(mx, v);
    X->cap[x] = mx;
}
static long long xr_cap_total(const Xrank* X, int x) {
    long long t = 0;
    for (long long v : X->capq[x]) t += v;
    return t;
}

// send (both parities) and receive buffers for the current capacities; bucket-record and
// bucket-list arrays for the binned records of all ranks. Capacities may shrink (xr_grow); a
// buffer is reallocated only when a capacity outgrows it, then with 1.25x room (a reallocation
// synchronises the device).
static int xr_buffers(hakai_ctx* c) {
    Contact* C = c->contact;
    Xrank* X = C->xr;
    const int nr = X->nranks, me = X->rank;
    bool sync = false;
    size_t need_send[Xrank::kNx], need_recv[Xrank::kNx];
    for (int x = 0; x < Xrank::kNx; ++x) {
        need_send[x] = xr_alloc_blk(X, x, me);
        need_recv[x] = 0;
        for (int q = 0; q < nr; ++q) need_recv[x] += xr_alloc_blk(X, x, q);
        sync |= X->send_bytes[x] < need_send[x] || (comm_is_rccl(c) && X->recv_bytes[x] < need_recv[x]);
    }
    const long long nb = xr_cap_total(X, 1);
    sync |= C->blist_cap < nb;
    if (!sync) return 0;
    HIPCHK(hipDeviceSynchronize());  // (in-process peers read the send blocks)
    auto room = [](size_t b) { return (b + b / 4 + 15) / 16 * 16; };
    for (int x = 0; x < Xrank::kNx; ++x) {
        if (X->send_bytes[x] < need_send[x]) {
            const size_t b = room(need_send[x]);
            for (int p = 0; p < 2; ++p) {
                HIPCHK(X->d_send[x][p].alloc(b));
                HIPCHK(hipMemset(X->d_send[x][p], 0, b));
            }
            X->send_bytes[x] = b;
        }
        if (comm_is_rccl(c) && X->recv_bytes[x] < need_recv[x]) {
            const size_t b = room(need_recv[x]);
            HIPCHK(X->d_recv[x].alloc(b));
            X->recv_bytes[x] = b;
        }
    }
    if (C->blist_cap < nb) {
        const long long n = nb + nb / 4;
        C->d_blist.free();
        C->d_bvel.free();
        HIPCHK(C->d_blist.alloc((size_t)n));
        HIPCHK(C->d_bvel.alloc((size_t)n));
        C->blist_cap = n;
    }
    return 0;
}

// the blocks of exchange x, parity par, of every rank: gathered over RCCL into the receive buffer
// (one grouped send/receive per peer, each block at its own rank's size), or read in place from the
// in-process peers (after a stream wait on their "sent" event); with every block's capacity and
// slot offset
static int xr_gather(hakai_ctx* c, int x, int par, bool full, XBlk& xb) {
    Xrank* X = c->contact->xr;
    const int nr = X->nranks;
    if (nr > kMaxXRanks) return fail(HAKAI_ERR_COMM, "multi-GPU contact: more than %d ranks", kMaxXRanks);
    long long run = 0;
    for (int q = 0; q < nr; ++q) {
        xb.cap[q] = (int)X->capq[x][q];
        xb.off[q] = (int)run;
        run += X->capq[x][q];
    }
    if (run > (long long)INT_MAX)  // (record slots and bucket-list indices are 32-bit)
        return fail(HAKAI_ERR_STATE, "multi-GPU contact: %lld exchange records over the ranks exceed 2^31", run);
    if (comm_is_rccl(c)) {
        size_t bytes[kMaxXRanks], off[kMaxXRanks];
        xr_layout(X, x, full, bytes, off);
        if (int rc = comm_allgatherv_raw(c, X->d_send[x][par], X->d_recv[x], bytes, off)) return rc;
        for (int q = 0; q < nr; ++q) xb.p[q] = q == X->rank ? X->d_send[x][par] : X->d_recv[x] + off[q];
        return 0;
    }
    for (int q = 0; q < nr; ++q) {
        hakai_ctx* pc = comm_peer_ctx(c, q);
        Xrank* P = pc && pc->contact ? pc->contact->xr : nullptr;
        // the peer packed this step's block: deletions at the end of the previous step (seq), bins in
        // this step's A2 (same seq and step), events in this step's A3 (same A3 count; a peer may have
        // ended the step already)
        const bool same = P && P->capq[x] == X->capq[x] &&
                          (x == 0 ? P->seq == X->seq
                                  : x == 1 ? P->seq == X->seq && P->t_a == X->t_a : P->phase_a == X->phase_a);
        if (!same)
            return fail(HAKAI_ERR_STATE, "multi-GPU contact: rank %d is not at the same step (step an in-process group "
                        "with hakai_step_group; hakai_set_contact_global, reset and upload on every rank)", q);
        if (q != X->rank) HIPCHK(hipStreamWaitEvent(c->stream, P->ev_sent[x][par], 0));
        xb.p[q] = P->d_send[x][par];
    }
    return 0;
}

// this rank's deletions since the last pack (or, full, every local deletion step) -> the deletion
// block of step X->seq
static int xr_dpack(hakai_ctx* c, bool full) {
    Xrank* X = c->contact->xr;
    const int par = (int)(X->seq & 1);
    if (full) HIPCHK(hipMemsetAsync(X->d_send[0][par], 0, kXHdr, c->stream));
    const int n = (int)std::max<long long>(X->nEloc, 1);
    hipLaunchKernelGGL(k_xr_dpack, dim3((unsigned)std::min((n + kB - 1) / kB, 1024)), dim3(kB), 0, c->stream,
                       c->d_del_step, c->d_del_step + c->nEp + 1, (int)X->nEloc, X->E0, X->d_last_del,
                       X->d_send[0][par], X->d_send[0][1 - par], X->capq[0][X->rank], full ? 1 : 0, X->t_a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(X->ev_sent[0][par], c->stream));
    X->full_del = full;
    return 0;
}

// Capacity of a block from its rank's recent counts: 1.25x the largest of the last kHist gathered
// counts plus a floor of records (the counts are two steps old when read: a burst beyond the
// headroom overflows, and the step runs again with the capacity grown past it, contact_after_overflow).
// Deletion blocks (8 B records, bursts at deletion waves) keep a floor of 1024 records.
static long long xr_cap_target(const Xrank* X, int x, long long mx) {
    return std::min<long long>(X->cap_max[x], std::max<long long>(X->cap_floor[x], mx + mx / 4 + (mx > 0 ? 32 : 0)));
}
// Capacities from the counts gathered two steps ago (the same numbers on every rank, so every rank
// sizes every block alike): a rank's block grows to its target at once and shrinks to it once it
// exceeds 1.5x the target (the headroom window keeps a recent burst's size). Exchange x in [x0, x1):
// the deletion block changes before it is packed (end of a step), the bin and event blocks at the
// start of the step that packs them -- never while an in-process peer may still read the block of
// the step before.
static int xr_grow(hakai_ctx* c, int x0, int x1) {
    Xrank* X = c->contact->xr;
    if (X->cnt_seq < 2) return 0;
    const long long sl = (X->cnt_seq - 2) & 3;
    HIPCHK(hipEventSynchronize(X->ev_cnt[sl]));
    const int* h = X->h_cnt + (size_t)sl * Xrank::kNx * X->nranks;
    const int nr = X->nranks, H = Xrank::kHist;
    for (int x = x0; x < x1; ++x) {
        for (int q = 0; q < nr; ++q) {
            int* hq = X->hist[x].data() + (size_t)q * H;
            hq[(X->cnt_seq - 2) % H] = h[x * nr + q];
            long long mx = 0;
            for (int j = 0; j < H; ++j) mx = std::max<long long>(mx, hq[j]);
            const long long tg = xr_cap_target(X, x, mx);
            long long& cq = X->capq[x][q];
            if (tg > cq || 2 * cq > 3 * tg) cq = tg;
        }
        xr_cap_sums(X, x);
    }
    return xr_buffers(c);
}

// state reset / upload: every deletion step travels with the next block
int xr_state_reset(hakai_ctx* c) {
    Xrank* X = c->contact->xr;
    HIPCHK(hipMemsetAsync(X->g_del, 0, ((size_t)X->nE_g + 2) * sizeof(int), c->stream));
    HIPCHK(hipMemsetAsync(X->d_xctl, 0, (4 + 2 * (size_t)Xrank::kNx * X->nranks) * sizeof(int), c->stream));
    X->seq = 0;
    X->cnt_seq = 0;
    return xr_dpack(c, true);
}

// multi-GPU, after the element kernel of a step: capacities for the next step, then this step's
// deletions into the next step's deletion block
int contact_post_step(hakai_ctx* c) {
    Contact* C = c->contact;
    if (!C || !C->xr) return 0;
    Xrank* X = C->xr;
    ++X->seq;
    if (int rc = xr_grow(c, 0, 1)) return rc;
    return xr_dpack(c, false);
}

// the step's input arrays of a rank: its own state, the global mass and deletion steps
static StepIn xr_step_in(hakai_ctx* c, double t, double d_time) {
    const Xrank* X = c->contact->xr;
    StepIn in = step_in(c, t, d_time);
    in.mass = X->g_mass;
    in.l2g = X->d_l2g;
    in.del_step = X->g_del;
    return in;
}

// A1 (multi-GPU): capacities, the deletions of the previous step of every rank, the step prologue,
// the live-list update of the own entries, this rank's partial pair boxes
int xr_a1(hakai_ctx* c, double t, double d_time) {
    Contact* C = c->contact;
    Xrank* X = C->xr;
    hipStream_t s = c->stream;
    const StepIn in = xr_step_in(c, t, d_time);
    if (int rc = xr_grow(c, 1, Xrank::kNx)) return rc;
    X->t_a = in.t;
    X->par_a = (int)(X->seq & 1);
    X->sl_a = (int)(X->cnt_seq & 3);
    XBlk xb{};
    if (int rc = xr_gather(c, 0, X->par_a, X->full_del, xb)) return rc;
    unsigned long long* bbox = X->d_box[X->par_a];
    int* bin_hdr = reinterpret_cast<int*>(X->d_send[1][X->par_a].get());  // this step's bin block (count, overflow)
    if (!step_begin(C, in.t)) {
        // the reset's share and every rank's deletions in one workgroup, then the append
        hipLaunchKernelGGL(k_xr_front, dim3(1), dim3(1024), 0, s, xb, X->nranks, X->d_eoff, X->g_del, X->nE_g,
                           c->d_poison, in.t, X->d_xctl, X->hcnt_slot(), C->d_ctl, C->d_dlist, bbox, C->npairs,
                           C->d_evs, C->d_ccnt, bin_hdr);
    } else {
        // full rebuild: the reset, then the deletions of every rank (after the reset: they fill its
        // deletion list), then the live lists from the global deletion steps
        launch_reset(c, bbox, true, nullptr, in.t, X->d_g2l, bin_hdr);
        const unsigned gx = (unsigned)std::min<long long>(std::max<long long>((X->maxEloc + kB - 1) / kB, 1), 256);
        hipLaunchKernelGGL(k_xr_dunpack, dim3(gx, (unsigned)X->nranks), dim3(kB), 0, s, xb, X->nranks, X->d_eoff,
                           X->g_del, X->nE_g, c->d_poison, in.t, X->d_xctl, X->hcnt_slot(), C->d_ctl, C->d_dlist);
        live_rebuild(c, X->g_del, in.t);
    }
    live_append(c, X->g_del, in.t);  // (k_xr_front / k_xr_dunpack listed the deleted elements)
    launch_boxes(c, in, bbox);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(X->ev_box[X->par_a], s));
    return 0;
}


// A2 (multi-GPU): the pair boxes of every rank combined, then this rank's live i-nodes inside
// their range boxes binned into its block
int xr_a2(hakai_ctx* c, double d_time) {
    Contact* C = c->contact;
    Xrank* X = C->xr;
    hipStream_t s = c->stream;
    const int par = X->par_a, nw = box_words(C->npairs);
    const unsigned gw = (unsigned)((nw + kB - 1) / kB);
    XBox xb{};
    int nxb = 0, flip = 0;
    if (comm_is_rccl(c)) {  // min words as they are, max words complemented: one MIN all-reduce, in place
        hipLaunchKernelGGL(k_xr_boxflip, dim3(gw), dim3(kB), 0, s, X->d_box[par], C->npairs);
        if (int rc = comm_allreduce_min_u64(c, X->d_box[par], X->d_box[par], (size_t)nw)) return rc;
        xb.p[0] = X->d_box[par];
        nxb = 1;
        flip = 1;
    } else {
        for (int q = 0; q < X->nranks; ++q) {
            hakai_ctx* pc = comm_peer_ctx(c, q);
            Xrank* P = pc && pc->contact ? pc->contact->xr : nullptr;
            if (!P || P->seq != X->seq || P->t_a != X->t_a)
                return fail(HAKAI_ERR_STATE, "multi-GPU contact: rank %d has not started step %d", q, X->t_a);
            if (q != X->rank) HIPCHK(hipStreamWaitEvent(s, P->ev_box[par], 0));
            xb.p[q] = P->d_box[par];
        }
        nxb = X->nranks;
    }
    if (C->npairs > kLdsPairs) {  // combined in global memory first
        if (flip) hipLaunchKernelGGL(k_xr_boxflip, dim3(gw), dim3(kB), 0, s, X->d_box[par], C->npairs);
        hipLaunchKernelGGL(k_xr_boxcomb, dim3(gw), dim3(kB), 0, s, xb, nxb, C->npairs, X->d_boxg);
        nxb = 0;
        flip = 0;
    }
    {  // (bin block header zeroed by this step's k_ct_reset)
        const StepIn in = xr_step_in(c, X->t_a, d_time);
        hipLaunchKernelGGL(k_xr_bin, dim3((unsigned)std::max(1, C->nseg * C->g_seg)), dim3(kB), 0, s, in,
                           C->d_seg, C->nseg, C->d_reg, C->d_ni_live, C->d_ni_pair, C->d_ni_node, C->d_par,
                           xb, nxb, flip, C->npairs, X->d_boxg, X->d_send[1][par], X->capq[1][X->rank], C->g_seg);
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(X->ev_sent[1][par], s));
    return 0;
}

// A3 (multi-GPU): one hash grid of every rank's binned i-nodes; this rank's own triangles searched
// against it; its events packed for phase B
int xr_a3(hakai_ctx* c, double d_time) {
    Contact* C = c->contact;
    Xrank* X = C->xr;
    hipStream_t s = c->stream;
    const int par = X->par_a;
    XBlk xb;
    if (int rc = xr_gather(c, 1, par, false, xb)) return rc;
    const unsigned gb = (unsigned)std::min<long long>(std::max<long long>((X->cap[1] + kB - 1) / kB, 1), 128);
    int* hc = X->hcnt_slot();
    const StepIn in = xr_step_in(c, X->t_a, d_time);
    if (C->n_tri > 0 && C->fuse_binfilter) {  // insert and prefilter side by side
        hipLaunchKernelGGL(k_xr_insfilter, dim3(gb * (unsigned)X->nranks + filter_grid(C)), dim3(kB), 0, s, xb,
                           X->nranks, C->d_par, C->d_ctl, C->d_head, C->d_blist, C->d_bvel, c->d_poison,
                           X->t_a, X->d_xctl, hc, (int)gb, in, C->d_reg + 2 * C->tri_reg + 1, C->d_tri_live,
                           C->d_tri_pair, C->d_tri_nodes, C->d_tri_ele, X->d_boxg, C->d_ccnt, C->d_cand,
                           C->cshard_cap, C->small ? nullptr : C->d_item);
        tri_search(c, in);
    } else {
        hipLaunchKernelGGL(k_xr_insert, dim3(gb, (unsigned)X->nranks), dim3(kB), 0, s, xb, X->nranks,
                           C->d_par, C->d_ctl, C->d_head, C->d_blist, C->d_bvel, c->d_poison, X->t_a, X->d_xctl, hc);
        if (C->n_tri > 0) {
            tri_prefilter(c, in, X->d_boxg);
            tri_search(c, in);
        }
    }
    hipLaunchKernelGGL(k_ev_pack, dim3((unsigned)C->g_ev), dim3(kB), 0, s, C->d_ctl, C->d_evs, C->cap / kEvShards,
                       C->d_ev_nodes, C->d_ev_f, X->d_send[2][par], X->capq[2][X->rank]);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(X->ev_sent[2][par], s));
    ++X->phase_a;
    C->use_velo0 = false;
    return 0;
}

// Phase B (multi-GPU): every rank's events -- RCCL all-gather, or the in-process peers' blocks read
// in place -- and the same count / scatter / double-double sums as one GPU, in the global node
// space; the sums of this rank's nodes go to its external force. Also records the step's gathered
// counts for the capacities of later steps.
int contact_step_b(hakai_ctx* c) {
    Contact* C = c->contact;
    Xrank* X = C ? C->xr : nullptr;
    if (!X) return 0;
    hipStream_t s = c->stream;
    const int par = X->par_a, nr = X->nranks;
    XBlk xb;
    if (int rc = xr_gather(c, 2, par, false, xb)) return rc;
    const int tsel = C->tsel;
    const unsigned ge = (unsigned)C->g_ev;
    hipLaunchKernelGGL(k_ct_count_g, dim3(ge), dim3(kB), 0, s, C->d_ctl, xb, nr, X->d_g2l, C->d_cnt,
                       C->d_touched[tsel], C->d_tpos, tsel, c->d_poison, X->t_a, X->d_xctl, X->hcnt_slot(),
                       C->d_touched[1 - tsel], c->d_fext);
    launch_alloc(c);
    hipLaunchKernelGGL(k_ct_scatter_g, dim3(ge), dim3(kB), 0, s, xb, nr, X->d_g2l, C->d_ctl, C->d_toff,
                       C->d_tpos, C->d_cnt, C->d_terms);
    launch_sum(c, X->d_g2l);
    // the step's counts (k_xr_dunpack, k_xr_bcount, k_ct_count_g wrote them into the host-mapped
    // ring slot), read by xr_grow two steps later
    HIPCHK(hipEventRecord(X->ev_cnt[X->sl_a], s));
    ++X->cnt_seq;
    HIPCHK(hipGetLastError());
    return 0;
}

// After a poisoned call (contact_after_overflow): if an exchange capacity overflowed (the same on
// every rank: they read the same headers), grow it past every count of the failed step and pack
// every deletion step again, so the step can run again from there (contact_exchange_retry).
void xr_after_overflow(hakai_ctx* c) {
    Xrank* X = c->contact->xr;
    int xc[4 + 2 * Xrank::kNx * kMaxXRanks] = {0};
    const int nr = X->nranks;
    const size_t n = 4 + 2 * (size_t)Xrank::kNx * nr;
    if (hipMemcpyAsync(xc, X->d_xctl, n * sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
        hipStreamSynchronize(c->stream) != hipSuccess)
        return;
    X->retry = false;
    if (xc[0] & 7) {  // past the largest count of the call (its steps after the poisoned one included)
        for (int x = 0; x < Xrank::kNx; ++x) {
            if (!(xc[0] & (1 << x))) continue;
            for (int q = 0; q < nr; ++q) {  // every block past its rank's largest count of the call
                const long long mx = xc[4 + (Xrank::kNx + x) * nr + q];
                X->capq[x][q] = std::max(X->capq[x][q], xr_cap_target(X, x, mx));
                int* hq = X->hist[x].data() + (size_t)q * Xrank::kHist;  // (kept by the window)
                for (int j = 0; j < Xrank::kHist; ++j) hq[j] = std::max<int>(hq[j], (int)std::min<long long>(mx, 1 << 30));
            }
            xr_cap_sums(X, x);
        }
        X->retry = true;
    }
    (void)hipMemsetAsync(X->d_xctl, 0, n * sizeof(int), c->stream);
    if (xr_buffers(c) == 0) (void)xr_dpack(c, true);
}

bool contact_exchange_retry(hakai_ctx* c) {
    Contact* C = c->contact;
    if (!C || !C->xr || !C->xr->retry) return false;
    C->xr->retry = false;
    return true;
}

// tuning keys contact_exchange_deletions / _bins / _events: records per rank block of an exchange
// (call on every rank, between steps); capacities also grow on their own, and a step that
// overflows one runs again (hakai_step)
int xr_tuning(hakai_ctx* c, const char* key, long long value) {
    Contact* C = c->contact;
    Xrank* X = C->xr;
    const int x = key[17] == 'd' ? 0 : (key[17] == 'b' ? 1 : 2);
    if (value < 1 || value > (1LL << 28)) return fail(HAKAI_ERR_ARG, "%s out of range", key);
    HIPCHK(hipDeviceSynchronize());
    for (auto& v : X->capq[x]) v = std::min<long long>(value, X->cap_max[x]);
    X->cap_floor[x] = value;  // (the capacities then follow the counts from there)
    xr_cap_sums(X, x);
    if (int rc = xr_buffers(c)) return rc;
    // the next step's deletion block again, in the new layout (a full block: every rank
    // rebuilds its live lists)
    if (x == 0 && c->state_ok) {
        C->force_rebuild = true;
        return xr_dpack(c, true);
    }
    return 0;
}

// the event block can hold at most the event buffer
void xr_event_cap(Contact* C) {
    Xrank* X = C->xr;
    X->cap_max[2] = C->cap;
    for (auto& v : X->capq[2]) v = std::min(v, C->cap);
    xr_cap_sums(X, 2);
}

int xr_check(hakai_ctx* c) {
    const Xrank* X = c->contact->xr;
    int xc = 0;
    HIPCHK(hipMemcpy(&xc, X->d_xctl, sizeof(int), hipMemcpyDeviceToHost));
    if (xc & 7)
        return fail(HAKAI_ERR_STATE, "contact exchange: a rank's %s exceeded its block (capacities now %lld / %lld / "
                    "%lld records; grown for the next step)", (xc & 1) ? "deletions" : (xc & 2) ? "binned contact "
                    "nodes" : "events", X->cap[0], X->cap[1], X->cap[2]);
    return 0;
}

// hakai_contact_stats [7], [8], [11]: contact-zone i-nodes all ranks binned in the last step; the
// bytes this rank's exchanges receive per step (the other ranks' blocks at their capacities) and
// the bytes of the records in them (headers + the last step's gathered counts)
int xr_stats(hakai_ctx* c, long long* binned, long long* bytes, long long* rec_bytes) {
    const Xrank* X = c->contact->xr;
    const int nr = X->nranks;
    std::vector<int> cnt((size_t)Xrank::kNx * nr);
    HIPCHK(hipMemcpy(cnt.data(), X->d_xctl + 4, cnt.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int q = 0; q < nr; ++q) *binned += cnt[(size_t)nr + q];
    for (int x = 0; x < Xrank::kNx; ++x)
        for (int q = 0; q < nr; ++q) {
            if (q == X->rank) continue;
            *bytes += (long long)xr_blkq(X, x, q);
            *rec_bytes += (long long)kXHdr + (long long)xr_rec_bytes(x) * cnt[(size_t)x * nr + q];
        }
    return 0;
}

void xr_destroy(Contact* C) {
    delete C->xr;
    C->xr = nullptr;
}

}  // namespace hkc

namespace {

// Multi-GPU (hkc::Xrank) for a contact set up on the global mesh with this rank's entries: the
// node maps, the global mass and deletion arrays, the exchange blocks; packs the first deletion
// block if a state exists.
int xr_build(hakai_ctx* c, const hkc::ContactOwnership& own, const std::vector<long long>& ni_per_rank, long long nNode,
             long long nElement, const double* diag_M, const int64_t* local_node_global) {
    const int64_t* rank_elem_off = own.rank_elem_off;
    hkc::Contact* C = c->contact;
    auto* X = new hkc::Xrank();
    C->xr = X;
    const int nr = own.nranks;
    X->rank = own.rank;
    X->nranks = nr;
    X->E0 = rank_elem_off[own.rank];
    X->nEloc = rank_elem_off[own.rank + 1] - rank_elem_off[own.rank];
    X->nN_g = nNode;
    X->nE_g = nElement;
    std::vector<long long> eoff((size_t)nr + 1);
    for (int q = 0; q <= nr; ++q) eoff[q] = rank_elem_off[q];
    for (int q = 0; q < nr; ++q) X->maxEloc = std::max<int>(X->maxEloc, (int)(eoff[q + 1] - eoff[q]));
    long long ci0 = 0, nimax = 1;
    for (int p = 0; p < C->npairs; ++p) ci0 += C->pair_counts[3 * p];
    for (long long v : ni_per_rank) nimax = std::max(nimax, v);
    // capacities (records per rank block): deletions up to a rank's elements, binned i-nodes up to
    // the entries a rank owns, events up to the event buffer; they start small and grow
    X->cap_max[0] = X->maxEloc;
    X->cap_max[1] = nimax;
    X->cap_max[2] = C->cap;
    const long long cap0[hkc::Xrank::kNx] = {std::min<long long>(X->cap_max[0], 1024),
                                        std::min<long long>(X->cap_max[1], std::max<long long>(4096, ci0 / (8 * nr))),
                                        std::min<long long>(X->cap_max[2], 4096)};
    for (int x = 0; x < hkc::Xrank::kNx; ++x) {
        X->capq[x].assign((size_t)nr, cap0[x]);
        X->hist[x].assign((size_t)nr * hkc::Xrank::kHist, 0);
        xr_cap_sums(X, x);
    }
    std::vector<int> l2g((size_t)c->nN);
    for (long long l = 0; l < c->nN; ++l) l2g[l] = (int)(local_node_global[l] - 1);
    std::vector<double> gmass((size_t)nNode);
    for (long long n = 0; n < nNode; ++n) gmass[n] = diag_M[3 * n];
    hipStream_t s = c->stream;
    HIPCHK(X->d_l2g.upload(l2g, s));
    HIPCHK(X->d_g2l.upload(*own.g2l, s));
    HIPCHK(X->g_mass.upload(gmass, s));
    HIPCHK(X->d_eoff.upload(eoff, s));
    HIPCHK(X->g_del.alloc((size_t)nElement + 2));
    HIPCHK(hipMemsetAsync(X->g_del, 0, ((size_t)nElement + 2) * sizeof(int), s));
    HIPCHK(X->d_last_del.alloc((size_t)std::max<long long>(X->nEloc, 1)));
    HIPCHK(hipMemsetAsync(X->d_last_del, 0, (size_t)std::max<long long>(X->nEloc, 1) * sizeof(int), s));
    HIPCHK(X->d_xctl.alloc(4 + 2 * (size_t)hkc::Xrank::kNx * nr));
    HIPCHK(hipMemsetAsync(X->d_xctl, 0, (4 + 2 * (size_t)hkc::Xrank::kNx * nr) * sizeof(int), s));
    for (int p = 0; p < 2; ++p) {
        HIPCHK(X->d_box[p].alloc((size_t)box_words(C->npairs)));
        HIPCHK(hipEventCreateWithFlags(&X->ev_box[p], hipEventDisableTiming));
        for (int x = 0; x < hkc::Xrank::kNx; ++x) HIPCHK(hipEventCreateWithFlags(&X->ev_sent[x][p], hipEventDisableTiming));
    }
    HIPCHK(X->d_boxg.alloc((size_t)box_words(C->npairs)));
    HIPCHK(hipHostMalloc((void**)&X->h_cnt, 4 * (size_t)hkc::Xrank::kNx * nr * sizeof(int),
                         hipHostMallocMapped | hipHostMallocCoherent));
    std::fill(X->h_cnt, X->h_cnt + 4 * (size_t)hkc::Xrank::kNx * nr, 0);
    HIPCHK(hipHostGetDevicePointer((void**)&X->d_hcnt, X->h_cnt, 0));
    for (auto& e : X->ev_cnt) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    HIPCHK(hipStreamSynchronize(s));
    if (int rc = hkc::xr_buffers(c)) return rc;
    if (c->state_ok)
        if (int rc = hkc::contact_state_reset(c, c->h_velo0.empty() ? nullptr : c->h_velo0.data())) return rc;
    HIPCHK(hipStreamSynchronize(s));
    return 0;
}

}  // namespace

extern "C" {

int hakai_set_contact_global(hakai_ctx* c, int32_t contact_flag, int64_t nNode, const double* coordmat,
                             int64_t nElement, const int64_t* elementmat, const int64_t* element_material,
                             const int64_t* element_instance, const double* diag_M, const int64_t* local_node_global,
                             const int64_t* rank_elem_off, int32_t n_cp, const int32_t* cp_instance,
                             const int64_t* cp_elem_off, const int64_t* cp_elems) {
    if (c) hkc::graph_invalidate(c);  // captured steps may hold stale buffers or settings
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (n_cp < 0 || (n_cp > 0 && (!cp_instance || !cp_elem_off || !cp_elems)))
        return fail(HAKAI_ERR_ARG, "set_contact_global: bad contact-pair arrays");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "set_contact_global before upload_model");
    if (!c->comm) return fail(HAKAI_ERR_STATE, "set_contact_global before comm_init / comm_init_local");
    HIPCHK(hipSetDevice(c->device));
    hkc::contact_destroy(c);
    if (contact_flag < 1) return 0;
    if (contact_flag > 2) return fail(HAKAI_ERR_ARG, "contact_flag %d (0, 1 or 2)", contact_flag);
    if (nNode <= 0 || nElement <= 0 || !coordmat || !elementmat || !element_material || !diag_M ||
        !local_node_global || !rank_elem_off)
        return fail(HAKAI_ERR_ARG, "set_contact_global: bad arguments");
    if (nNode >= (int64_t)INT32_MAX || 8 * nElement >= (int64_t)INT32_MAX)
        return fail(HAKAI_ERR_ARG, "set_contact_global: mesh too large for int32 indexing");
    const int nr = hkc::comm_size(c), rank = hkc::comm_rank(c);
    if (rank_elem_off[0] != 0 || rank_elem_off[nr] != nElement)
        return fail(HAKAI_ERR_ARG, "set_contact_global: rank_elem_off must run from 0 to nElement");
    for (int q = 0; q < nr; ++q)
        if (rank_elem_off[q + 1] < rank_elem_off[q]) return fail(HAKAI_ERR_ARG, "set_contact_global: rank_elem_off decreases");
    if (rank_elem_off[rank] != c->elem_offset || rank_elem_off[rank + 1] - rank_elem_off[rank] != c->nE)
        return fail(HAKAI_ERR_ARG, "set_contact_global: rank %d holds elements %lld..+%lld, rank_elem_off says %lld..%lld",
                    rank, c->elem_offset, c->nE, (long long)rank_elem_off[rank], (long long)rank_elem_off[rank + 1]);
    std::vector<double> gx(coordmat, coordmat + 3 * nNode);
    std::vector<int> gconn(8 * (size_t)nElement), gmat((size_t)nElement);
    for (int64_t e = 0; e < nElement; ++e) {
        for (int i = 0; i < 8; ++i) {
            const int64_t n = elementmat[8 * e + i];
            if (n < 1 || n > nNode) return fail(HAKAI_ERR_ARG, "set_contact_global: elementmat[%d,%lld] = %lld", i + 1, (long long)e + 1, (long long)n);
            gconn[8 * e + i] = (int)(n - 1);
        }
        const int64_t m = element_material[e];
        if (m < 1 || m > c->nmat) return fail(HAKAI_ERR_ARG, "set_contact_global: element_material[%lld] = %lld", (long long)e + 1, (long long)m);
        gmat[e] = (int)(m - 1);
    }
    // local -> global nodes, checked against this rank's uploaded connectivity
    std::vector<int> g2l((size_t)nNode, -1);
    for (long long l = 0; l < c->nN; ++l) {
        const int64_t g = local_node_global[l];
        if (g < 1 || g > nNode || g2l[g - 1] >= 0)
            return fail(HAKAI_ERR_ARG, "set_contact_global: local_node_global[%lld] = %lld", l + 1, (long long)g);
        g2l[g - 1] = (int)l;
    }
    for (long long e = 0; e < c->nE; ++e)
        for (int i = 0; i < 8; ++i)
            if (gconn[8 * (c->elem_offset + e) + i] != local_node_global[c->h_conn[8 * e + i]] - 1)
                return fail(HAKAI_ERR_ARG, "set_contact_global: local element %lld differs from global element %lld", e + 1,
                            c->elem_offset + e + 1);
    if (nr > hkc::kMaxXRanks) return fail(HAKAI_ERR_ARG, "set_contact_global: more than %d ranks", hkc::kMaxXRanks);
    // the plan keeps this rank's entries: those of the nodes it owns and of its elements
    hkc::ContactOwnership own;
    own.rank = rank, own.nranks = nr, own.rank_elem_off = rank_elem_off, own.g2l = &g2l;
    hkc::ContactInput in;
    in.nN = nNode, in.nE = nElement, in.coord = &gx, in.conn = &gconn, in.mat = &gmat;
    in.young = &c->h_young, in.contact_flag = contact_flag, in.element_instance = element_instance;
    in.n_cp = n_cp, in.cp_instance = cp_instance, in.cp_elem_off = cp_elem_off, in.cp_elems = cp_elems;
    in.own = &own;
    hkc::ContactPlan plan;
    int rc = hkc::contact_setup(c, in, plan);
    if (rc || !c->contact) return rc;
    rc = xr_build(c, own, plan.ni_per_rank, nNode, nElement, diag_M, local_node_global);
    if (rc) hkc::contact_destroy(c);
    return rc;
}

}  // extern "C"
