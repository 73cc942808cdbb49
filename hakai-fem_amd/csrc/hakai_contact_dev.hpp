// hakai_contact_dev.hpp -- device code both translation units of the contact search call
// (hakai_contact.hip: the one-GPU step; hakai_contact_xr.hip: the multi-GPU exchange): the encoded
// pair boxes, the control words and shard counters, the step's input arrays, block-wide appends,
// the hash-record forms and the triangle prefilter. Everything is __forceinline__: no kernel calls
// into this header, it is compiled into each kernel that names it.
#pragma once
#include <hip/hip_runtime.h>

#include "hakai_contact_cells.hpp"
#include "hakai_contact_state.hpp"

namespace hkc {
namespace ck {

constexpr int kB = 256;

__device__ __forceinline__ unsigned long long enc(double d) {
    const unsigned long long u = (unsigned long long)__double_as_longlong(d);
    return (u >> 63) ? ~u : (u | 0x8000000000000000ULL);
}
__device__ __forceinline__ double dec(unsigned long long e) {
    const unsigned long long u = (e >> 63) ? (e & 0x7FFFFFFFFFFFFFFFULL) : ~e;
    return __longlong_as_double((long long)u);
}

__device__ __forceinline__ double my3norm(double a, double b, double c) {
#pragma clang fp contract(off)
    return sqrt(a * a + b * b + c * c);
}

__device__ __forceinline__ unsigned hash3(long long x, long long y, long long z) {
    const unsigned long long h = (unsigned long long)x * 0x9E3779B97F4A7C15ULL ^
                                 (unsigned long long)y * 0xC2B2AE3D27D4EB4FULL ^
                                 (unsigned long long)z * 0x165667B19E3779F9ULL;
    return (unsigned)(h ^ (h >> 29));
}

struct Range {
    double mn[3], mx[3], amn[3];
    bool empty;
};

__device__ __forceinline__ Range pair_range(const unsigned long long* bb_) {
    // the pair's 12 words as six 16-B loads, all in flight together (bbox + 12 * pair is 16-B aligned)
    unsigned long long bb[12];
#pragma unroll
    for (int w = 0; w < 6; ++w) {
        const ulonglong2 v = reinterpret_cast<const ulonglong2*>(bb_)[w];
        bb[2 * w] = v.x;
        bb[2 * w + 1] = v.y;
    }
    Range r;
    r.empty = false;
#pragma unroll
    for (int d = 0; d < 3; ++d) {  // branch-free: a side without live nodes makes the range empty
        const bool none = bb[d] == ~0ULL || bb[6 + d] == ~0ULL;
        const double mni = dec(bb[d]), mxi = dec(bb[3 + d]), mnj = dec(bb[6 + d]), mxj = dec(bb[9 + d]);
        r.empty |= none;
        r.mn[d] = none ? 0.0 : fmax(mni, mnj);
        r.mx[d] = none ? 0.0 : fmin(mxi, mxj);
        r.amn[d] = none ? 0.0 : fmin(mni, mnj);
    }
    if (!r.empty && (r.mn[0] > r.mx[0] || r.mn[1] > r.mx[1] || r.mn[2] > r.mx[2])) r.empty = true;  // :2304-2306
    return r;
}

// Control words (device): events this step, max events seen, full rebuild of the live lists,
// incremental update (an element was deleted in the previous step), deleted elements found, and
// the number of nodes with contact force in each of the two ping-pong "touched" lists.
enum { kEv = 0, kEvMax = 1, kDirty = 2, kDel = 3, kNdel = 4, kTouched = 5 /* [5], [6] */, kNcand = 7, kTerms = 8,
       kNcandMax = 9, kEvShardMax = 10, kCandShardMax = 11, kCandOver = 12, kSeq = 13, kItemShardMax = 14,
       kCtl = 16 };
// Events are appended into kEvShards shards, each with its own counter on its own 128-B line: with
// one counter, every wave that found an event waited on the same memory-side atomic (measured:
// 0.13 ms of a 0.30 ms contact step on C4).
constexpr int kEvShards = 64;
constexpr int kShardStride = 32;  // unsigned ints between shard counters
// Candidate triangles likewise: prefilter block b appends to shard b % kCandShards (one atomic per
// block on that shard's counter; clustered candidates fall in consecutive blocks, so shards stay even).
constexpr int kCandShards = 64;
constexpr int kItemWord = 1;       // a shard's item counter: with the candidate counter one 64-bit word
constexpr int kTestWord = 8;       // triangles the shard's prefilter blocks tested in full (stats)
constexpr int kItemsPerCand = 16;  // item capacity per candidate slot (a candidate has <= 27)
constexpr int kFilterBlocks = 2048;  // prefilter grid cap

// Counters the kernels of one launch read after other workgroups' (or, in the fused small-deck
// kernels, other waves') atomics: an agent-scope load, never a stale L1 line.
__device__ __forceinline__ unsigned ld_ctl(const unsigned int* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The box array: 12 words per pair (pair_range), ordered-integer encoded doubles; min words start
// at +inf, max words at -inf (0).
__host__ __device__ __forceinline__ int box_words(int npairs) { return 12 * npairs; }
__device__ __forceinline__ bool box_max(int q) { return ((q % 12) / 3) % 2 == 1; }

// A buffer overflowed in step `step`: the first one of a call poisons it from that step on (the
// nodal, BC, element and interface kernels then write nothing, hakai_device.hpp poisoned)
__device__ __forceinline__ void poison_from(int* poison, int step) {
    if (poison[0] == 0) {
        poison[1] = step;
        poison[0] = 1;
    }
}

// an event's term of one of its four nodes: role 0 (the contact point) gets f, the triangle nodes
// -f / 3.0 each (c_force3, :2653-2667)
__device__ __forceinline__ void term_write(double* o, int role, const double* f) {
#pragma clang fp contract(off)
    if (role == 0) {
        o[0] = f[0];
        o[1] = f[1];
        o[2] = f[2];
    } else {
        o[0] = -f[0] / 3.0;
        o[1] = -f[1] / 3.0;
        o[2] = -f[2] / 3.0;
    }
}

struct StepIn {
    const double* coord;
    const double* u;       // disp at the start of the step
    const double* u_pre;   // disp_pre
    const double* velo0;   // non-null before the first step
    double d_time;
    const int* del_step;   // (multi-GPU: the global deletion steps)
    const int* flag;
    const int* conn;
    const double* mass;    // per node, indexed by global node id (multi-GPU: the global array)
    const int* l2g;        // multi-GPU: local -> global node id (null: the ids are global)
    int t;
};

__device__ __forceinline__ int gid(const StepIn& s, int n) { return s.l2g ? s.l2g[n] : n; }

// velocity of node n at the start of step t: the initial one before the first step, else d_disp /
// d_time of the previous step (:628)
__device__ __forceinline__ void velo(const StepIn& s, int n, double v[3]) {
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c)
        v[c] = s.velo0 ? s.velo0[3 * n + c] : (s.u[3 * n + c] - s.u_pre[3 * n + c]) / s.d_time;
}

__device__ __forceinline__ void pos(const StepIn& s, int n, double p[3]) {
#pragma clang fp contract(off)
    for (int c = 0; c < 3; ++c) p[c] = s.coord[3 * n + c] + s.u[3 * n + c];  // position, :653-655
}

__device__ __forceinline__ unsigned long long umin64(unsigned long long a, unsigned long long b) { return a < b ? a : b; }
__device__ __forceinline__ unsigned long long umax64(unsigned long long a, unsigned long long b) { return a > b ? a : b; }

// the hash record of live i-node nd (local id) of pair pr at position p inside the range box r
__device__ __forceinline__ void bin_rec(const StepIn& s, const Range& r, const PairParam& pp, int pr, int nd,
                                        const double p[3], BRec& e) {
#pragma clang fp contract(off)
    for (int d = 0; d < 3; ++d) e.e.m[d] = hk::cell_index(p[d], r.amn[d], pp.ddiv);
    const int g = gid(s, nd);
    e.e.node = g;
    e.e.pad = pr;
    for (int d = 0; d < 3; ++d) e.e.p[d] = p[d];
    e.e.next = -1;
    velo(s, nd, e.w.v);
    e.w.mq = s.mass[g / 3];  // diag_M[i] with the node id i (:2592)
}

// entry `slot` of the bucket list into bucket b of search sequence seq: pushed onto the bucket's
// chain (the order of a bucket's entries is the atomics' and irrelevant: every event's force is
// summed order-independently)
__device__ __forceinline__ void bucket_push(unsigned long long* head, int b, unsigned seq, int slot, BEnt e, BVel w,
                                            BEnt* blist, BVel* bvel) {
    const unsigned long long old = atomicExch(&head[b], ((unsigned long long)seq << 32) | (unsigned)slot);
    e.next = (unsigned)(old >> 32) == seq ? (long long)(unsigned)old : -1LL;
    blist[slot] = e;
    bvel[slot] = w;
}

// wave-aggregated append: one atomic per wave; every lane of the wave must call it
__device__ __forceinline__ unsigned wave_append(unsigned int* ctr, bool pred) {
    const unsigned long long m = __ballot(pred);
    const int lane = (int)(threadIdx.x & 63);
    const int leader = m ? __ffsll((long long)m) - 1 : 0;
    unsigned base = 0;
    if (m && lane == leader) base = atomicAdd(ctr, (unsigned)__popcll(m));
    base = __shfl(base, leader);
    return base + (unsigned)__popcll(m & ((1ULL << lane) - 1ULL));
}

// Same with one global atomic per BLOCK (the per-wave atomics of a large grid on one counter
// serialise): every thread of the block must call it (block-uniform trip counts).
__device__ __forceinline__ unsigned block_append(unsigned int* ctr, bool pred, unsigned* s_ctl) {
    if (threadIdx.x == 0) s_ctl[0] = 0;
    __syncthreads();
    const unsigned long long m = __ballot(pred);
    const int lane = (int)(threadIdx.x & 63);
    const int leader = m ? __ffsll((long long)m) - 1 : 0;
    unsigned off = 0;
    if (m && lane == leader) off = atomicAdd(&s_ctl[0], (unsigned)__popcll(m));
    off = __shfl(off, leader);
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[1] = s_ctl[0] ? atomicAdd(ctr, s_ctl[0]) : 0u;
    __syncthreads();
    return s_ctl[1] + off + (unsigned)__popcll(m & ((1ULL << lane) - 1ULL));
}

// The same for two counts per thread packed in one 64-bit value (low and high 32 bits; a block's
// sums stay below 2^32 each), appended to one 64-bit counter with one atomic per block: the
// thread's first slots, packed (every thread of the block calls it)
__device__ __forceinline__ unsigned long long block_append2(unsigned long long* ctr, unsigned long long v,
                                                            unsigned long long* s_ctl) {
    if (threadIdx.x == 0) s_ctl[0] = 0;
    __syncthreads();
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long x = v;  // wave inclusive scan
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o);
        if (lane >= o) x += y;
    }
    unsigned long long woff = 0;
    const unsigned long long wtot = __shfl(x, 63);
    if (lane == 63 && wtot) woff = atomicAdd(&s_ctl[0], wtot);
    woff = __shfl(woff, 63);
    __syncthreads();
    if (threadIdx.x == 0) s_ctl[1] = s_ctl[0] ? atomicAdd(ctr, s_ctl[0]) : 0ULL;
    __syncthreads();
    return s_ctl[1] + woff + x - v;
}

// Prefix of 64 shard counters (each clamped to the shard capacity) in LDS, one lane per shard of
// wave 0 (one load and a wave scan, not 64 dependent loads on one thread): s_pre[0..64] = prefix,
// s_pre[65] = some shard overflowed, s_pre[66] = raw total, s_pre[67] = largest shard. Returns the
// clamped total. s_pre holds 68 entries.
__device__ __forceinline__ long long shard_scan(const unsigned int* cnts, long long shard_cap, unsigned* s_pre) {
    if (threadIdx.x < 64) {
        const int q = (int)threadIdx.x;
        const unsigned v = cnts[q * kShardStride];
        const unsigned cl = (long long)v < shard_cap ? v : (unsigned)shard_cap;
        unsigned x = cl, raw = v, mx = v;
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned y = __shfl_up(x, o);
            if (q >= o) x += y;
            raw += __shfl_xor(raw, o);
            mx = max(mx, __shfl_xor(mx, o));
        }
        s_pre[q] = x - cl;
        const bool over = __any((long long)v > shard_cap);
        if (q == 63) {
            s_pre[64] = x;
            s_pre[65] = over ? 1u : 0u;
            s_pre[66] = raw;
            s_pre[67] = mx;
        }
    }
    __syncthreads();
    return s_pre[64];
}

// index in shard-prefix order -> slot of the shard buffers
__device__ __forceinline__ long long shard_slot(const unsigned* s_pre, long long shard_cap, long long ev) {
    int lo = 0, hi = kEvShards;  // s_pre[lo] <= ev < s_pre[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((long long)s_pre[mid] <= ev) lo = mid; else hi = mid;
    }
    return (long long)lo * shard_cap + (ev - s_pre[lo]);
}

// Per-candidate triangle record, written by the prefilter: everything of the loop body at
// :2371-2698 that does not depend on the contact point (same expressions as the reference, so the
// same bits), so the per-cell threads start from one load instead of a chain of dependent ones.
struct TriRec {
    double q0[3], c[3], Rmax, n[3], vdet, im[9], kk;
    double vj[3];  // velocity of the triangle's first node (the event's relative velocity, :2580-2582)
    long long mj[3];
    int j0, j1, j2, eleid, pr;  // global node ids; eleid: the (local) element, for the self-contact test
    int hoff, hmask, self;  // the pair's hash region and self-contact flag (no parameter load in the search)
};

__device__ __forceinline__ void tri_geom(int pr, const Range& r, const PairParam& pp, int nd0, int nd1, int nd2,
                                         int ele, const double q0[3], const double q1[3], const double q2[3],
                                         const double vj[3], TriRec& T) {
#pragma clang fp contract(off)
    const double cx = (q0[0] + q1[0] + q2[0]) / 3.0, cy = (q0[1] + q1[1] + q2[1]) / 3.0,
                 cz = (q0[2] + q1[2] + q2[2]) / 3.0;
    const double R0 = my3norm(q0[0] - cx, q0[1] - cy, q0[2] - cz);
    const double R1 = my3norm(q1[0] - cx, q1[1] - cy, q1[2] - cz);
    const double R2 = my3norm(q2[0] - cx, q2[1] - cy, q2[2] - cz);
    const double v1x = q1[0] - q0[0], v1y = q1[1] - q0[1], v1z = q1[2] - q0[2];
    const double v2x = q2[0] - q0[0], v2y = q2[1] - q0[1], v2z = q2[2] - q0[2];
    const double L1 = my3norm(v1x, v1y, v1z), L2 = my3norm(v2x, v2y, v2z);
    const double Lmax = fmax(L1, L2);
    double nx = v1y * v2z - v1z * v2y, ny = v1z * v2x - v1x * v2z, nz = v1x * v2y - v1y * v2x;  // my3crossNNz
    const double mag_n = sqrt(nx * nx + ny * ny + nz * nz);
    nx = nx / mag_n;
    ny = ny / mag_n;
    nz = nz / mag_n;
    const double d12 = v1x * v2x + v1y * v2y + v1z * v2z;
    const double S = 0.5 * sqrt(L1 * L1 * L2 * L2 - d12 * d12);
    const double A11 = v1x, A21 = v1y, A31 = v1z, A12 = v2x, A22 = v2y, A32 = v2z, A13 = -nx, A23 = -ny, A33 = -nz;
    // my3SolveAb (:3342-3373): determinant and adjugate do not depend on the point
    T.vdet = (A11 * A22 * A33 + A12 * A23 * A31 + A13 * A21 * A32 - A11 * A23 * A32 - A12 * A21 * A33 -
              A13 * A22 * A31);
    T.im[0] = A22 * A33 - A23 * A32;  // im11
    T.im[1] = A13 * A32 - A12 * A33;  // im12
    T.im[2] = A12 * A23 - A13 * A22;  // im13
    T.im[3] = A23 * A31 - A21 * A33;  // im21
    T.im[4] = A11 * A33 - A13 * A31;  // im22
    T.im[5] = A13 * A21 - A11 * A23;  // im23
    T.im[6] = A21 * A32 - A22 * A31;  // im31
    T.im[7] = A12 * A31 - A11 * A32;  // im32
    T.im[8] = A11 * A22 - A12 * A21;  // im33
    T.kk = pp.young * S / Lmax * pp.kc;  // :2575
    for (int d = 0; d < 3; ++d) {
        T.q0[d] = q0[d];
        T.mj[d] = hk::cell_index(q0[d], r.amn[d], pp.ddiv);
    }
    T.c[0] = cx;
    T.c[1] = cy;
    T.c[2] = cz;
    T.Rmax = fmax(fmax(R0, R1), R2);
    T.n[0] = nx;
    T.n[1] = ny;
    T.n[2] = nz;
    T.j0 = nd0;
    T.j1 = nd1;
    T.j2 = nd2;
    T.eleid = ele;
    T.vj[0] = vj[0];
    T.vj[1] = vj[1];
    T.vj[2] = vj[2];
    T.pr = pr;
    T.hoff = pp.hash_off;
    T.hmask = pp.hash_size - 1;
    T.self = pp.self ? 1 : 0;
}

// The full prefilter test (:2374-2411) of live triangle j of pair pr with range box r (act: a real
// entry; every thread of the block calls it): active element, not entirely on one side of the range
// box along any axis -> candidate record in the block's shard (multi-GPU: a rank's lists hold the
// triangles of its own elements only) and one search item per cell of its neighbourhood that its
// sphere can reach (reach_mask)
__device__ __forceinline__ void tri_test(int bid, const StepIn& s, int j, int pr, const Range& r, bool act,
                                         const int* tri_nodes, const int* tri_ele, const PairParam* par,
                                         unsigned int* ccnt, TriRec* cand, long long cshard_cap, uint2* item,
                                         unsigned long long* s_app) {
#pragma clang fp contract(off)
    // every load issued up front (inactive lanes re-read a real entry)
    const int ele = tri_ele[j];
    const int nd0 = tri_nodes[3 * j], nd1 = tri_nodes[3 * j + 1], nd2 = tri_nodes[3 * j + 2];
    const int fl = s.flag[ele];
    const PairParam pp = par[pr];
    double p0[3], p1[3], p2[3];
    pos(s, nd0, p0);
    pos(s, nd1, p1);
    pos(s, nd2, p2);
    bool keep = act && fl == 1;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        keep &= !(p0[d] < r.mn[d] && p1[d] < r.mn[d] && p2[d] < r.mn[d]);
        keep &= !(p0[d] > r.mx[d] && p1[d] > r.mx[d] && p2[d] > r.mx[d]);
    }
    TriRec T;
    unsigned mask = 0u;
    if (keep) {
        double vj[3];
        velo(s, nd0, vj);
        tri_geom(pr, r, pp, gid(s, nd0), gid(s, nd1), gid(s, nd2), ele, p0, p1, p2, vj, T);
        // (small decks: no items, k_ct_tri32)
        if (item) mask = hk::reach_mask(T.mj, T.c, T.Rmax, r.amn, pp.ddiv);
    }
    const unsigned ni = (unsigned)__popc(mask);
    // the candidate and its items appended with ONE atomic per block (the shard's two counters are
    // one 64-bit word: candidates low, items high)
    const int shard = bid % kCandShards;
    const unsigned long long at = block_append2(
        reinterpret_cast<unsigned long long*>(&ccnt[shard * kShardStride]), (keep ? 1ULL : 0ULL) | (unsigned long long)ni << 32,
        s_app);
    const unsigned slot = (unsigned)at;
    const bool stored = keep && (long long)slot < cshard_cap;
    if (stored) cand[shard * cshard_cap + slot] = T;
    if (ni) {
        const long long icap = kItemsPerCand * cshard_cap;
        uint2* out = item + (long long)shard * icap;
        unsigned it = (unsigned)(at >> 32);
        // (a candidate past its shard fails the step -- kCandOver poisons it -- but its items must
        // still name a real record: the shard's first)
        const unsigned cs = (unsigned)(shard * cshard_cap + (stored ? slot : 0u));
        for (unsigned mm = mask; mm; mm &= mm - 1) {
            const int dc = __ffs(mm) - 1;
            const unsigned b = (unsigned)T.hoff + (hash3(T.mj[0] + (dc % 3 - 1), T.mj[1] + ((dc / 3) % 3 - 1),
                                                         T.mj[2] + (dc / 9 - 1)) & (unsigned)T.hmask);
            if ((long long)it < icap) out[it] = make_uint2(cs, ((unsigned)dc << 27) | b);
            ++it;
        }
    }
}

// triangle prefilter over the live triangles, one per thread: the full test
__device__ __forceinline__ void tri_filter_body(int bid, int nb, const StepIn& s, const int* tri_cnt,
                                                const int* tri_live, const int* tri_pair, const int* tri_nodes,
                                                const int* tri_ele, const PairParam* par,
                                                const unsigned long long* bbox, unsigned int* ccnt, TriRec* cand,
                                                long long cshard_cap, uint2* item) {
    const int n = *tri_cnt;
    __shared__ unsigned long long s_app[2];
    const int tid = (int)threadIdx.x;
    unsigned* tested = &ccnt[(bid % kCandShards) * kShardStride + kTestWord];
    for (int q0 = bid * kB; q0 < n; q0 += nb * kB) {  // block-uniform trip count
        const int q = q0 + tid;
        const int j = tri_live[q < n ? q : n - 1];
        const int pr = tri_pair[j];
        const Range r = pair_range(bbox + 12 * pr);
        const bool act = q < n && !r.empty;
        const unsigned long long m = __ballot(act);
        if ((tid & 63) == 0 && m) atomicAdd(tested, (unsigned)__popcll(m));
        tri_test(bid, s, j, pr, r, act, tri_nodes, tri_ele, par, ccnt, cand, cshard_cap, item, s_app);
    }
}

__device__ __forceinline__ long long ll2(unsigned lo, unsigned hi) {
    return (long long)(((unsigned long long)hi << 32) | lo);
}

// the event shards; block 0 also publishes the totals for the overflow check and the stats
static_assert(kEvShards == 64 && kCandShards == 64, "shard_scan: one wave lane per shard");
__device__ __forceinline__ long long shard_prefix(int bid, unsigned int* ctl, const unsigned int* evs,
                                                  long long shard_cap, unsigned* s_pre) {
    const long long n = shard_scan(evs, shard_cap, s_pre);
    if (bid == 0 && threadIdx.x == 0) {
        ctl[kEv] = s_pre[kEvShards + 2];
        atomicMax(&ctl[kEvMax], s_pre[kEvShards + 2]);
        atomicMax(&ctl[kEvShardMax], s_pre[kEvShards + 3]);
    }
    return n;
}

}  // namespace ck
}  // namespace hkc
