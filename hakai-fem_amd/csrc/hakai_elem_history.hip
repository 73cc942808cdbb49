// hakai_elem_history.hip -- element-set history: per element set the active and deleted counts,
// current and reference volume, the volume-weighted sums of stress, strain and equivalent plastic
// strain, the elastic strain energy, the plastic dissipation, the largest equivalent plastic strain
// and Mises stress with their elements, and the smallest volume ratio (include/hakai_hip.h
// hakai_elem_history_*, DESIGN.md "Element-set history"). The arithmetic of a Gauss point and of an
// element is hakai_elem_history_gp.hpp, compiled here without contraction.
//
//   k_elem_history_part    one block per group of kEGroup 32-element chunks: every element's 20
//                          values (8 lanes per element, lane k = Gauss point k), per set the wave's 8
//                          elements by shuffles, the block's 4 waves through LDS, the group's chunks
//                          combined pairwise in chunk order
//   k_elem_history_finish  one block: the group partials combined pairwise in group order, the
//                          record written
//   k_elem_history_one     both in one launch: one block walks every group (small meshes)
//
// Evaluated only at record steps, off the other kernels: it reads coord, u_k, the plain
// connectivity, the flags, the deletion steps, the material ids and the Gauss-point state
// (nontemporal: streamed once, it must not evict the node arrays and owner sums the next kernels
// read) and writes only its own buffers. SE + PD is not W_int and eroded energy is not tracked
// (hakai_elem_history_gp.hpp has the reasons).
// The launch boundary is the only hand-off between blocks: no atomics, no flags, no spins. Every sum
// is a node of one binary tree over the element numbers (a wave's 8 elements, the block's 4 waves as
// (w0+w1)+(w2+w3), then chunks and groups of chunks by hakai_pair_tree.hpp), so its bits depend on the
// element numbering and the sets alone, not on the launch form or the grid. Counts, extremes and ids
// are exact and order-free; `>` and `<` let a NaN never win. On a rank the tree runs over the rank's
// local elements; nothing is exchanged, hakai_elem_history_combine (host) combines the ranks' records.
// The sets' masks and the record ring on the host are hakai_record_sets.hpp's and hakai_record_ring.hpp's.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_device.hpp"
#include "hakai_elem_history.hpp"
#include "hakai_elem_history_gp.hpp"
#include "hakai_internal.hpp"
#include "hakai_pair_tree.hpp"
#include "hakai_record_ring.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace hk {

constexpr int kEB = 256;                                   // threads per block
constexpr int kEChunk = 32;                                // elements per chunk: 8 lanes each
constexpr int kEGroup = 8;                                 // chunks per group (one block of the part kernel)
constexpr int kEF = HAKAI_ELEM_HISTORY_FIELDS;             // values per set
constexpr int kEMaxS = HAKAI_ELEM_HISTORY_MAX_SETS + 1;    // set 0 (every element) + the caller's
constexpr int kEW = kEMaxS * kEF;                          // values of a record
constexpr int kESlots = (kEW + kEB - 1) / kEB;             // values a thread combines
constexpr int kEDepth = 4;                                 // open subtrees while a group's chunks are combined
constexpr int kELastSum = 18;                              // fields 0..18 add (the counts exactly)
static_assert(kEF == 24 && kESlots == 2, "field layout, two values per thread");
static_assert((1 << (kEDepth - 1)) >= kEGroup, "stack of the group's chunk tree");
static_assert(kEhSums == 17 && kEhElem == 20, "lane k takes sums k, k + 8 and (lane 0) 16");

struct EhArgs {
    const double* coord;
    const double* u;              // u_k
    const int* conn;              // the plain connectivity [nEp][8]
    const int* flag;
    const int* mat;
    const int* del_step;
    const double* stress;         // SoA: base[c * ld + 8e + k]
    const double* strain;
    const double* eqps;
    long long ld;
    const ElemHistMat* mats;
    const unsigned short* mask;   // [nE] bit s-1: the element is in set s (set 0 is every element)
    long long nE, nchunks, ngroups, elem_offset;
    int S;                        // sets, set 0 included
    double* gp;                   // [ngroups][S][24] group partials (ids local 0-based, +inf: none)
    double* per_elem;             // [nE][20] or null
    double* out;                  // the probe's record [S][24]; null in a step
    double* ring;                 // [cap][1 + 24 S]: step k (as int64), then the values
    unsigned long long* count;    // records written since the (re)start
    long long stride, cap;
    const double* t_rd;           // graph mode: the record's step is *t_rd (read on the device), else t - 1
    double t;
    const int* poison;
};

// Block-uniform: a step the record skips (a poisoned one, one off the stride). The probe never skips.
__device__ __forceinline__ bool eh_skip(const EhArgs& a, long long* k) {
    if (a.out) return false;
    if (poisoned(a.poison)) return true;
    *k = a.t_rd ? (long long)*a.t_rd : (long long)a.t - 1;  // the record describes state k
    return *k % a.stride != 0;
}

__device__ __forceinline__ void eh_take_max(double& v, double& id, double ov, double oid) {
    if (ov > v || (ov == v && oid < id)) {
        v = ov;
        id = oid;
    }
}

// The value of field f for a set without any element.
__device__ __forceinline__ double eh_neutral(int f) {
    return f <= kELastSum ? 0.0 : (f == 19 || f == 21) ? -1.0 : HUGE_VAL;
}

// A thread's tree (hakai_pair_tree.hpp): `stk` is its column of an LDS array [depth][kEB].
using EhTree = PairTree<kEB, unsigned>;

// The largest of the 8 lanes' values and 0 (elem_hist_max8: order-free, a NaN never wins).
__device__ __forceinline__ double eh_max8(double v) {
    double m = v > 0.0 ? v : 0.0, o;
    o = dpp<kDppXor1>(m);
    m = o > m ? o : m;
    o = dpp<kDppXor2>(m);
    m = o > m ? o : m;
    o = dpp<kDppHalfMir>(m);
    m = o > m ? o : m;
    return m;
}

// A lane's control words of a chunk: its element's flag, deletion step and set mask, its node. The
// group loop loads them one chunk ahead, so a chunk's node gathers and state loads start at once
// instead of behind two dependent loads.
struct EhPre {
    int flag, del, n;
    unsigned mask;
};
__device__ __forceinline__ EhPre eh_pre(const EhArgs& a, long long ch) {
    const int tid = threadIdx.x;
    const long long e = ch * kEChunk + (tid >> 3);
    const bool in = e < a.nE;
    const long long ee = in ? e : a.nE - 1;  // lanes past the end take the last element and drop it
    EhPre p = {0, 0, 0, 0u};
    if (a.nE <= 0) return p;  // block-uniform: nothing to address
    p.flag = in ? a.flag[ee] : 0;
    p.del = in ? a.del_step[ee] : 0;
    p.mask = in ? (unsigned)a.mask[ee] : 0u;
    p.n = a.conn[8 * ee + (tid & 7)];
    return p;
}

// Chunk ch: its 32 elements' values and, per set, each wave's partial into lds_w[wave][set][24].
__device__ __forceinline__ void eh_chunk(const EhArgs& a, long long ch, const EhPre& pre, double* lds_w) {
    const int tid = threadIdx.x, k = tid & 7, lane = tid & 63, w = tid >> 6;
    const long long e = ch * kEChunk + (tid >> 3);
    const bool in = e < a.nE;
    const long long ee = in ? e : a.nE - 1;  // lanes past the end compute the last element and drop it
    const bool active = in && pre.flag == 1;
    const bool deleted = in && pre.del != 0;
    const unsigned member = in ? (1u | (pre.mask << 1)) : 0u;
    double v[kEhElem];
#pragma unroll
    for (int j = 0; j < kEhElem; ++j) v[j] = 0.0;
    if (__ballot(active) != 0ull) {  // wave-uniform: a wave of deleted or padding elements loads nothing more
        const long long n = pre.n;
        double Xk[3], xk[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            Xk[c] = a.coord[3 * n + c];
            xk[c] = a.coord[3 * n + c] + a.u[3 * n + c];
        }
        // (one position array at a time: the reference weights first, then the current ones)
        double p[8][3];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[i][c] = __shfl(Xk[c], i, 8);
        const double a0 = elem_hist_absdet(k, p);
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) p[i][c] = __shfl(xk[c], i, 8);
        const double ak = elem_hist_absdet(k, p);
        const long long g = 8 * ee + k;
        double sig[6], eps[6];
#pragma unroll
        for (int c = 0; c < 6; ++c) {
            sig[c] = __builtin_nontemporal_load(a.stress + c * a.ld + g);
            eps[c] = __builtin_nontemporal_load(a.strain + c * a.ld + g);
        }
        const double eq = __builtin_nontemporal_load(a.eqps + g);
        double t[kEhTerms];
        elem_hist_gp(ak, a0, sig, eps, eq, a.mats[a.mat[ee]], t);
#pragma unroll
        for (int j = 0; j < kEhSums; ++j) v[j] = allreduce8(t[j]);
        v[17] = eh_max8(t[17]);
        v[18] = eh_max8(t[18]);
        v[19] = v[0] / v[1];
    }
    if (a.per_elem && in) {  // lane k stores the values k, k + 8, k + 16; an inactive element zeros
#pragma unroll
        for (int j = 0; j < kEhElem; ++j)
            if ((j & 7) == k) a.per_elem[e * kEhElem + j] = active ? v[j] : 0.0;
    }
    // lane k carries the sums k, k + 8 and (lane 0) 16 through the wave's tree
    double m0 = v[0], m1 = v[8];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
        m0 = k == j ? v[j] : m0;
        m1 = k == j ? v[8 + j] : m1;
    }
    const double m2 = v[16];
    const double J = v[19] < HUGE_VAL ? v[19] : HUGE_VAL;  // (a NaN ratio never wins)
    for (int s = 0; s < a.S; ++s) {
        const bool mem = (member >> s) & 1u;
        double* out = lds_w + (w * kEMaxS + s) * kEF;
        if (__ballot(mem) == 0ull) {  // wave-uniform: none of the set's elements in this wave
            if (lane < kEF) out[lane] = eh_neutral(lane);
            continue;
        }
        const bool sel = mem && active;
        const int n_act = __popcll(__ballot(sel && k == 0));
        const int n_del = __popcll(__ballot(mem && deleted && k == 0));
        double x0 = sel ? m0 : 0.0, x1 = sel ? m1 : 0.0, x2 = sel ? m2 : 0.0;
        double ev = sel ? v[17] : -1.0, eid = sel ? (double)e : HUGE_VAL;
        double qv = sel ? v[18] : -1.0, qid = eid;
        double jm = sel ? J : HUGE_VAL;
#pragma unroll
        for (int m = 8; m < 64; m <<= 1) {  // ((e0+e1)+(e2+e3))+((e4+e5)+(e6+e7))
            x0 += __shfl_xor(x0, m);
            x1 += __shfl_xor(x1, m);
            x2 += __shfl_xor(x2, m);
            const double oev = __shfl_xor(ev, m), oeid = __shfl_xor(eid, m);
            const double oqv = __shfl_xor(qv, m), oqid = __shfl_xor(qid, m);
            const double oj = __shfl_xor(jm, m);
            eh_take_max(ev, eid, oev, oeid);
            eh_take_max(qv, qid, oqv, oqid);
            jm = oj < jm ? oj : jm;
        }
        if (lane < 8) {
            out[2 + k] = x0;
            out[10 + k] = x1;
            if (k == 0) {
                out[0] = (double)n_act;
                out[1] = (double)n_del;
                out[18] = x2;
                out[19] = ev;
                out[20] = eid;
                out[21] = qv;
                out[22] = qid;
                out[23] = jm;
            }
        }
    }
}

// Group g: its chunks' partials combined pairwise in chunk order into gp[g]. lds_w: [4][kEMaxS][24],
// stk: [kESlots][kEDepth][kEB]. Every thread of the block takes every barrier. kAhead: the control
// words are loaded one chunk ahead (the part kernel; the one-block kernel, which serves meshes of a
// few chunks, loads them in place and keeps its registers: the same values either way).
template <bool kAhead>
__device__ __forceinline__ void eh_group(const EhArgs& a, long long g, double* lds_w, double* stk) {
    const int tid = threadIdx.x;
    const int W = a.S * kEF;
    EhTree tree[kESlots];
    double rv[kESlots], rid[kESlots];
#pragma unroll
    for (int q = 0; q < kESlots; ++q) {
        tree[q].stk = stk + q * kEDepth * kEB + tid;
        rv[q] = eh_neutral((tid + q * kEB) % kEF);
        rid[q] = HUGE_VAL;
    }
    const long long c0 = g * kEGroup, c1 = c0 + kEGroup < a.nchunks ? c0 + kEGroup : a.nchunks;
    // (chunk c1 of the last group does not exist: the lanes take the last element's words and drop them)
    EhPre next = {0, 0, 0, 0u};
    if (kAhead) next = eh_pre(a, c0 < a.nchunks ? c0 : 0);
    for (long long ch = c0; ch < c1; ++ch) {
        const EhPre cur = kAhead ? next : eh_pre(a, ch);
        if (kAhead) next = eh_pre(a, ch + 1);  // in flight while this chunk is evaluated
        eh_chunk(a, ch, cur, lds_w);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < kESlots; ++q) {  // thread (s, f): the four waves, in wave order
            const int j = tid + q * kEB, f = j % kEF;
            if (j >= W) continue;
            const double* p = lds_w + j;
            if (f <= kELastSum) {
                tree[q].push((p[0] + p[kEW]) + (p[2 * kEW] + p[3 * kEW]));
            } else if (f == 19 || f == 21) {
#pragma unroll
                for (int ww = 0; ww < 4; ++ww) eh_take_max(rv[q], rid[q], p[ww * kEW], p[ww * kEW + 1]);
            } else if (f == 23) {
#pragma unroll
                for (int ww = 0; ww < 4; ++ww) rv[q] = p[ww * kEW] < rv[q] ? p[ww * kEW] : rv[q];
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int q = 0; q < kESlots; ++q) {
        const int j = tid + q * kEB, f = j % kEF;
        if (j >= W) continue;
        double* o = a.gp + g * W + j;
        if (f <= kELastSum) {
            o[0] = tree[q].fold();
        } else if (f == 19 || f == 21) {
            o[0] = rv[q];
            o[1] = rid[q];
        } else if (f == 23) {
            o[0] = rv[q];
        }
    }
}

// One block of any size: the group partials combined pairwise in group order, level by level in place
// (the block's own stores, ordered by its barriers), then the record. Every (pair, value) of a level
// is one independent operation, so the bits do not depend on the number of threads.
__device__ __forceinline__ void eh_finish(const EhArgs& a, long long k) {
    const int tid = threadIdx.x, nt = blockDim.x;
    const int W = a.S * kEF;
    const unsigned long long cnt = a.out ? 0ull : *a.count;  // (thread 0 stores the new count after a barrier)
    for (long long st = 1; st < a.ngroups; st *= 2) {
        const long long np = (a.ngroups + 2 * st - 1) / (2 * st);
        for (long long idx = tid; idx < np * W; idx += nt) {
            const long long p = idx / W, i = 2 * st * p;
            const int j = (int)(idx - p * W), f = j % kEF;
            if (i + st >= a.ngroups) continue;  // no right sibling: the left one moves up unchanged
            double* A = a.gp + i * W + j;
            const double* B = a.gp + (i + st) * W + j;
            if (f <= kELastSum) {
                A[0] = A[0] + B[0];
            } else if (f == 19 || f == 21) {
                double v = A[0], id = A[1];
                eh_take_max(v, id, B[0], B[1]);
                A[0] = v;
                A[1] = id;
            } else if (f == 23) {
                A[0] = B[0] < A[0] ? B[0] : A[0];
            }
        }
        __syncthreads();
    }
    __syncthreads();
    double* rec = a.out ? a.out : a.ring + (long long)(cnt % (unsigned long long)a.cap) * (1 + W) + 1;
    for (int j = tid; j < W; j += nt) {
        const int f = j % kEF;
        double x = a.gp[j];
        if (f == 19 || f == 21) {
            x = a.gp[j + 1] < HUGE_VAL ? x : 0.0;  // a set without active elements
        } else if (f == 20 || f == 22) {
            x = x < HUGE_VAL ? x + (double)(1 + a.elem_offset) : 0.0;  // the global 1-based id
        }
        rec[j] = x;
    }
    if (tid == 0 && !a.out) {
        rec[-1] = __longlong_as_double(k);
        *a.count = cnt + 1ull;
    }
}

__global__ __launch_bounds__(kEB) void k_elem_history_part(EhArgs a) {
    long long k = 0;
    if (eh_skip(a, &k)) return;  // block-uniform
    __shared__ double lds_w[4 * kEW];
    __shared__ double stk[kESlots * kEDepth * kEB];
    eh_group<true>(a, blockIdx.x, lds_w, stk);
}

constexpr int kEFinishB = 1024;  // threads of the combining launch: it streams the group partials alone
__global__ __launch_bounds__(kEFinishB) void k_elem_history_finish(EhArgs a) {
    long long k = 0;
    if (eh_skip(a, &k)) return;
    eh_finish(a, k);
}

__global__ __launch_bounds__(kEB) void k_elem_history_one(EhArgs a) {
    long long k = 0;
    if (eh_skip(a, &k)) return;
    __shared__ double lds_w[4 * kEW];
    __shared__ double stk[kESlots * kEDepth * kEB];
    for (long long g = 0; g < a.ngroups; ++g) eh_group<false>(a, g, lds_w, stk);
    __syncthreads();  // the block's own gp stores, read below by other threads
    eh_finish(a, k);
}

static hipError_t launch_elem_history(const EhArgs& a, bool one, hipStream_t s) {
    if (one) {
        hipLaunchKernelGGL(k_elem_history_one, dim3(1), dim3(kEB), 0, s, a);
    } else {
        hipLaunchKernelGGL(k_elem_history_part, dim3((unsigned)a.ngroups), dim3(kEB), 0, s, a);
        hipLaunchKernelGGL(k_elem_history_finish, dim3(1), dim3(kEFinishB), 0, s, a);
    }
    return hipGetLastError();
}

}  // namespace hk

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
namespace hkc {

// One launch while the chunks are one group (256 elements): the part kernel would be a single block
// anyway and the two forms take the same time; from two groups on the groups run side by side and two
// launches win (512 elements: 81 against 120 us per probe, 4096: 86 against 678; DESIGN.md
// "Element-set history").
constexpr long long kElemHistOneBlockChunks = hk::kEGroup;

struct ElemHistory {
    bool on = false;             // the in-step history is enabled (else only the probe's scratch lives)
    int n_sets = 0;
    long long nchunks = 0, ngroups = 1;
    DevBuf<hk::ElemHistMat> d_mats;
    DevBuf<unsigned short> d_mask;
    DevBuf<double> d_gp;
    RecordRing ring;
    // the probe's own scratch, sized at its calls
    int p_sets = -1;
    DevBuf<unsigned short> d_pmask;
    DevBuf<double> d_pgp, d_pout, d_pelem;
};

void elem_history_destroy(hakai_ctx* c) {
    if (!c->ehist) return;
    (void)hipStreamSynchronize(c->stream);
    delete c->ehist;
    c->ehist = nullptr;
}

int elem_history_restart(hakai_ctx* c) {
    if (!c->ehist || !c->ehist->on) return 0;
    HIPCHK(c->ehist->ring.restart(c->stream));
    return 0;
}

// The state with the model's material table on the device (the first enable or probe after a model).
static int eh_state(hakai_ctx* c) {
    if (c->ehist) return 0;
    std::unique_ptr<ElemHistory> H(new ElemHistory());
    std::vector<hk::ElemHistMat> mats;
    for (const hk::DevMat& m : c->h_mats)
        mats.push_back(hk::elem_hist_mat(m.Dn, m.Do, m.G, m.yield0, m.npp, m.pl_eps, m.Hd));
    HIPCHK(H->d_mats.upload(mats, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));  // (before mats goes)
    H->nchunks = (c->nE + hk::kEChunk - 1) / hk::kEChunk;
    H->ngroups = std::max<long long>(1, (H->nchunks + hk::kEGroup - 1) / hk::kEGroup);
    c->ehist = H.release();
    return 0;
}

static hk::EhArgs eh_args(const hakai_ctx* c) {
    const ElemHistory* H = c->ehist;
    hk::EhArgs a;
    std::memset(&a, 0, sizeof a);
    a.coord = c->d_coord;
    a.u = c->d_u[c->sv.cur];
    a.conn = c->d_conn;
    a.flag = c->d_flag;
    a.mat = c->d_mat;
    a.del_step = c->d_del_step;
    a.stress = c->d_stress;
    a.strain = c->d_strain;
    a.eqps = c->d_eqps;
    a.ld = c->ld;
    a.mats = H->d_mats;
    a.nE = c->nE;
    a.nchunks = H->nchunks;
    a.ngroups = H->ngroups;
    a.elem_offset = c->elem_offset;
    a.poison = c->d_poison;
    return a;
}

static bool eh_one_block(const hakai_ctx* c) {
    return c->ehist_one_block == 1 || (c->ehist_one_block < 0 && c->ehist->nchunks <= kElemHistOneBlockChunks);
}

int elem_history_step(hakai_ctx* c, double t, const double* t_rd, hipStream_t s) {
    const ElemHistory* H = c->ehist;
    if (!H || !H->on) return 0;
    if (!t_rd && ((long long)t - 1) % H->ring.stride != 0) return 0;  // stream mode: the host knows the step
    hk::EhArgs a = eh_args(c);
    a.mask = H->d_mask;
    a.S = H->n_sets + 1;
    a.gp = H->d_gp;
    a.ring = H->ring.d_ring;
    a.count = H->ring.d_count;
    a.stride = H->ring.stride;
    a.cap = H->ring.cap;
    a.t = t;
    a.t_rd = t_rd;
    HIPCHK(hk::launch_elem_history(a, eh_one_block(c), s));
    return 0;
}

}  // namespace hkc

extern "C" {

int hakai_elem_history_enable(hakai_ctx* c, int32_t n_sets, const int64_t* set_off, const int64_t* set_elems,
                              int64_t stride, int64_t capacity) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "elem_history_enable before upload_model");
    std::vector<unsigned short> mask;
    if (int r = hkc::parse_sets("elem_history_enable", "element", HAKAI_ELEM_HISTORY_MAX_SETS, c->nE, n_sets, set_off,
                                set_elems, mask))
        return r;
    const size_t W = (size_t)hk::kEF * (size_t)(n_sets + 1);
    if (int r = hkc::ring_check("elem_history_enable", stride, capacity, (int64_t)W)) return r;
    HIPCHK(hipSetDevice(c->device));
    if (int r = hkc::eh_state(c)) return r;
    hkc::ElemHistory* H = c->ehist;
    hipStream_t st = c->stream;
    // the new buffers first: a failed allocation leaves the previous state in force
    hkc::DevBuf<unsigned short> d_mask;
    hkc::DevBuf<double> d_gp;
    hkc::RecordRing ring;
    HIPCHK(d_mask.upload(mask, st));
    HIPCHK(d_gp.alloc_zero((size_t)H->ngroups * W, st));
    HIPCHK(ring.alloc(W, stride, capacity, st));
    HIPCHK(hipStreamSynchronize(st));  // (before mask goes; the stream's earlier steps are done with the old buffers)
    hkc::graph_invalidate(c);  // the captured steps change
    H->d_mask = std::move(d_mask);
    H->d_gp = std::move(d_gp);
    H->ring = std::move(ring);
    H->n_sets = n_sets;
    H->on = true;
    return 0;
}

int hakai_elem_history_disable(hakai_ctx* c) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    HIPCHK(hipSetDevice(c->device));
    hkc::graph_invalidate(c);
    if (c->ehist && c->ehist->on) {
        HIPCHK(hipStreamSynchronize(c->stream));
        hkc::ElemHistory* H = c->ehist;
        H->on = false;
        H->d_mask.free();
        H->d_gp.free();
        H->ring = hkc::RecordRing();
    }
    return 0;
}

int hakai_elem_history_count(hakai_ctx* c, int64_t* n_written, int64_t* n_held) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->ehist || !c->ehist->on) return fail(HAKAI_ERR_STATE, "element history is not enabled");
    HIPCHK(hipSetDevice(c->device));
    return c->ehist->ring.count(c->stream, n_written, n_held);
}

int hakai_elem_history_read(hakai_ctx* c, int64_t first, int64_t n, int64_t* steps, double* values) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->ehist || !c->ehist->on) return fail(HAKAI_ERR_STATE, "element history is not enabled");
    HIPCHK(hipSetDevice(c->device));
    return c->ehist->ring.read(c->stream, "elem_history_read", first, n, steps, values);
}

int hakai_elem_history_probe(hakai_ctx* c, int32_t n_sets, const int64_t* set_off, const int64_t* set_elems,
                             double* values, double* per_elem) {
    if (!c || !values) return fail(HAKAI_ERR_ARG, "elem_history_probe: null");
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "elem_history_probe without state");
    std::vector<unsigned short> mask;
    if (int r = hkc::parse_sets("elem_history_probe", "element", HAKAI_ELEM_HISTORY_MAX_SETS, c->nE, n_sets, set_off,
                                set_elems, mask))
        return r;
    HIPCHK(hipSetDevice(c->device));
    if (int r = hkc::eh_state(c)) return r;
    hkc::ElemHistory* H = c->ehist;
    hipStream_t st = c->stream;
    const size_t W = (size_t)hk::kEF * (size_t)(n_sets + 1), nE = (size_t)c->nE;
    if (H->p_sets != n_sets) {
        H->p_sets = -1;
        HIPCHK(H->d_pgp.alloc((size_t)H->ngroups * W));
        HIPCHK(H->d_pout.alloc(W));
        H->p_sets = n_sets;
    }
    if (!H->d_pmask) HIPCHK(H->d_pmask.alloc(nE));
    if (per_elem && !H->d_pelem) HIPCHK(H->d_pelem.alloc(nE * hk::kEhElem));
    if (nE > 0) HIPCHK(hipMemcpyAsync(H->d_pmask, mask.data(), nE * sizeof(unsigned short), hipMemcpyHostToDevice, st));
    hk::EhArgs a = hkc::eh_args(c);
    a.mask = H->d_pmask;
    a.S = n_sets + 1;
    a.gp = H->d_pgp;
    a.out = H->d_pout;
    a.per_elem = per_elem ? H->d_pelem.get() : nullptr;
    a.stride = a.cap = 1;
    HIPCHK(hk::launch_elem_history(a, hkc::eh_one_block(c), st));
    HIPCHK(hipMemcpyAsync(values, H->d_pout, W * sizeof(double), hipMemcpyDeviceToHost, st));
    if (per_elem && nE > 0)
        HIPCHK(hipMemcpyAsync(per_elem, H->d_pelem, nE * hk::kEhElem * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));  // (mask lives until here)
    return 0;
}

}  // extern "C"
