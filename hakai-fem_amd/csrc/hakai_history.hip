// hakai_history.hip -- per-step history output: per node set, the sums of internal and external
// force, momentum, kinetic energy, displacement, and the accumulated internal, external and
// constraint work (include/hakai_hip.h hakai_history_*, DESIGN.md "History output").
//
//   k_history_part    one block per group of kHGroup 256-node chunks: every node's 16 terms, the
//                     chunk sums (wave butterfly, then the four waves through LDS), the group's
//                     chunks combined pairwise in chunk order; also stores du_prev
//   k_history_finish  one block: the group partials combined pairwise in group order, the works
//                     added to their accumulators, the record written
//   k_history_one     both in one launch: one block walks every group (small decks)
//
// The launch boundary is the only hand-off between blocks: no atomics, no flags, no spins. Every
// sum is a node of the one binary tree over the node numbers (hakai_pair_tree.hpp), so its bits depend
// on the node numbering and the sets alone, not on the launch form or the grid. The sets' mask and the
// record ring on the host are hakai_record_sets.hpp's and hakai_record_ring.hpp's.
// Compiled without contraction: Q is formed with k_nodal's additions in k_nodal's order.
// On a rank (a context with a communicator) the same tree runs over the rank's local numbering and
// over the nodes it owns: a node shared with the rank below counts nowhere, and at a node shared
// with the rank above Q is the cross-rank sum the interface fix consumed (hist_q_up). Nothing is
// exchanged; hakai_history_combine (host) adds the ranks' records in rank order.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_history.hpp"
#include "hakai_internal.hpp"
#include "hakai_kernels.hpp"
#include "hakai_pair_tree.hpp"
#include "hakai_record_ring.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace hk {

constexpr int kHB = 256;                                // nodes per chunk = threads per block
constexpr int kHGroup = 8;                              // chunks per group (one block of k_history_part)
constexpr int kHF = HAKAI_HISTORY_FIELDS;               // values per set
constexpr int kHMaxS = HAKAI_HISTORY_MAX_SETS + 1;      // set 0 (every node) + the caller's
constexpr int kHDepthPart = 4;                          // open subtrees while a group's chunks are combined
constexpr int kHDepth = 24;                             // ... while up to 2^23 group partials are
constexpr unsigned kHNotOwned = 0x8000u;                // HistArgs::set: bits 0-14 are the caller's sets
constexpr unsigned kHUp = 0x80u;                        // HistArgs::presc: bits 0-2 are the dofs
static_assert(kHF == 16 && kHMaxS * kHF <= kHB, "one thread per (set, field) in a block");
static_assert(HAKAI_HISTORY_MAX_SETS <= 15, "the not-owned mark takes bit 15 of the set mask");
static_assert((1 << (kHDepthPart - 1)) >= kHGroup, "stack of the group's chunk tree");

struct HistArgs {
    NodalArgs na;               // as launch_nodal took it: u = u_k, u_pre_out = u_{k+1} (seed: u_{k-1})
    double* du_prev;            // [3nN] u_k - u_{k-1}; the step stores u_{k+1} - u_k
    const unsigned short* set;  // [nN] bit s-1: the node is in set s (set 0 is every node);
                                // kHNotOwned: a rank's node that the rank below owns (in no set, set 0 included)
    const unsigned char* presc; // [nN] bit c: dof c of the node is prescribed; kHUp: shared with the rank above
    // a rank's interface with the rank above (null / 0 without one): the nodes ascending, each with its
    // position in the exchange buffers; up_sendP is null in a step whose nodal update no fix followed
    const int* up_node;         // [n_up]
    const int* up_slot;         // [n_up]
    const double* up_sendP;     // [n_up][3]
    const double* up_recvC;     // [n_up][nslot][3]
    int n_up, nslot;
    int S;                      // sets, set 0 included
    int seed;                   // 1: the (re)start pass (du_prev, KE_seed, accumulators and count zeroed)
    double* gp;                 // [ngroups][S][16] group partials
    long long nchunks, ngroups;
    double* acc;                // [S][3] W_int, W_ext, W_bc
    double* ke_seed;            // [S]
    double* ring;               // [cap][1 + 16 S]: step k (as int64), then the values
    unsigned long long* count;  // records written since the (re)start
    long long stride, cap;
    const double* t_rd;         // graph mode: the step number is *t_rd + 1 (read on the device), else t
    double t;
};

// A thread's tree (hakai_pair_tree.hpp): `stk` is its column of an LDS array [depth][kHB].
using HistTree = PairTree<kHB, unsigned long long>;

// Q_k of node n from the source launch_nodal selected: k_nodal's additions in k_nodal's order
// (MODE as there: 0 padded table, 1 CSR, 2 uploaded Q, 3 owner-computed sums + rows).
template <int MODE>
__device__ __forceinline__ void hist_q(const NodalArgs& a, long long n, double Q[3]) {
#pragma clang fp contract(off)
    double Q0 = 0.0, Q1 = 0.0, Q2 = 0.0;
    if (MODE == 2) {
        Q0 = a.qbuf[3 * n + 0];
        Q1 = a.qbuf[3 * n + 1];
        Q2 = a.qbuf[3 * n + 2];
    } else if (MODE == 3) {
        Q0 = a.own_q[3 * n + 0];
        Q1 = a.own_q[3 * n + 1];
        Q2 = a.own_q[3 * n + 2];
        const int j0 = a.own_rp[n], j1 = a.own_rp[n + 1];
        for (int j = j0; j < j1; ++j) {
            const long long r = a.own_ridx[j];
            Q0 += a.own_rows[3 * r + 0];
            Q1 += a.own_rows[3 * r + 1];
            Q2 += a.own_rows[3 * r + 2];
        }
    } else if (MODE == 0) {
        const int4 lo = reinterpret_cast<const int4*>(a.inc8)[2 * n];
        const int4 hi = reinterpret_cast<const int4*>(a.inc8)[2 * n + 1];
        const int idx[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double* p = a.fe + idx[j];
            Q0 += p[0];
            Q1 += p[1];
            Q2 += p[2];
        }
    } else {
        const int j0 = a.inc_ptr[n], j1 = a.inc_ptr[n + 1];
        for (int j = j0; j < j1; ++j) {
            const double* f = a.fe + a.inc[j];
            Q0 += f[0];
            Q1 += f[1];
            Q2 += f[2];
        }
    }
    Q[0] = Q0;
    Q[1] = Q1;
    Q[2] = Q2;
}

// Q_k of a node shared with the rank above, in a step whose nodal update the interface fix
// followed: the cross-rank sum the fix consumed, k_fix's (k_fix_own's) additions in their order --
// this rank's partial sum, then the upper rank's contributions one by one. The node's position in
// the exchange buffers comes from a search of the ascending node list (interface nodes only take
// this branch). False if the node is not in the list (the caller then takes the nodal source).
__device__ __forceinline__ bool hist_q_up(const HistArgs& h, long long n, double Q[3]) {
#pragma clang fp contract(off)
    int lo = 0, hi = h.n_up;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (h.up_node[mid] < n) lo = mid + 1;
        else hi = mid;
    }
    if (lo >= h.n_up || h.up_node[lo] != n) return false;
    const int j = h.up_slot[lo];
    double Q0 = h.up_sendP[3 * j + 0], Q1 = h.up_sendP[3 * j + 1], Q2 = h.up_sendP[3 * j + 2];
    const double* r = h.up_recvC + (long long)3 * h.nslot * j;
    for (int s = 0; s < h.nslot; ++s) {
        Q0 += r[3 * s + 0];
        Q1 += r[3 * s + 1];
        Q2 += r[3 * s + 2];
    }
    Q[0] = Q0;
    Q[1] = Q1;
    Q[2] = Q2;
    return true;
}

// The 16 terms of node n (field order of the header) and its new du_prev.
template <int MODE>
__device__ __forceinline__ void hist_node(const HistArgs& h, long long n, double val[kHF]) {
#pragma clang fp contract(off)
    const NodalArgs& a = h.na;
    const double m = a.mass[n], dt = a.dt;
    double uk[3], uo[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        uk[c] = a.u[3 * n + c];
        uo[c] = a.u_pre_out[3 * n + c];
    }
    if (h.seed) {  // du_prev = disp - disp_pre, KE_seed
        double v[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const double du = uk[c] - uo[c];
            h.du_prev[3 * n + c] = du;
            v[c] = du / dt;
        }
        val[9] = 0.5 * m * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
        return;
    }
    double Q[3];
    const unsigned pm = h.presc[n];
    if (!((pm & kHUp) && h.up_sendP && hist_q_up(h, n, Q))) hist_q<MODE>(a, n, Q);
    double v[3], wi[3], we[3], wb = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double f = a.fext ? a.fext[3 * n + c] : 0.0;
        const double du = uo[c] - uk[c], dup = h.du_prev[3 * n + c];
        const double ck = 0.5 * (du + dup);  // the centred increment
        v[c] = du / dt;
        val[c] = Q[c];
        val[3 + c] = f;
        val[6 + c] = m * v[c];
        wi[c] = Q[c] * ck;
        we[c] = f * ck;
        if ((pm >> c) & 1u) {  // the constraint force's work
            const double r = m * (du - dup) / (dt * dt) + Q[c] - f;
            wb += r * ck;
        }
        val[13 + c] = uk[c];
        h.du_prev[3 * n + c] = du;
    }
    val[9] = 0.5 * m * ((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
    val[10] = (wi[0] + wi[1]) + wi[2];
    val[11] = (we[0] + we[1]) + we[2];
    val[12] = wb;
}

// The 16 sums over a wave's 64 lanes in 17 exchanges instead of 96: four halving steps (partners
// 32, 16, 8, 4 lanes apart; a lane keeps half of its values, adds its partner's and hands the
// other half over), then two butterfly steps. Lane l with l % 4 == 0 returns the total of field
// l / 4. Every total is one fixed pairwise tree over the lanes.
__device__ __forceinline__ double wave_sum16(const double v[kHF], int lane) {
#pragma clang fp contract(off)
    double a[8], b[4], c[2];
    bool hi = (lane & 32) != 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) a[j] = (hi ? v[j + 8] : v[j]) + __shfl_xor(hi ? v[j] : v[j + 8], 32, 64);
    hi = (lane & 16) != 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) b[j] = (hi ? a[j + 4] : a[j]) + __shfl_xor(hi ? a[j] : a[j + 4], 16, 64);
    hi = (lane & 8) != 0;
#pragma unroll
    for (int j = 0; j < 2; ++j) c[j] = (hi ? b[j + 2] : b[j]) + __shfl_xor(hi ? b[j] : b[j + 2], 8, 64);
    hi = (lane & 4) != 0;
    double d = (hi ? c[1] : c[0]) + __shfl_xor(hi ? c[0] : c[1], 4, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 1, 64);
    return d;
}

// Group g: its chunks' sums, combined pairwise in chunk order, into gp[g]. lds_w: [4][kHMaxS][16],
// stk: [kHDepthPart][kHB]. Every thread of the block takes every barrier.
template <int MODE>
__device__ __forceinline__ void hist_group(const HistArgs& h, long long g, double* lds_w, double* stk) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int S16 = h.S * kHF;
    HistTree tree;
    tree.stk = stk + tid;
    const long long c0 = g * kHGroup, c1 = c0 + kHGroup < h.nchunks ? c0 + kHGroup : h.nchunks;
    for (long long ch = c0; ch < c1; ++ch) {
        const long long n = ch * kHB + tid;
        double val[kHF];
#pragma unroll
        for (int f = 0; f < kHF; ++f) val[f] = 0.0;
        unsigned member = 0;
        if (n < h.na.nN) {
            // a node the rank below owns counts nowhere, like a lane past nN: a wave of them has
            // nothing to load, and every set's ballot below skips its sums
            const unsigned sv = h.set[n];
            if (!(sv & kHNotOwned)) {
                hist_node<MODE>(h, n, val);
                member = 1u | (sv << 1);
            }
        }
        for (int s = 0; s < h.S; ++s) {
            const bool in = (member >> s) & 1u;
            double* out = lds_w + (w * kHMaxS + s) * kHF;
            if (__ballot(in) == 0ull) {  // wave-uniform: none of the set's nodes in this wave
                if (lane < kHF) out[lane] = 0.0;
                continue;
            }
            double x[kHF];
#pragma unroll
            for (int f = 0; f < kHF; ++f) x[f] = in ? val[f] : 0.0;
            const double tot = wave_sum16(x, lane);
            if ((lane & 3) == 0) out[lane >> 2] = tot;
        }
        __syncthreads();
        if (tid < S16) {  // thread (s, f): the four waves, in wave order
            const double* p = lds_w + tid;
            tree.push((p[0] + p[kHMaxS * kHF]) + (p[2 * kHMaxS * kHF] + p[3 * kHMaxS * kHF]));
        }
        __syncthreads();
    }
    if (tid < S16) h.gp[g * S16 + tid] = tree.fold();
}

// One block: the group partials combined pairwise in group order, R threads per value on aligned
// ranges (subtrees of the same tree for any R), then the accumulators and the record.
// stk: [kHDepth][kHB], red: [kHB].
__device__ __forceinline__ void hist_finish(const HistArgs& h, double* stk, double* red) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    const int S16 = h.S * kHF;
    int R = 1;
    while (2 * R * S16 <= kHB) R *= 2;
    long long P = 1;
    while (P < h.ngroups) P *= 2;
    const long long sub = P / R > 0 ? P / R : 1;  // groups per thread: a power of two
    const int r = tid / S16, j = tid % S16;
    const bool active = tid < R * S16;
    const unsigned long long cnt = *h.count;  // (thread 0 stores the new count after the last barrier)
    double x = 0.0;
    if (active) {
        HistTree tree;
        tree.stk = stk + tid;
        const long long g0 = r * sub, g1 = g0 + sub < h.ngroups ? g0 + sub : h.ngroups;
        // (eight loads in flight: the pushes walk an LDS stack and would wait for each load in turn)
        for (long long g = g0; g < g1; g += 8) {
            double b[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) b[q] = g + q < g1 ? h.gp[(g + q) * S16 + j] : 0.0;
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (g + q < g1) tree.push(b[q]);
        }
        x = tree.fold();
    }
    red[tid] = x;
    for (int st = 1; st < R; st *= 2) {
        __syncthreads();
        // (a right sibling without groups does not exist: its left one moves up unchanged)
        if (active && r % (2 * st) == 0 && (long long)(r + st) * sub < h.ngroups) red[tid] += red[tid + st * S16];
    }
    __syncthreads();
    if (tid >= S16) return;
    const int s = tid / kHF, f = tid % kHF;
    double tot = red[tid];
    if (h.seed) {
        if (f == 9) h.ke_seed[s] = tot;
        if (f >= 10 && f <= 12) h.acc[3 * s + f - 10] = 0.0;
        if (tid == 0) *h.count = 0ull;
        return;
    }
    if (f >= 10 && f <= 12) {  // the works accumulate every step
        tot = h.acc[3 * s + f - 10] + tot;
        h.acc[3 * s + f - 10] = tot;
    }
    const double t = h.t_rd ? *h.t_rd + 1.0 : h.t;
    const long long k = (long long)t - 1;  // the record describes state k
    if (k % h.stride != 0) return;
    double* rec = h.ring + (long long)(cnt % (unsigned long long)h.cap) * (1 + S16);
    rec[1 + tid] = tot;
    if (tid == 0) {
        rec[0] = __longlong_as_double(k);
        *h.count = cnt + 1ull;
    }
}

template <int MODE>
__global__ __launch_bounds__(kHB) void k_history_part(HistArgs h) {
    if (!h.seed && poisoned(h.na.poison)) return;  // block-uniform
    __shared__ double lds_w[4 * kHMaxS * kHF];
    __shared__ double stk[kHDepthPart * kHB];
    hist_group<MODE>(h, blockIdx.x, lds_w, stk);
}

__global__ __launch_bounds__(kHB) void k_history_finish(HistArgs h) {
    if (!h.seed && poisoned(h.na.poison)) return;
    __shared__ double stk[kHDepth * kHB];
    __shared__ double red[kHB];
    hist_finish(h, stk, red);
}

template <int MODE>
__global__ __launch_bounds__(kHB) void k_history_one(HistArgs h) {
    if (!h.seed && poisoned(h.na.poison)) return;
    __shared__ double lds_w[4 * kHMaxS * kHF];
    __shared__ double stk[kHDepth * kHB];
    __shared__ double red[kHB];
    for (long long g = 0; g < h.ngroups; ++g) hist_group<MODE>(h, g, lds_w, stk);
    __syncthreads();  // the block's own gp stores, read below by other threads
    hist_finish(h, stk, red);
}

template <int MODE>
static void launch_history_m(const HistArgs& h, bool one, hipStream_t s) {
    if (one) {
        hipLaunchKernelGGL((k_history_one<MODE>), dim3(1), dim3(kHB), 0, s, h);
    } else {
        hipLaunchKernelGGL((k_history_part<MODE>), dim3((unsigned)h.ngroups), dim3(kHB), 0, s, h);
        hipLaunchKernelGGL(k_history_finish, dim3(1), dim3(kHB), 0, s, h);
    }
}

static hipError_t launch_history(const HistArgs& h, bool one, hipStream_t s) {
    if (h.na.nN <= 0) return hipSuccess;
    if (h.na.qbuf)  // the order of launch_nodal's choice
        launch_history_m<2>(h, one, s);
    else if (h.na.own_q)
        launch_history_m<3>(h, one, s);
    else if (h.na.inc8)
        launch_history_m<0>(h, one, s);
    else
        launch_history_m<1>(h, one, s);
    return hipGetLastError();
}

}  // namespace hk

// ---------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------
namespace hkc {

// One launch while the chunks are one group (2048 nodes): k_history_part would be a single block
// anyway, and the second launch costs about 1 us per step; from two groups on the groups run side
// by side and two launches win (4096 nodes: 64 against 111 us per step; DESIGN.md "History output").
constexpr long long kHistOneBlockChunks = hk::kHGroup;

struct History {
    int n_sets = 0;
    long long nchunks = 0, ngroups = 0;
    bool need_seed = true;
    DevBuf<double> d_du_prev;
    DevBuf<unsigned short> d_set;
    DevBuf<unsigned char> d_presc;
    DevBuf<double> d_acc, d_ke, d_gp;
    RecordRing ring;
    int n_up = 0;                // a rank: its nodes shared with the rank above, ascending, and their
    DevBuf<int> d_up_node;       // positions in the exchange buffers (hist_q_up)
    DevBuf<int> d_up_slot;
};

void history_destroy(hakai_ctx* c) {
    if (!c->hist) return;
    (void)hipStreamSynchronize(c->stream);
    delete c->hist;
    c->hist = nullptr;
}

bool history_needs_seed(const hakai_ctx* c) { return c->hist && c->hist->need_seed; }

int history_restart(hakai_ctx* c) {
    History* H = c->hist;
    if (!H) return 0;
    H->need_seed = true;
    const int S = H->n_sets + 1;
    HIPCHK(H->ring.restart(c->stream));
    HIPCHK(hipMemsetAsync(H->d_acc, 0, 3 * S * sizeof(double), c->stream));
    HIPCHK(hipMemsetAsync(H->d_ke, 0, S * sizeof(double), c->stream));
    return 0;
}

int history_bc_changed(hakai_ctx* c) {
    History* H = c->hist;
    if (!H) return 0;
    std::vector<int> dof((size_t)c->bc.n);
    if (c->bc.n > 0) HIPCHK(hipMemcpy(dof.data(), c->bc.d_dof, dof.size() * sizeof(int), hipMemcpyDeviceToHost));
    std::vector<unsigned char> pm((size_t)c->nN, 0);
    for (int d : dof) pm[(size_t)d / 3] |= (unsigned char)(1u << (d % 3));
    if (const std::vector<int>* up = comm_up_nodes(c))  // a rank: the nodes whose Q the interface fix forms
        for (int n : *up) pm[(size_t)n] |= (unsigned char)hk::kHUp;
    HIPCHK(hipMemcpyAsync(H->d_presc, pm.data(), pm.size(), hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

static hk::HistArgs hist_args(hakai_ctx* c, const hk::NodalArgs& na, const CommFix* fix = nullptr) {
    const History* H = c->hist;
    hk::HistArgs h;
    std::memset(&h, 0, sizeof h);
    h.na = na;
    h.du_prev = H->d_du_prev;
    h.set = H->d_set;
    h.presc = H->d_presc;
    h.S = H->n_sets + 1;
    h.gp = H->d_gp;
    h.nchunks = H->nchunks;
    h.ngroups = H->ngroups;
    h.acc = H->d_acc;
    h.ke_seed = H->d_ke;
    h.ring = H->ring.d_ring;
    h.count = H->ring.d_count;
    h.stride = H->ring.stride;
    h.cap = H->ring.cap;
    h.up_node = H->d_up_node;
    h.up_slot = H->d_up_slot;
    h.n_up = H->n_up;
    if (fix && fix->ran && fix->n_up == H->n_up && H->n_up > 0) {  // (set_interface is refused while history is on)
        h.up_sendP = fix->up_sendP;
        h.up_recvC = fix->up_recvC;
        h.nslot = fix->nslot;
    }
    return h;
}

static bool hist_one_block(const hakai_ctx* c) {
    return c->hist_one_block == 1 || (c->hist_one_block < 0 && c->hist->nchunks <= kHistOneBlockChunks);
}

int history_seed(hakai_ctx* c, const hk::NodalArgs& na, hipStream_t s) {
    if (!c->hist || !c->hist->need_seed) return 0;
    hk::HistArgs h = hist_args(c, na);
    h.seed = 1;
    HIPCHK(hk::launch_history(h, hist_one_block(c), s));
    c->hist->need_seed = false;
    return 0;
}

int history_step(hakai_ctx* c, const hk::NodalArgs& na, const CommFix& fix, double t, const double* t_rd,
                 hipStream_t s) {
    if (!c->hist) return 0;
    if (fix.ran && fix.n_up != c->hist->n_up)
        return fail(HAKAI_ERR_STATE, "history: the interface changed since history_enable");
    hk::HistArgs h = hist_args(c, na, &fix);
    h.t = t;
    h.t_rd = t_rd;
    HIPCHK(hk::launch_history(h, hist_one_block(c), s));
    return 0;
}

}  // namespace hkc

extern "C" {

int hakai_history_enable(hakai_ctx* c, int32_t n_sets, const int64_t* set_off, const int64_t* set_nodes,
                         int64_t stride, int64_t capacity) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "history_enable before upload_model");
    if (c->comm && !hkc::comm_iface_set(c))  // a rank's node ownership comes from its interface
        return fail(HAKAI_ERR_STATE, "history_enable: a context with a communicator needs hakai_set_interface first "
                    "(an empty interface counts)");
    std::vector<unsigned short> set;
    if (int r = hkc::parse_sets("history_enable", "node", HAKAI_HISTORY_MAX_SETS, c->nN, n_sets, set_off, set_nodes,
                                set))
        return r;
    const int S = n_sets + 1;
    if (int r = hkc::ring_check("history_enable", stride, capacity, 16 * S)) return r;
    // a rank: the nodes shared with the rank below are that rank's (the contact search's owner rule);
    // the nodes shared with the rank above ascending, each with its position in the exchange buffers
    std::vector<int> up_node, up_slot;
    if (c->comm) {
        for (int n : *hkc::comm_dn_nodes(c)) set[(size_t)n] = (unsigned short)hk::kHNotOwned;
        const std::vector<int>& up = *hkc::comm_up_nodes(c);
        std::vector<int> order(up.size());
        for (size_t j = 0; j < up.size(); ++j) order[j] = (int)j;
        std::sort(order.begin(), order.end(), [&](int a, int b) { return up[a] < up[b]; });
        for (int j : order) {
            up_node.push_back(up[j]);
            up_slot.push_back(j);
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hkc::graph_invalidate(c);  // the captured steps change
    hkc::history_destroy(c);
    std::unique_ptr<hkc::History> H(new hkc::History());
    H->n_up = (int)up_node.size();
    H->n_sets = n_sets;
    H->nchunks = (c->nN + hk::kHB - 1) / hk::kHB;
    H->ngroups = (H->nchunks + hk::kHGroup - 1) / hk::kHGroup;
    const size_t nN = (size_t)c->nN, S16 = 16 * (size_t)S;
    hipStream_t st = c->stream;
    HIPCHK(H->d_du_prev.alloc_zero(3 * nN, st));
    HIPCHK(H->d_set.alloc_zero(nN, st));
    HIPCHK(H->d_presc.alloc_zero(nN, st));
    HIPCHK(H->d_acc.alloc_zero(3 * (size_t)S, st));
    HIPCHK(H->d_ke.alloc_zero((size_t)S, st));
    HIPCHK(H->ring.alloc(S16, stride, capacity, st));
    HIPCHK(H->d_gp.alloc_zero((size_t)H->ngroups * S16, st));
    if (H->n_up > 0) {
        HIPCHK(H->d_up_node.alloc_zero(up_node.size(), st));
        HIPCHK(H->d_up_slot.alloc_zero(up_slot.size(), st));
        HIPCHK(hipMemcpyAsync(H->d_up_node, up_node.data(), up_node.size() * sizeof(int), hipMemcpyHostToDevice, st));
        HIPCHK(hipMemcpyAsync(H->d_up_slot, up_slot.data(), up_slot.size() * sizeof(int), hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipMemcpyAsync(H->d_set, set.data(), nN * sizeof(unsigned short), hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));
    c->hist = H.release();
    if (int r = hkc::history_bc_changed(c)) {
        hkc::history_destroy(c);
        return r;
    }
    return 0;
}

int hakai_history_disable(hakai_ctx* c) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    HIPCHK(hipSetDevice(c->device));
    hkc::graph_invalidate(c);
    hkc::history_destroy(c);
    return 0;
}

int hakai_history_count(hakai_ctx* c, int64_t* n_written, int64_t* n_held) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->hist) return fail(HAKAI_ERR_STATE, "history is not enabled");
    HIPCHK(hipSetDevice(c->device));
    return c->hist->ring.count(c->stream, n_written, n_held);
}

int hakai_history_read(hakai_ctx* c, int64_t first, int64_t n, int64_t* steps, double* values, double* ke_seed) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->hist) return fail(HAKAI_ERR_STATE, "history is not enabled");
    HIPCHK(hipSetDevice(c->device));
    const hkc::History* H = c->hist;
    if (int r = H->ring.read(c->stream, "history_read", first, n, steps, values)) return r;
    if (ke_seed) {
        HIPCHK(hipMemcpyAsync(ke_seed, H->d_ke, (H->n_sets + 1) * sizeof(double), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
    }
    return 0;
}

}  // extern "C"
