// hakai_elem_io.hpp -- what both modes of the element kernel (hakai_element.hip) share: the LDS
// layout, one lane's loads from HBM (connectivity, node, Gauss-point state), the write-back and the
// graph-mode step slot. Device code, included by hakai_element.hip only.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "hakai_kernels.hpp"

namespace hk {

constexpr int kLdsStride = 50;       // doubles per element slot: 8 nodes x (X,du) + pad (bank spread)
// Owner-assembly force staging: [element][local node][3] with one pad double per element, so a
// pass's entries reading the same local node of consecutive elements (lane stride 8) hit spread
// banks (stride 24 doubles = 48 dwords put a 32-lane read on 4 banks: 8-way conflicts)
constexpr int kFeStride = 25;
__device__ __forceinline__ int fe_at(int l, int c) { return (l >> 3) * kFeStride + 3 * (l & 7) + c; }
// Pusai table in LDS: 24 doubles per Gauss point padded to 26 (lanes k and k+4 of an element read
// rows 4 x 24 doubles apart: the same bank; 26 keeps the rows 16-byte aligned for 128-bit reads)
constexpr int kPusStride = 26;
// Reference-order mode (hakai_elem_exact.hpp):
constexpr int kXbStride = 74;  // doubles of LDS per element: exchange area [8 nodes][8 lanes] + one scalar row + pad
static_assert(kEPB * kLdsStride * 8 == 12800 && kEPB * kFeStride * 8 == 6400 &&
                  kEPB * kXbStride * 8 + 8 * kPusStride * 8 == 20608,
              "own_slot_cap (hakai_kernels.hpp) assumes these LDS sizes");

// Reference node index (C3D8 order) of the node with sign bits s = (x>0)<<2 | (y>0)<<1 | (z>0).
__device__ __forceinline__ int ref_of_sign(int s) {
    constexpr unsigned kTab = 0u | 4u << 3 | 3u << 6 | 7u << 9 | 1u << 12 | 5u << 15 | 2u << 18 | 6u << 21;
    return (int)((kTab >> (3 * s)) & 7u);
}

// Node sign table delta_mat (v2/HAKAI_j.jl:1900-1907).
__device__ constexpr double kSx[8] = {-1., 1., 1., -1., -1., 1., 1., -1.};
__device__ constexpr double kSy[8] = {-1., -1., 1., 1., -1., -1., 1., 1.};
__device__ constexpr double kSz[8] = {-1., -1., -1., -1., 1., 1., 1., 1.};

// Everything one lane needs from HBM for one element, gathered ahead of the compute.
struct ElemIn {
    int n, fl, mt, fb;   // stage A: local node, element flag, material, force base offset
    double x[3], du[3];  // stage B: this lane's node: position = coord + u, d_disp = u - u_pre
    double cx[3], uu[3], up[3];  // reference-order mode: the node's raw coord, u, u_pre (formed at use)
    double sig[6], eps[6], eqp, ys;
};

// Element arrays are padded to whole 32-element batches; padding elements carry flag 0 (they
// behave like deleted elements), so every load and store below is unconditional: the compiler can
// then count outstanding memory operations exactly and keep prefetches in flight across the
// stores of the previous batch (a conditional store makes its vmcnt accounting fall back to 0).
// EXACT: lane k stores the force of local node k (elem_step_exact); otherwise that of node
// ref_of_sign(k) (elem_step's relative slots).
// Addressing: a wave-uniform base (SGPRs) plus a 32-bit per-lane byte offset, so every access is a
// global_load/store with an SGPR base and one VGPR offset instead of a 64-bit VGPR address per
// array and component (12 Gauss-point components, 3 node arrays: ~60 VGPRs of addresses in the
// element kernel otherwise). The host keeps every element-kernel array below 4 GB
// (hakai_upload_model: nEp <= kMaxElemPerCtx).
template <class T>
__device__ __forceinline__ T* at32(T* base, unsigned bytes) {
    using C = typename std::conditional<std::is_const<T>::value, const char, char>::type;
    return reinterpret_cast<T*>(reinterpret_cast<C*>(base) + bytes);
}

// Orders this wave's LDS accesses around a cross-lane exchange (the 8 lanes of an element write,
// then read each other's values). A wave's LDS operations execute in order, so this only stops the
// compiler from moving LDS accesses across it; restricted to the local address space, it leaves
// the global loads and stores (the pipeline's prefetches, the write-back) free to be scheduled
// across the exchanges.
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront", "local");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront", "local");
}

// CT: connectivity templates (ElemArgs::conn_rec) -- in.n is left to the caller, which loads the
// element's record (conn_rec) and resolves the node in two more steps (conn_off, conn_node).
template <bool EXACT = false, bool CT = false>
__device__ __forceinline__ void load_stage_a(const ElemArgs& a, long long e, int k, ElemIn& in) {
    const unsigned ue = (unsigned)e;
    in.fl = *at32(a.flag, 4u * ue);
    if (!CT) in.n = *at32(a.conn, 32u * ue + 4u * (unsigned)k);
    in.mt = *at32(a.mat, a.mat_stride * ue);  // (stride 0: one material, every lane reads mat[0] = 0)
    const int kn = EXACT ? k : ref_of_sign(k);  // the node whose force lane k ends up with
    in.fb = (int)(24 * e + 3 * kn);
}

// Connectivity templates (hakai_conn_plan.hpp): lane k's node is the element's base node plus entry k
// of the element's offset pattern. Three steps, each a batch apart in k_element_pipe so that none
// waits: the element's 4-B record (the eight lanes of an element read the same word); the offset,
// a dependent load from a table of at most 8 KB that stays in the caches; their sum.
__device__ __forceinline__ int conn_rec(const ElemArgs& a, long long e) {
    return (int)*at32(a.conn_rec, 4u * (unsigned)e);
}
__device__ __forceinline__ int conn_off(const ElemArgs& a, int rec, int k) {
    const int* pat = reinterpret_cast<const int*>(a.conn_rec + a.nEp);
    return *at32(pat, 32u * ((unsigned)rec >> a.conn_bits) + 4u * (unsigned)k);
}
__device__ __forceinline__ int conn_node(const ElemArgs& a, int rec, int off) {
    return (int)((unsigned)rec & ((1u << a.conn_bits) - 1u)) + off;
}

// Gauss-point state accesses: plain, or nontemporal (streamed once per step; keeps the caches for
// the node data and the element forces the nodal kernel reads next)
// (NT bit 0: loads, bit 1: stores)
template <int NT>
__device__ __forceinline__ double gp_ld(const double* p) {
    if (NT & 1) return __builtin_nontemporal_load(p);
    return *p;
}
template <int NT>
__device__ __forceinline__ void gp_st(double* p, double v) {
    if (NT & 2)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// stage B: the lane's node (position = coord + u, d_disp = u - u_pre) and its Gauss-point state
__device__ __forceinline__ unsigned gp_off(long long e, int k) { return 64u * (unsigned)e + 8u * (unsigned)k; }

template <bool ANY_PLASTIC, int NT = 0>
__device__ __forceinline__ void load_gp(const ElemArgs& a, long long e, int k, ElemIn& in) {
    const unsigned go = gp_off(e, k);
#pragma unroll
    for (int c = 0; c < 6; ++c) in.sig[c] = gp_ld<NT>(at32(a.sc[c], go));
#pragma unroll
    for (int c = 0; c < 6; ++c) in.eps[c] = gp_ld<NT>(at32(a.ec[c], go));
    in.eqp = 0.0;
    in.ys = 0.0;
    if (ANY_PLASTIC) {
        in.eqp = gp_ld<NT>(at32(a.eqps, go));
        in.ys = gp_ld<NT>(at32(a.yield, go));
    }
}

__device__ __forceinline__ void load_node(const ElemArgs& a, ElemIn& in) {
    const unsigned no = 24u * (unsigned)in.n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double uc = at32(a.u, no)[c];
        in.x[c] = at32(a.coord, no)[c] + uc;
        in.du[c] = uc - at32(a.u_pre, no)[c];
    }
}

// The same node, raw: the reference-order kernel issues these loads before the previous batch's
// summing pass and forms x and du only where it stores them to LDS.
__device__ __forceinline__ void load_node_raw(const ElemArgs& a, ElemIn& in) {
    const unsigned no = 24u * (unsigned)in.n;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        in.cx[c] = at32(a.coord, no)[c];
        in.uu[c] = at32(a.u, no)[c];
        in.up[c] = at32(a.u_pre, no)[c];
    }
}

template <bool ANY_PLASTIC, int NT = 0>
__device__ __forceinline__ void load_stage_b(const ElemArgs& a, long long e, int k, ElemIn& in) {
    load_node(a, in);
    load_gp<ANY_PLASTIC, NT>(a, e, k, in);
}

// Unconditional write-back of one lane (selects, no branches): its node's force fk, its Gauss
// point's state, the element flag and the deletion log.
// PRESEL: fin/eps/eqp/ys already hold the values to store (the caller selected the previous state
// for inactive elements early, so in.sig/eps need not stay live until here).
// PART: kWbAll every store; kWbState the Gauss-point state, flag and deletion log only; kWbForce the
// node forces only (the state can then be stored before the force pass, freeing its registers).
enum { kWbAll = 0, kWbState = 1, kWbForce = 2 };
template <bool DO_DELETE, bool STORE_TRIAX, bool ANY_PLASTIC, int NT, bool EXACT_NODE = false, bool OWN = false,
          bool PRESEL = false, int PART = kWbAll>
__device__ __forceinline__ void elem_writeback(const ElemArgs& a, long long e, int k, const ElemIn& in, bool active,
                                               bool kill, const double (&fk)[3], const double (&fin)[6],
                                               const double (&eps)[6], double eqp, double ys, double tri,
                                               double* sfe = nullptr) {
    const unsigned go = gp_off(e, k);
    if (PART != kWbState && OWN) {  // owner-computed assembly: the batch's forces go to LDS [element][local node][3]
        double* fo = sfe + (threadIdx.x >> 3) * kFeStride + 3 * (EXACT_NODE ? k : ref_of_sign(k));
        fo[0] = active ? fk[0] : 0.0;
        fo[1] = active ? fk[1] : 0.0;
        fo[2] = active ? fk[2] : 0.0;
    }
    if (PART != kWbState && (!OWN || STORE_TRIAX)) {  // fe; with owner assembly only on a call's last step (Q / Qe downloads, mode switches)
        double* fg = at32(a.fe, 8u * (unsigned)in.fb);
        fg[0] = active ? fk[0] : 0.0;
        fg[1] = active ? fk[1] : 0.0;
        fg[2] = active ? fk[2] : 0.0;
    }
    if (PART == kWbForce) return;
    // deletion zeroes stress/strain (:742-756); inactive elements keep their state
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        gp_st<NT>(at32(a.sc[c], go), kill ? 0.0 : (PRESEL || active ? fin[c] : in.sig[c]));
        gp_st<NT>(at32(a.ec[c], go), kill ? 0.0 : (PRESEL || active ? eps[c] : in.eps[c]));
    }
    if (ANY_PLASTIC) {
        gp_st<NT>(at32(a.eqps, go), PRESEL || active ? eqp : in.eqp);
        gp_st<NT>(at32(a.yield, go), PRESEL || active ? ys : in.ys);
    }
    if (STORE_TRIAX) *at32(a.triax, go) = active ? tri : 0.0;
    // (a wave without a deletion and without an element deleted in the previous step changes no flag
    // and logs nothing: it skips both stores; C3 fused -1.0 %, profiles/r05_flag_store_skip_ab.log)
    if (DO_DELETE && __builtin_amdgcn_ballot_w64(kill || in.fl == 2) != 0) {
        *at32(a.flag, 4u * (unsigned)e) = kill ? 2 : (in.fl == 2 ? 0 : in.fl);  // 8 lanes, same value
        // lane 0: the element's deletion step; lanes 1-7 of a killed element: slot nEp+1, "last step
        // with a deletion" (contact rebuilds its live surface lists from it); others: dump slot nEp
        const unsigned di = kill ? (k == 0 ? (unsigned)e : (unsigned)a.nEp + 1u) : (unsigned)a.nEp;
        *at32(a.del_step, 4u * di) = a.step_i;
    }
}

// Pusai table (cal_Pusai_hexa, 192 doubles, built on the host) into LDS.
__device__ __forceinline__ void stage_pusai(const ElemArgs& a, double* s_pus) {
    for (int w = threadIdx.x; w < 192; w += blockDim.x) s_pus[w / 24 * kPusStride + w % 24] = a.pusai[w];
}

// Graph mode (hipGraph of two steps, hakai_step): the step number is not a kernel argument but a
// device counter. Every kernel of a step reads slot 1-p (the previous step's number) and adds 1;
// the element kernel, the last of the step, stores that number into slot p, which the next step
// reads. A divergent lane stores it, so it is an ordinary vector store.
__device__ __forceinline__ void graph_step(ElemArgs& a) {
    if (a.t_rd) {
        const double tp = *a.t_rd;
        a.step_i = (int)tp + 1;
        if (a.t_wr && blockIdx.x == 0 && threadIdx.x == 0) *a.t_wr = tp + 1.0;
    }
}

}  // namespace hk
