// hakai_element.hip -- the element kernels of the HAKAI explicit time step for gfx950 (MI355X, CDNA4).
//
// Per step the device runs (DESIGN.md "Kernels"):
//   k_nodal    central difference u_new = f(u, u_pre, Q) per node, Q gathered from the previous
//              step's element forces in ascending element order (= the reference's serial assembly,
//              v2/HAKAI_j.jl:668-675, bit-for-bit) -- replaces :562-567 and :668-675 (hakai_nodal.hip);
//   k_bc       prescribed displacements with amplitude (v2/HAKAI_j.jl:585-617) (hakai_nodal.hip);
//   k_element  fused hex8 B-bar + J2 radial return + internal force + triaxiality + ductile
//              deletion (v2/HAKAI_j.jl:1033-1371, :982-1022, :682-764) (this file).
// d_disp (:625), disp_pre/disp shift (:626-627) and position (:650-652) are never materialised:
// disp/disp_pre are ping-pong buffers and the element kernel forms coord+u and u-u_pre on the fly.
//
// Here: k_element (one batch per block), k_element_pipe (persistent, pipelined, with the owner
// pass), the launch dispatch and the negative-Jacobian diagnostic. The device code they call:
//   hakai_elem_io.hpp     LDS layout, lane loads, write-back, graph-mode step slot
//   hakai_elem_fused.hpp  elem_step          hakai_elem_exact.hpp  elem_step_exact
//   hakai_own_pass.hpp    owner-computed assembly's summing pass
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>

#include "hakai_elem_exact.hpp"
#include "hakai_elem_fused.hpp"
#include "hakai_elem_io.hpp"
#include "hakai_kernels.hpp"
#include "hakai_own_pass.hpp"

namespace hk {

// One batch of 32 elements per block (simple form; small meshes, the literal drop-in).
template <bool DO_DELETE, bool STORE_TRIAX, bool WITH_VOL, bool EXACT>
__global__ __launch_bounds__(kBlock, 2) void k_element(ElemArgs a) {
    __shared__ __attribute__((aligned(16))) double s_nd[kEPB * kLdsStride];
    __shared__ __attribute__((aligned(16))) double s_xb[EXACT ? kEPB * kXbStride : 1];
    __shared__ __attribute__((aligned(16))) double s_pus[EXACT ? 8 * kPusStride : 1];
    const long long vb = xcd_remap(blockIdx.x, gridDim.x);
    if (poisoned(a.poison)) return;  // block-uniform
    graph_step(a);
    const int k = threadIdx.x & 7;
    const int grp = threadIdx.x >> 3;
    if (EXACT) {
        stage_pusai(a, s_pus);
        __syncthreads();
    }
    const long long e = vb * kEPB + grp;
    ElemIn in;
    load_stage_a<EXACT>(a, e, k, in);
    if (EXACT) {
        load_node_raw(a, in);
        load_gp<true>(a, e, k, in);
    } else {
        load_stage_b<true>(a, e, k, in);
    }
#ifdef HK_DIAG_PHASE
    PhaseClock pc;
#endif
    if (EXACT)
        elem_step_exact<DO_DELETE, STORE_TRIAX, true, WITH_VOL>(a, a.mats, e, k, s_nd + grp * kLdsStride,
                                                                s_xb + grp * kXbStride, s_pus, in, nullptr HK_PH_PASS);
    else
        elem_step<DO_DELETE, STORE_TRIAX, true, WITH_VOL>(a, a.mats, e, k, s_nd + grp * kLdsStride, in);
}

// Diagnostic build only (-DHK_DIAG_WAVE, hakai_own_pass.hpp): the per-wave clock table, read back
// through hk_diag_read below.
#ifdef HK_DIAG_WAVE
constexpr int kDiagWaves = 8192, kDiagWords = 8;
__device__ unsigned long long g_diag[kDiagWaves * kDiagWords];
#endif

// Persistent, software-pipelined form: each block walks a contiguous range of batches (XCD-aware),
// issuing the loads of batch b+2 (connectivity, flags) and b+1 (node gathers, Gauss-point state)
// before computing batch b, so HBM latency hides under the FP64 work even at 2 waves per SIMD.
// Material tables are staged in LDS (segment searches hit LDS, not L2).
// TPL: the owner-assembly lists are in template form (compile-time, so neither form pays a branch).
// CT: connectivity templates (conn_rec, conn_off, conn_node), compile-time for the same reason; fused
// kernel only. The record is loaded three batches ahead (stage B needs the node a batch ahead), the
// offset at the top of the next iteration -- the record landed a batch ago, and no store of this
// iteration is older than the load, so waiting for it later waits for nothing else -- and the two
// are added at the end of that iteration, behind the batch's arithmetic and summing pass. Two more
// registers are live across the arithmetic than with conn. The reference-order kernel has none to
// spare: with the record where conn was and the offset loaded behind the arithmetic (the only place
// that costs it no register) the wait for the offset also waits for the batch's state stores, and
// C3 ran 2.3 % slower (profiles/conn_templates_ab.json), so that kernel keeps conn.
template <bool DO_DELETE, bool STORE_TRIAX, bool ANY_PLASTIC, bool LDS_MATS, int NT, bool EXACT, int OS = 0,
          bool TPL = false, bool CT = false>
__global__ __launch_bounds__(kBlock, 2) void k_element_pipe(ElemArgs a) {
    constexpr bool OWN = OS > 0;                 // owner-computed assembly, OS batches per super-batch
    constexpr int kOwnFe = OS * kEPB * kFeStride;  // staged forces per pass (doubles)
    __shared__ __attribute__((aligned(16))) double s_nd[kEPB * kLdsStride];
    __shared__ __attribute__((aligned(16))) double s_fe[OWN ? 2 * kOwnFe : 1];
    // dynamic LDS (sized by the launch, launch_pipe): [own_slots][3] running sums, then the
    // nmat staged materials
    extern __shared__ __attribute__((aligned(16))) double s_dyn[];
    double* s_part = s_dyn;
    DevMat* s_mats = reinterpret_cast<DevMat*>(s_dyn + (OWN ? 3 * a.own_slots : 0));
    __shared__ __attribute__((aligned(16))) double s_xb[EXACT ? kEPB * kXbStride : 1];
    __shared__ __attribute__((aligned(16))) double s_pus[EXACT ? 8 * kPusStride : 1];
    if (poisoned(a.poison)) return;  // block-uniform
    graph_step(a);
    const int k = threadIdx.x & 7;
    const int grp = threadIdx.x >> 3;
    if (LDS_MATS) {
        const int words = a.nmat * (int)(sizeof(DevMat) / sizeof(double));
        const double* src = reinterpret_cast<const double*>(a.mats);
        double* dst = reinterpret_cast<double*>(s_mats);
        for (int w = threadIdx.x; w < words; w += kBlock) dst[w] = src[w];
    }
    if (EXACT) stage_pusai(a, s_pus);
    if (LDS_MATS || EXACT) __syncthreads();
    const DevMat* mats = LDS_MATS ? s_mats : a.mats;
    double* nd8 = s_nd + grp * kLdsStride;
    double* xb = s_xb + (EXACT ? grp * kXbStride : 0);
    const long long nb = a.nEp / kEPB;
    // Batch schedule, as (first, stride, count):
    //  * owner assembly: each block walks a contiguous run of batches, in order (own_plan's partition);
    //  * otherwise each XCD owns a contiguous run and its blocks stride through it together, so the
    //    batches that share a node layer (one element layer apart) are processed close in time on
    //    the same L2 (blocks are dealt round-robin over the 8 XCDs; C3 element reads 2.39 -> 2.20 GB).
    long long first, stride, count;
    if (OWN) {  // the block's run of schedule positions (own_choose: contiguous batches, or row bands)
        first = a.own_bstart[blockIdx.x];
        stride = 1;
        count = a.own_bstart[blockIdx.x + 1] - first;
    } else if (gridDim.x % 8 != 0) {
        first = (long long)blockIdx.x * nb / gridDim.x;
        stride = 1;
        count = ((long long)blockIdx.x + 1) * nb / gridDim.x - first;
    } else {
        const long long x = blockIdx.x & 7, j = blockIdx.x >> 3, per = gridDim.x >> 3;
        const long long r0 = x * nb / 8, r1 = (x + 1) * nb / 8;
        first = r0 + j;
        stride = per;
        count = first < r1 ? (r1 - first + per - 1) / per : 0;
    }
    if (count <= 0) return;  // block-uniform
    // iterations past the end are clamped to the last batch (loaded, never computed)
    auto pos_of = [&](long long i) { return first + (i < count ? i : count - 1) * stride; };
    auto vb_of = [&](long long i) { return OWN ? (long long)a.own_seq[pos_of(i)] : pos_of(i); };
    auto elem_of = [&](long long i) { return vb_of(i) * kEPB + grp; };

#ifdef HK_DIAG_WAVE
    PassClock dg;
    const long long dg_t0 = clock64();
#endif
#ifdef HK_DIAG_PHASE
    PhaseClock pc;
#endif
    ElemIn cur, nxt;
    int4 ent_cur = {0, 0, 0, 0}, ent_nxt = {0, 0, 0, 0};
    load_stage_a<EXACT, CT>(a, elem_of(0), k, cur);
    load_stage_a<EXACT, CT>(a, elem_of(1), k, nxt);
    static_assert(!(CT && EXACT), "connectivity templates: fused kernel only");
    // (CT, at the top of iteration i: cur.n and nxt.n are nodes, rec_nn is the record of batch i + 2.
    // The prologue waits for its loads.)
    int rec_nn = 0;
    if (CT) {
        const int r0 = conn_rec(a, elem_of(0)), r1 = conn_rec(a, elem_of(1));
        cur.n = conn_node(a, r0, conn_off(a, r0, k));
        nxt.n = conn_node(a, r1, conn_off(a, r1, k));
        rec_nn = conn_rec(a, elem_of(2));
    }
    if (!EXACT) load_stage_b<ANY_PLASTIC, NT>(a, elem_of(0), k, cur);
    // (OWN: super-batch of iteration i starts at iteration i - i % OS; its entries are listed under
    // the schedule position of its first batch)
    constexpr int S = OS > 0 ? OS : 1;
    auto sb_of = [&](long long i) { return pos_of((i < count ? i : count - 1) / S * S); };
    // (TPL: headers of the super-batches of iterations i, i + 1, i + 2)
    int4 hdr_cur = {0, 0, 0, 0}, hdr_nxt = {0, 0, 0, 0}, hdr_nn = {0, 0, 0, 0};
    if (OWN && TPL) {
        hdr_cur = own_hdr_load(a, sb_of(0));
        hdr_nxt = own_hdr_load(a, sb_of(1));
        ent_cur = own_load_tpl(a, hdr_cur);
    } else if (OWN) {
        ent_cur = own_load(a, sb_of(0));
    }
    for (long long i = 0; i < count; ++i) {
        ElemIn nn;
        load_stage_a<EXACT, CT>(a, elem_of(i + 2), k, nn);
        int off = 0;  // CT: the offset of nn's lane, in flight over this batch
        if (CT) {
            nn.n = rec_nn;
            rec_nn = conn_rec(a, elem_of(i + 3));
            off = conn_off(a, nn.n, k);
        }
        if (OWN && TPL) hdr_nn = own_hdr_load(a, sb_of(i + 2));
        // (reference-order mode: its longer arithmetic holds more registers, so nothing of the
        // current batch's nodes or Gauss points is loaded a batch ahead -- only connectivity and
        // flags, two batches ahead. The node gathers are issued at the start of the batch and
        // first used by the Jacobian, the Gauss-point state first after the B-bar and strain passes.
        // Measured on C3, one box: 1.090 against 1.120 ms per step with the node gathers a batch ahead;
        // issuing this batch's node and/or Gauss-point loads at the end of the previous batch (before
        // its summing pass) spills and measured 1.18-1.28 against 1.10 ms, profiles/r03_exact_early_loads_ab.log.)
        if (!EXACT) load_stage_b<ANY_PLASTIC, NT>(a, elem_of(i + 1), k, nxt);
        if (OWN) ent_nxt = TPL ? own_load_tpl(a, hdr_nxt) : own_load(a, sb_of(i + 1));
        double* sfe = s_fe + ((i / S) & 1) * kOwnFe + (i % S) * (kEPB * kFeStride);
        if (EXACT) {
#ifdef HK_DIAG_PHASE
            pc.last = clock64();
#endif
            load_node_raw(a, cur);
            load_gp<ANY_PLASTIC, NT>(a, elem_of(i), k, cur);
            HK_PH(pc, 0);
            elem_step_exact<DO_DELETE, STORE_TRIAX, ANY_PLASTIC, false, NT, OWN>(a, mats, elem_of(i), k, nd8, xb, s_pus,
                                                                                 cur, sfe HK_PH_PASS);
        }
        else
            elem_step<DO_DELETE, STORE_TRIAX, ANY_PLASTIC, false, NT, OWN>(a, mats, elem_of(i), k, nd8, cur, sfe);
        if (OWN) {
            // block-uniform branch; the compiler's load accounting is the same on both sides
            // (checked in the ISA: identical vmcnt waits with or without balancing stores)
            if ((i + 1) % S == 0 || i + 1 == count)
                own_pass<TPL>(a, ent_cur, hdr_cur, sb_of(i), s_fe + ((i / S) & 1) * kOwnFe, s_part HK_DIAG_PASS);
            ent_cur = ent_nxt;
            if (TPL) {
                hdr_cur = hdr_nxt;
                hdr_nxt = hdr_nn;
            }
        }
        if (CT) nn.n = conn_node(a, nn.n, off);
        cur = nxt;
        nxt = nn;
    }
#ifdef HK_DIAG_WAVE
    const long long dg_t1 = clock64();
    const unsigned gw = blockIdx.x * (kBlock / 64) + threadIdx.x / 64;
    if ((threadIdx.x & 63) == 0 && gw < (unsigned)kDiagWaves) {
        unsigned long long* d = g_diag + (size_t)kDiagWords * gw;
        atomicAdd(d + 0, (unsigned long long)(dg_t1 - dg_t0));
        atomicAdd(d + 1, (unsigned long long)dg.bar);
        atomicAdd(d + 2, (unsigned long long)dg.pass);
        atomicAdd(d + 3, (unsigned long long)dg.n);
        atomicAdd(d + 4, (unsigned long long)count);
        atomicAdd(d + 5, 1ull);
        atomicExch(d + 6, (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4));  // HW_ID
#ifdef HK_DIAG_PHASE
        unsigned long long* q = g_diag + (size_t)kDiagWords * (kDiagWaves / 2 + gw);
        for (int j = 0; j < 8; ++j) atomicAdd(q + j, (unsigned long long)pc.t[j]);
#endif
    }
#endif
}

#ifdef HK_DIAG_WAVE
extern "C" int hk_diag_reset() {
    void* p = nullptr;
    if (hipGetSymbolAddress(&p, HIP_SYMBOL(g_diag)) != hipSuccess) return -1;
    return hipMemset(p, 0, sizeof(g_diag)) == hipSuccess ? 0 : -1;
}
extern "C" int hk_diag_read(unsigned long long* out, int n) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_diag), sizeof(unsigned long long) * (size_t)std::min(n, kDiagWaves * kDiagWords)) == hipSuccess ? 0 : -1;
}
#endif

// Runtime flags -> template instantiations. sel<Vs...>(v) names a run-time value and the constants
// it can take; with_consts(f, sels...) calls f(std::integral_constant<T, V>{}...) with the constant
// each value equals (no call if a value is none of its constants).
template <class T, T... Vs>
struct Sel {
    T v;
};
static Sel<bool, false, true> sel(bool v) { return {v}; }
template <int... Vs>
static Sel<int, Vs...> sel(int v) {
    return {v};
}
template <class F>
static void with_consts(F&& f) {
    f();
}
template <class F, class T, T... Vs, class... Rest>
static void with_consts(F&& f, Sel<T, Vs...> s, Rest... rest) {
    (void)((s.v == Vs &&
            (with_consts([&](auto... cs) { f(std::integral_constant<T, Vs>{}, cs...); }, rest...), true)) ||
           ...);
}

// The instantiations of k_element_pipe that exist (launch_pipe names no other):
//  * owner assembly (OS batches per summing pass) forces LDS_MATS, and TPL, the lists' template form
//    (own_hdr), applies only with it;
//  * CT, connectivity templates: instantiated for the fused kernel's owner-assembly template variants
//    only, the default path -- it names no reference-order instantiation; every other variant reads
//    the plain array.
constexpr bool pipe_exists(bool lds_mats, bool exact, int os, bool tpl, bool ct) {
    return (os > 0 ? lds_mats : !tpl) && (!ct || (!exact && tpl));
}

static void launch_pipe(const ElemArgs& a, bool do_delete, bool store_triax, unsigned grid, hipStream_t s) {
    const int os = a.own == 1 || a.own == 2 ? a.own : 0;
    const bool lds = os > 0 || a.nmat <= kMaxLdsMats;
    const bool tpl = os > 0 && a.own_hdr;
    const bool ct = !a.exact && tpl && a.conn_rec;
    const size_t dyn = (os > 0 ? 24 * (size_t)a.own_slots : 0) + (lds ? sizeof(DevMat) * (size_t)a.nmat : 0);
    with_consts(
        [&](auto DD, auto ST, auto AP, auto LDS, auto NT, auto EX, auto OS, auto TPL, auto CT) {
            if constexpr (pipe_exists(LDS(), EX(), OS(), TPL(), CT()))
                hipLaunchKernelGGL((k_element_pipe<DD(), ST(), AP(), LDS(), NT(), EX(), OS(), TPL(), CT()>), dim3(grid),
                                   dim3(kBlock), dyn, s, a);
        },
        sel(do_delete), sel(store_triax), sel(a.any_plastic != 0), sel(lds), sel<0, 3>(a.gp_nt ? 3 : 0),
        sel(a.exact != 0), sel<0, 1, 2>(os), sel(tpl), sel(ct));
}

// One batch per block: with_vol selects the single k_element<false, false, true, EXACT>.
static void launch_batch(const ElemArgs& a, bool do_delete, bool store_triax, unsigned grid, hipStream_t s) {
    const bool with_vol = a.vol != nullptr;
    with_consts(
        [&](auto DD, auto ST, auto VOL, auto EX) {
            if constexpr (!VOL() || (!DD() && !ST()))
                hipLaunchKernelGGL((k_element<DD(), ST(), VOL(), EX()>), dim3(grid), dim3(kBlock), 0, s, a);
        },
        sel(!with_vol && do_delete), sel(!with_vol && store_triax), sel(with_vol), sel(a.exact != 0));
}

hipError_t launch_element(const ElemArgs& a, bool do_delete, bool store_triax, hipStream_t s) {
    if (a.nE <= 0) return hipSuccess;
    if (a.exact && !a.pusai) return hipErrorInvalidValue;
    const long long nb = a.nEp / kEPB;
    if (nb <= 0) return hipSuccess;
    if (a.own) {  // owner-computed assembly: persistent kernel only (own_plan sized its lists for it)
        if (a.own > 2 || a.vol || a.pipe_blocks <= 0 || a.nmat > kMaxLdsMats || !(a.own_off || a.own_hdr) || !a.own_list ||
            !a.own_seq || !a.own_bstart || !a.own_q || !a.own_dump || a.own_slots < 1 ||
            a.own_slots > own_slot_cap(a.exact != 0, a.own, a.nmat))
            return hipErrorInvalidValue;
        if (a.own_grid <= 0 || a.own_grid > nb) return hipErrorInvalidValue;  // (own_bstart has grid+1 entries)
        if (a.conn_rec && (a.conn_bits < 0 || a.conn_bits > 31)) return hipErrorInvalidValue;
        launch_pipe(a, do_delete, store_triax, (unsigned)a.own_grid, s);
    } else if (a.pipe_blocks > 0 && !a.vol) {
        launch_pipe(a, do_delete, store_triax, (unsigned)std::min<long long>(nb, a.pipe_blocks), s);
    } else {
        launch_batch(a, do_delete, store_triax, (unsigned)nb, s);
    }
    return hipGetLastError();
}

// Negative-Jacobian diagnostic (the reference prints a warning, v2/HAKAI_j.jl:1736-1739): counts
// Gauss points of active elements with det J < 0 at the current configuration. Off the hot path.
__global__ void k_negjac(ElemArgs a, unsigned long long* count) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= 8 * a.nE) return;
    const long long e = t >> 3;
    const int k = t & 7;
    if (a.flag[e] != 1) return;
    const double g = 1.0 / __builtin_sqrt(3.0);
    const double gz = (k & 4) ? g : -g, et = (k & 2) ? g : -g, tu = (k & 1) ? g : -g;
    double J[3][3] = {{0., 0., 0.}, {0., 0., 0.}, {0., 0., 0.}};
    for (int i = 0; i < 8; ++i) {
        const long long n = a.conn[8 * e + i];
        const double p0 = 0.125 * kSx[i] * (1.0 + et * kSy[i]) * (1.0 + tu * kSz[i]);
        const double p1 = 0.125 * kSy[i] * (1.0 + gz * kSx[i]) * (1.0 + tu * kSz[i]);
        const double p2 = 0.125 * kSz[i] * (1.0 + gz * kSx[i]) * (1.0 + et * kSy[i]);
        for (int c = 0; c < 3; ++c) {
            const double X = a.coord[3 * n + c] + a.u[3 * n + c];
            J[0][c] += p0 * X;
            J[1][c] += p1 * X;
            J[2][c] += p2 * X;
        }
    }
    const double det = J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) +
                       J[0][1] * (J[1][2] * J[2][0] - J[1][0] * J[2][2]) +
                       J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]);
    if (det < 0.0) atomicAdd(count, 1ull);
}

hipError_t launch_negjac(const ElemArgs& a, unsigned long long* count, hipStream_t s) {
    if (a.nE <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_negjac, dim3((unsigned)((8 * a.nE + 255) / 256)), dim3(256), 0, s, a, count);
    return hipGetLastError();
}

}  // namespace hk
