// hakai_own_pass.hpp -- the summing pass of owner-computed assembly inside the persistent element
// kernel: entry and header loads, one entry's additions, the pass behind its LDS barrier. Device
// code, included by hakai_element.hip only.
#pragma once
#include "hakai_elem_io.hpp"

namespace hk {

// ---------------------------------------------------------------------------------------------
// Owner-computed assembly (ElemArgs::own). The block sums node forces per SUPER-BATCH of OS
// consecutive batches of its range (the last one may be shorter), one 16-B entry per thread
// (format: hakai_own_entry.hpp).
// An ACC entry continues node `target`'s running sum in LDS slot `slot` (INIT: from 0.0, the nodal
// gather's own start) with the super-batch's contributions in element order; FIN stores the sum to
// own_q (the node's Q, or its prefix partial when later blocks hold more incidences); EXP copies one
// up to kOwnExpRows contributions (of any nodes) unchanged to consecutive own_rows. Stores are issued
// unconditionally (unused ones to a per-block dump line, which a wave's lanes share) so the loads of
// the pipeline stay in flight across the pass. The force staging is double-buffered by super-batch, so one barrier per super-batch suffices.
// ---------------------------------------------------------------------------------------------
// LDS running sums per block: what two blocks per CU leave (own_slot_cap, up to 2048), sized per
// launch to what the lists use (ElemArgs::own_slots, dynamic LDS next to the staged materials)
// batches per super-batch: 2, or 1 for meshes whose 64-element super-batches need more than 512
// entries; the host picks (hakai_own_plan.cpp own_choose), the kernel is instantiated for both

// LDS-only barrier: the pipeline's global prefetches stay in flight.
__device__ __forceinline__ void lds_barrier() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// The thread's entry of super-batch b, prefetched a batch ahead; kOwnRound2 in .y (a bit the list's
// encoding leaves free) marks a super-batch with a second round of entries, so the pass itself loads
// nothing unless that round exists (a load inside the pass waits for every prefetch issued before it).
__device__ __forceinline__ int4 own_load(const ElemArgs& a, long long b) {
    const int o0 = a.own_off[b], o1 = a.own_off[b + 1];
    const int idx = o0 + (int)threadIdx.x;
    int4 en = a.own_list[idx < o1 ? idx : a.own_nop];
    en.y |= (o1 - o0 > kBlock) ? kOwnRound2 : 0;
    return en;
}

// Template form (ElemArgs::own_hdr, hakai_own_plan.hpp): the super-batch's header is block-uniform
// and is loaded one stage before its entries (with load_stage_a of the batch after), so the entry
// load, which needs the header's offset and count, keeps its place one batch ahead and waits for
// nothing that is still far away. The entries are shared between super-batches and stay in L2.
//
// The header is read through the constant address space, i.e. with a scalar load into SGPRs: the
// headers are written by the host before the launch and by nothing else, the index is the same for
// the whole block, and a vector load would hold four VGPRs per header in flight (three headers are
// live: the kernel has none to spare in reference-order mode) and count against vmcnt.
__device__ __forceinline__ int4 own_hdr_load(const ElemArgs& a, long long b) {
    typedef const int __attribute__((address_space(4))) * ConstInt;
    const ConstInt p = (ConstInt)(unsigned long long)(a.own_hdr + b);
    return make_int4(p[0], p[1], p[2], p[3]);  // (one s_load_dwordx4)
}

__device__ __forceinline__ int4 own_load_tpl(const ElemArgs& a, int4 h) {
    const int cnt = own_hdr_count(h.y);
    int4 en = a.own_list[(int)threadIdx.x < cnt ? h.x + (int)threadIdx.x : a.own_nop];
    en.y |= (cnt > kBlock) ? kOwnRound2 : 0;
    return en;
}

__device__ __forceinline__ int own_lane(int4 en, int j) { return own_lane(en.y, en.z, en.w, j); }

// h: the super-batch's header (TPL only): targets are relative to its bases, an ACC entry's slot is
// node mod own_slots (own_tpl_slot)
template <bool TPL>
__device__ __forceinline__ void own_entry(const ElemArgs& a, int4 en, int4 h, const double* s_fe, double* s_part) {
#pragma clang fp contract(off)
    const int flags = own_flags(en.y), n = own_n(en.y);
    int slot = own_slot(en.y);
    if (TPL) {
        if (!(flags & (kOwnExp | kOwnNop))) slot = own_tpl_slot(en.x, own_hdr_sofs(h.y), a.own_slots);
        en.x += (flags & kOwnExp) ? h.w : h.z;
    }
    double* dump = a.own_dump + 8 * (long long)blockIdx.x;
    double v[3];
    if (flags & (kOwnExp | kOwnNop)) {  // EXP: up to kOwnExpRows contributions -> rows target + j * stride
        // (stride: the entry's group of EXP entries in this wave, in the slot field; consecutive
        // lanes write consecutive rows, hakai_own_plan.cpp own_plan)
#pragma unroll
        for (int j = 0; j < kOwnExpRows; ++j) {
            const int l = own_lane(en, j);
            double* dst = ((flags & kOwnExp) && j < n) ? a.own_rows + 3 * ((long long)en.x + (long long)j * slot) : dump;
#pragma unroll
            for (int c = 0; c < 3; ++c) dst[c] = s_fe[fe_at(l, c)];
        }
        return;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = (flags & kOwnInit) ? 0.0 : s_part[3 * slot + c];
    for (int j = 0; j < n; ++j) {
        const int l = own_lane(en, j);
#pragma unroll
        for (int c = 0; c < 3; ++c) v[c] += s_fe[fe_at(l, c)];
    }
    if (!(flags & kOwnFin)) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s_part[3 * slot + c] = v[c];
    }
    double* dst = (flags & kOwnFin) ? a.own_q + 3 * (long long)en.x : dump;
#pragma unroll
    for (int c = 0; c < 3; ++c) dst[c] = v[c];
}

// Diagnostic build only (tools/variants.sh with -DHK_DIAG_WAVE, tools/diag_wave.py): per-wave clock
// totals of the persistent kernel -- loop, block-barrier wait, summing pass -- accumulated over launches
// into a device table the tool reads back (hakai_element.hip). Product builds compile none of it.
#ifdef HK_DIAG_WAVE
struct PassClock {
    long long bar = 0, pass = 0, n = 0;
};
#define HK_DIAG_ARG , PassClock& dg
#define HK_DIAG_PASS , dg
#else
#define HK_DIAG_ARG
#define HK_DIAG_PASS
#endif

// One summing pass: the prefetched entry of this thread, then -- only for a super-batch with more
// than kBlock entries (wide cross-sections) -- a second one, loaded here (that pass waits for it).
// Entries of one pass touch distinct LDS slots, so the two rounds need no barrier between them.
template <bool TPL>
__device__ __forceinline__ void own_pass(const ElemArgs& a, int4 en, int4 h, long long sb, const double* s_fe,
                                         double* s_part HK_DIAG_ARG) {
#ifdef HK_DIAG_WAVE
    const long long t0 = clock64();
#endif
    lds_barrier();  // the super-batch's forces are in s_fe, the previous pass is done with s_part
#ifdef HK_DIAG_WAVE
    const long long t1 = clock64();
#endif
    // a wave whose threads hold no entry of this round skips it (wave-uniform: no-op entries only
    // store to the dump line; C3 -0.8 to -1.0 %, C4 -1.0 %, profiles/r05_pass_skip_empty_waves_ab.log)
    int o0, o1;  // the super-batch's entries (TPL: in the template store, from the header)
    if (TPL) {
        o0 = h.x;
        o1 = h.x + own_hdr_count(h.y);
    } else {
        o0 = a.own_off[sb];
        o1 = a.own_off[sb + 1];
    }
    if (o0 + (int)(threadIdx.x & ~63u) < o1) own_entry<TPL>(a, en, h, s_fe, s_part);
    if (en.y & kOwnRound2) {  // block-uniform
        const int idx = o0 + kBlock + (int)threadIdx.x;
        if (o0 + kBlock + (int)(threadIdx.x & ~63u) < o1)
            own_entry<TPL>(a, a.own_list[idx < o1 ? idx : a.own_nop], h, s_fe, s_part);
    }
#ifdef HK_DIAG_WAVE
    const long long t2 = clock64();
    dg.bar += t1 - t0;
    dg.pass += t2 - t1;
    dg.n += 1;
#endif
}

}  // namespace hk
