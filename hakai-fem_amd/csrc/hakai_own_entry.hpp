// hakai_own_entry.hpp -- the 16-byte list entry of owner-computed assembly, stated once. The planner
// (hakai_own_plan.cpp) packs entries, the element kernel (hakai_own_pass.hpp own_load, own_lane,
// own_entry) and the CPU replay (tools/own_plan_check.cpp) read them, all through this file: no
// other file holds a shift or a mask of the format. Plain ints, no device types: nothing in here
// needs hip_runtime.h.
//
// One entry is four ints (x, y, z, w; the kernel loads them as one int4):
//   x = target (node for ACC entries, first row for EXP), y = slot bits 0-9 | flags << 10 | n << 14 |
//   lane7 << 18 | kOwnRound2 (bit 27, set in the kernel) | slot bit 10 << 28,
//   z | w << 32 = lanes 0-6, 9 bits each; a lane is ((schedule position of the element's batch -
//   the super-batch's first position) * 32 + element % 32) * 8 + local node, in ascending element
//   order.
// n (0-8) is the number of lanes in use. An ACC entry continues node `target`'s running sum in LDS
// slot `slot` (INIT: from 0.0, FIN: store it to own_q); an EXP entry copies up to kOwnExpRows
// contributions to rows target + j * slot (its slot field is the row stride); a NOP entry pads.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_HD __host__ __device__ __forceinline__
#else
#define HK_HD static inline
#endif

namespace hk {

enum { kOwnInit = 1, kOwnFin = 2, kOwnExp = 4, kOwnNop = 8 };  // flags
constexpr int kOwnExpRows = 4;      // contributions per EXP entry
constexpr int kOwnSlotsMax = 2048;  // 11-bit slot ids
// Set by the kernel in its register copy of y (own_load): the super-batch has a second round of
// entries. The planner never writes it and no reader sees it.
constexpr int kOwnRound2 = 1 << 27;

HK_HD constexpr int own_pack_y(int slot, int flags, int n, int lane7) {
    return (int)(((unsigned)slot & 1023u) | (unsigned)flags << 10 | (unsigned)n << 14 | (unsigned)lane7 << 18 |
                 ((unsigned)slot & 1024u) << 18);
}
static_assert((own_pack_y(kOwnSlotsMax - 1, 15, 15, 511) & kOwnRound2) == 0, "kOwnRound2 overlaps a packed field");

HK_HD void own_pack(int target, int slot, int flags, int n, const int lanes[8], int w[4]) {
    unsigned long long lo = 0;
    for (int q = 0; q < 7; ++q) lo |= (unsigned long long)lanes[q] << (9 * q);
    w[0] = target;
    w[1] = own_pack_y(slot, flags, n, lanes[7]);
    w[2] = (int)(unsigned)(lo & 0xffffffffu);
    w[3] = (int)(unsigned)(lo >> 32);
}

HK_HD int own_slot(int y) { return (y & 1023) | ((y >> 18) & 1024); }
HK_HD int own_flags(int y) { return (y >> 10) & 15; }
HK_HD int own_n(int y) { return (y >> 14) & 15; }
HK_HD int own_lane(int y, int z, int w, int j) {
    const unsigned long long lo = (unsigned long long)(unsigned)z | ((unsigned long long)(unsigned)w << 32);
    return j < 7 ? (int)((lo >> (9 * j)) & 511) : (int)(((unsigned)y >> 18) & 511);  // bits 18-26
}

// Template form (hakai_own_plan.hpp): the entries of a super-batch are stored with relative targets
// (ACC: node - tbase, EXP: row - rbase; an ACC entry's slot field is 0, its slot is node mod P) and
// shared between super-batches whose relative lists are equal. One 16-byte header per super-batch:
//   x = offset of its entries in the template store, y = entry count | (tbase mod P) << 16,
//   z = tbase, w = rbase.
constexpr int kOwnTplMinEntries = 1 << 16;  // shorter plain lists (1 MiB) sit in L2 whole: the form is kept whatever it stores

HK_HD void own_pack_hdr(int toff, int count, int sofs, int tbase, int rbase, int h[4]) {
    h[0] = toff;
    h[1] = (int)((unsigned)count | (unsigned)sofs << 16);
    h[2] = tbase;
    h[3] = rbase;
}
HK_HD int own_hdr_count(int y) { return y & 0xffff; }
HK_HD int own_hdr_sofs(int y) { return (int)((unsigned)y >> 16); }
// node mod P of a relative ACC target: rel < 2 P and sofs = tbase mod P < P, so two conditional
// subtractions (the unsigned minimum takes the difference exactly when it does not wrap)
HK_HD int own_tpl_slot(int rel, int sofs, int P) {
    unsigned s = (unsigned)rel + (unsigned)sofs, t = s - (unsigned)P;
    s = t < s ? t : s;
    t = s - (unsigned)P;
    return (int)(t < s ? t : s);
}

}  // namespace hk
