// hakai_pair_tree.hpp -- the ordered binary tree every history sum goes through (DESIGN.md "Record
// rings and the ordered tree"): pairs of neighbours, then pairs of pairs; a subtree without a right
// sibling moves up unchanged. One source for the device (hakai_history.hip, hakai_elem_history.hip)
// and for the CPU: tests/test_pair_tree_cpu.py compiles THIS file with a host compiler (kStride = 1)
// and holds it against mass_scale_ref.tree_sum bit for bit. No device types.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_PT_HD __host__ __device__ __forceinline__
#else
#define HK_PT_HD inline
#endif

namespace hk {

// One binary tree over items pushed in order: an item whose index has k trailing one bits closes
// k subtrees. `stk` is the owner's column of an array [depth][kStride] (a thread's column of an LDS
// array); n pushes leave one open subtree per one bit of n, at most floor(log2 n) + 1. Idx counts the items.
template <int kStride, typename Idx>
struct PairTree {
    double* stk;
    int depth = 0;
    Idx idx = 0;
    HK_PT_HD void push(double x) {
#pragma clang fp contract(off)
        for (Idx m = idx; m & Idx(1); m >>= 1) x = stk[(--depth) * kStride] + x;
        stk[(depth++) * kStride] = x;
        ++idx;
    }
    HK_PT_HD double fold() {  // the open subtrees, smallest first into its left neighbour
#pragma clang fp contract(off)
        if (depth == 0) return 0.0;
        double x = stk[(--depth) * kStride];
        while (depth > 0) x = stk[(--depth) * kStride] + x;
        return x;
    }
};

}  // namespace hk
