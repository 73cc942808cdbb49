"""The ordered binary tree of the history outputs (hk::PairTree) on the CPU.

The tree under test is the kernels' own: this file compiles hakai-fem_amd/csrc/hakai_pair_tree.hpp,
the header hakai_history.hip and hakai_elem_history.hip include, with a host compiler (no
contraction, kStride = 1) at both item-counter widths the kernels use. n doubles pushed in order and
folded must equal mass_scale_ref.tree_sum -- neighbours first, a subtree without a right sibling
moves up unchanged -- BIT FOR BIT, and the stack never holds more than floor(log2 n) + 1 open
subtrees: the bound the kernels' kHDepthPart, kHDepth and kEDepth static asserts rest on."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from mass_scale_ref import tree_sum
from util import bitwise_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hakai-fem_amd")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC"]
SIZES = list(range(71)) + [255, 256, 257, 1000]

# The harness only pushes and folds; max_depth is the largest number of open subtrees after a push.
SRC = r"""
#include "hakai_pair_tree.hpp"
template <typename Idx>
static double run(const double* v, long long n, int* max_depth) {
    double stk[64];
    hk::PairTree<1, Idx> tree;
    tree.stk = stk;
    *max_depth = 0;
    for (long long i = 0; i < n; ++i) {
        tree.push(v[i]);
        if (tree.depth > *max_depth) *max_depth = tree.depth;
    }
    return tree.fold();
}
extern "C" {
double tree_u32(const double* v, long long n, int* d) { return run<unsigned>(v, n, d); }
double tree_u64(const double* v, long long n, int* d) { return run<unsigned long long>(v, n, d); }
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("pair_tree")
    c, so = d / "pair_tree.cpp", d / "pair_tree.so"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", os.path.join(PKG, "csrc"), "-o", str(so), str(c)], check=True)
    L = ctypes.CDLL(str(so))
    for f in (L.tree_u32, L.tree_u64):
        f.restype = ctypes.c_double
        f.argtypes = [ctypes.c_void_p, ctypes.c_longlong, ctypes.POINTER(ctypes.c_int)]
    return L


def values(n):
    """Values whose order of addition matters (the recipe of test_history_combine_cpu.random_parts):
    magnitudes over 2^-60 .. 2^60, mixed signs, every fifth value cancels its left neighbour exactly."""
    rng = np.random.default_rng(1000 + n)
    v = rng.standard_normal(n) * np.exp2(rng.integers(-60, 61, n))
    v[5::5] = -v[4:-1:5]
    return v


@pytest.mark.parametrize("width", ["u32", "u64"])
def test_tree_is_tree_sum_bit_for_bit(lib, width):
    f = getattr(lib, "tree_" + width)
    order_matters = 0
    for n in SIZES:
        v = values(n)
        depth = ctypes.c_int(-1)
        got = f(v.ctypes.data, n, ctypes.byref(depth))
        want = tree_sum(v)
        assert bitwise_equal(np.float64(got), np.float64(want)), (n, got, want)
        assert depth.value <= (n.bit_length() if n else 0), (n, depth.value)  # floor(log2 n) + 1
        if n > 2:
            left = 0.0
            for x in v:
                left = left + x
            order_matters += not bitwise_equal(np.float64(left), np.float64(want))
    assert order_matters > len(SIZES) // 2  # a left-to-right sum gives other bits: the values tell the orders apart


def test_depth_bound_is_reached(lib):
    """n = 2^k - 1 leaves k open subtrees: the bound is tight, so the check above can fail."""
    for k in range(1, 11):
        n = 2 ** k - 1
        depth = ctypes.c_int(-1)
        lib.tree_u32(values(n).ctypes.data, n, ctypes.byref(depth))
        assert depth.value == k
