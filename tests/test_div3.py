"""The exact element kernel's divisions must equal IEEE division bit for bit. The functions under
test are the kernel's own: this file compiles hakai-fem_amd/csrc/hakai_exact_math.hpp, the header
the element kernel (hakai_elem_exact.hpp) includes, with a host compiler (fma enabled, no contraction) -- there is no copy
of div3 or div_cr here.
  * div3(x) against `x / 3.0` over EVERY binade from 2^-1074 to 2^1023, both signs, 20 000 random
    mantissas per binade and sign, plus +-0, the smallest and largest subnormals and normals,
    multiples of 3 (exact quotients) and the neighbours of every power of two and of 3 * 2^k.
    (The two-operation form of round 6 is one ulp off for a third of the mantissas of the binades
    2^-1021 and 2^-1020; a sample over 2^-200..2^200 could not see that.)
  * div_cr(a, b, RN(1/b)) against `a / b` inside the exponent window the header states
    (kDivCr* there), at every edge of that window: random pairs, pairs whose quotient lies next to
    a rounding midpoint (the hard cases of correct rounding) moved to both ends of the window by
    exact power-of-two scaling, exact quotients and +0 numerators; and on random pairs over the
    range the kernel meets."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-shared", "-fPIC"]

# The harness only calls the header's functions and counts disagreements with IEEE division.
SRC = r"""
#include <stdint.h>
#include <string.h>
#include "hakai_exact_math.hpp"
static inline int same(double a, double b) { return memcmp(&a, &b, sizeof a) == 0; }
extern "C" {
/* number of x with div3(x) != x / 3.0 (bitwise, signed zeros included); *first: index of the first */
int64_t check(const double* x, int64_t n, int64_t* first) {
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
        if (!same(hk::div3(x[i]), x[i] / 3.0) && bad++ == 0) *first = i;
    return bad;
}
/* the same for both signs of every double whose bits are base | (mantissa & mask), n mantissas from
   a splitmix64 stream: one binade (or the subnormals below one bit) without a 2 * n array */
int64_t check_binade(uint64_t base, uint64_t mask, int64_t n, uint64_t seed) {
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i) {
        uint64_t z = (seed += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        for (uint64_t s = 0; s < 2; ++s) {
            const uint64_t b = base | (z & mask) | (s << 63);
            double x;
            memcpy(&x, &b, sizeof x);
            bad += !same(hk::div3(x), x / 3.0);
        }
    }
    return bad;
}
/* pairs with div_cr(a, b, RN(1/b)) != a / b (bitwise); *first: index of the first */
int64_t check_div(const double* a, const double* b, int64_t n, int64_t* first) {
    int64_t bad = 0;
    for (int64_t i = 0; i < n; ++i)
        if (!same(hk::div_cr(a[i], b[i], 1.0 / b[i]), a[i] / b[i]) && bad++ == 0) *first = i;
    return bad;
}
void window(int* w) {
    w[0] = hk::kDivCrMinExpA; w[1] = hk::kDivCrMinExpB; w[2] = hk::kDivCrMaxExpB;
    w[3] = hk::kDivCrMinExpQ; w[4] = hk::kDivCrMaxExpQ;
}
}
"""


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("div3")
    c, so = d / "div3.cpp", d / "div3.so"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", CSRC, "-o", str(so), str(c)], check=True)
    lib = ctypes.CDLL(str(so))
    P, I64, U64 = ctypes.c_void_p, ctypes.c_int64, ctypes.c_uint64
    lib.check.restype = I64
    lib.check.argtypes = [P, I64, ctypes.POINTER(I64)]
    lib.check_binade.restype = I64
    lib.check_binade.argtypes = [U64, U64, I64, U64]
    lib.check_div.restype = I64
    lib.check_div.argtypes = [P, P, I64, ctypes.POINTER(I64)]
    lib.window.argtypes = [ctypes.POINTER(ctypes.c_int * 5)]
    return lib


def _div3_ok(L, x):
    x = np.ascontiguousarray(x, np.float64)
    first = ctypes.c_int64(-1)
    bad = L.check(x.ctypes.data, x.size, ctypes.byref(first))
    assert bad == 0, f"{bad} of {x.size} differ from x/3.0, first x = {float(x[max(first.value, 0)]).hex()}"


def _div_ok(L, a, b, what):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape and a.size > 0
    first = ctypes.c_int64(-1)
    bad = L.check_div(a.ctypes.data, b.ctypes.data, a.size, ctypes.byref(first))
    i = max(first.value, 0)
    assert bad == 0, f"{what}: {bad} of {a.size} differ from a/b, first a = {float(a[i]).hex()}, b = {float(b[i]).hex()}"


N_PER_BINADE = 20_000


def test_div3_equals_ieee_division(L):
    """2^-1074 .. 2^1023: the 52 subnormal 'binades' (leading bit k, k random bits below it) and the
    2046 normal ones, both signs, 20 000 mantissas each."""
    bad = {}
    for k in range(52):                                   # subnormals with leading bit k: [2^(k-1074), 2^(k-1073))
        n = L.check_binade(1 << k, (1 << k) - 1, N_PER_BINADE, 1000 + k)
        if n:
            bad[k - 1074] = n
    for e in range(1, 2047):                              # normal binades 2^(e-1023)
        n = L.check_binade(e << 52, (1 << 52) - 1, N_PER_BINADE, 5000 + e)
        if n:
            bad[e - 1023] = n
    assert not bad, f"div3 != x/3.0 in binades (exponent: count of {2 * N_PER_BINADE}): {bad}"


def test_div3_edges_of_the_whole_range(L):
    tiny, big = np.float64(5e-324), np.finfo(np.float64).max
    mn = np.finfo(np.float64).tiny                         # 2^-1022
    sub_max = np.nextafter(mn, 0)
    edge = np.array([0.0, tiny, 2 * tiny, 3 * tiny, 4 * tiny, 5 * tiny, 6 * tiny, 7 * tiny, sub_max,
                     np.nextafter(sub_max, 0), mn, np.nextafter(mn, 1), 3 * mn, big, np.nextafter(big, 0),
                     big / 3, 1.0, 3.0])
    # every power of two and 3 * 2^k over the whole range, with both neighbours
    p2 = np.ldexp(1.0, np.arange(-1074, 1024))
    p3 = np.ldexp(3.0, np.arange(-1074, 1022))
    near = np.concatenate([p2, np.nextafter(p2, 0), np.nextafter(p2, np.inf)[:-1],
                           p3, np.nextafter(p3, 0), np.nextafter(p3, np.inf)])
    # exact multiples of 3 (up to 53 bits) at every exponent, and their neighbours
    rng = np.random.default_rng(0)
    n = 400_000
    m = (rng.integers(1, 1 << 51, size=n) * 3).astype(np.float64)      # < 2^53: exact
    m3 = np.ldexp(m, rng.integers(-1074, 1023 - 53, size=n))             # integer * 2^k, k >= -1074: exact
    small3 = np.arange(0, 3 * 4096, 3).astype(np.float64) * tiny         # subnormal multiples of 3 * 2^-1074
    allx = np.concatenate([edge, near, m3, np.nextafter(m3, 0), np.nextafter(m3, np.inf), small3])
    assert np.all(np.isfinite(allx))
    _div3_ok(L, np.concatenate([allx, -allx]))


# ---- div_cr ------------------------------------------------------------------------------------

def _window(L):
    w = (ctypes.c_int * 5)()
    L.window(ctypes.byref(w))
    return tuple(w)


def _mant(rng, n):
    """Random doubles in [1, 2) with all 52 mantissa bits random."""
    return (rng.integers(0, 1 << 52, size=n, dtype=np.uint64) | np.uint64(1023 << 52)).view(np.float64)


def _rand_doubles(rng, n, lo, hi, signed=True):
    mant = rng.integers(0, 1 << 52, size=n, dtype=np.uint64)
    expo = rng.integers(1023 + lo, 1023 + hi, size=n, dtype=np.uint64)
    sign = rng.integers(0, 2, size=n, dtype=np.uint64) if signed else np.zeros(n, np.uint64)
    return ((sign << np.uint64(63)) | (expo << np.uint64(52)) | mant).view(np.float64)


def _edge_exponents(w):
    """(ea, eb) pairs on every edge and corner of the window {ea >= A, B0 <= eb <= B1,
    Q0 <= ea - eb <= Q1, ea <= 1023}."""
    A, B0, B1, Q0, Q1 = w
    inside = lambda ea, eb: A <= ea <= 1023 and B0 <= eb <= B1 and Q0 <= ea - eb <= Q1  # noqa: E731
    pts = set()
    for ea in range(A, 1024):
        for eb in (B0, B0 + 1, B1 - 1, B1, ea - Q0, ea - Q0 - 1, ea - Q1, ea - Q1 + 1):
            if inside(ea, eb):
                pts.add((ea, eb))
    for eb in range(B0, B1 + 1):
        for ea in (A, A + 1, 1022, 1023):
            if inside(ea, eb):
                pts.add((ea, eb))
    return np.array(sorted(pts))


def test_div_cr_window_is_the_documented_one(L):
    assert _window(L) == (-969, -1022, 1021, -1021, 1022)


def test_div_cr_edges_of_the_window(L):
    """Random mantissas at every (ea, eb) on the window's boundary: ~9 000 exponent pairs x 300."""
    w = _window(L)
    pts = _edge_exponents(w)
    assert len(pts) > 5000
    rng = np.random.default_rng(1)
    rep = 300
    ea, eb = np.repeat(pts[:, 0], rep), np.repeat(pts[:, 1], rep)
    a = np.ldexp(_mant(rng, ea.size), ea) * rng.choice([-1.0, 1.0], ea.size)
    b = np.ldexp(_mant(rng, eb.size), eb)
    q = a / b
    assert np.all(np.isfinite(q)) and np.all(np.abs(q) >= np.finfo(np.float64).tiny), "the window keeps a/b normal"
    assert np.all(np.abs(1.0 / b) >= np.finfo(np.float64).tiny), "and 1/b"
    _div_ok(L, a, b, "window edges")


def test_div_cr_midpoint_cases_at_both_ends_of_the_window(L):
    """Quotients next to a rounding midpoint: a0 = RN(b0 * (q + ulp(q)/2)) for random q, b0 in [1, 2),
    and a0's neighbours; then a = a0 * 2^sa, b = b0 * 2^sb, exact scalings that keep a/b next to the
    midpoint, placed at the middle and at every end of the window."""
    A, B0, B1, Q0, Q1 = _window(L)
    rng = np.random.default_rng(2)
    m = 200_000
    q, b0 = _mant(rng, m), _mant(rng, m)
    mid = q.astype(np.longdouble) + (np.spacing(q).astype(np.longdouble) / 2)
    a0 = (b0.astype(np.longdouble) * mid).astype(np.float64)           # in [1, 4): exponent 0 or 1
    # (sa, sb): a has exponent sa or sa + 1, b exponent sb
    ends = [(0, 0), (A, 0), (A, B0), (A, A - Q0), (B1 + Q0, B1), (B0 + Q1 - 1, B0), (1022, 1022 - Q1 + 1),
            (1022, B1), (-500, -500 - Q0), (500, 500 - Q1 + 1)]
    for sa, sb in ends:
        for e in (sa, sa + 1):
            assert A <= e <= 1023 and B0 <= sb <= B1 and Q0 <= e - sb <= Q1, (sa, sb)
        b = np.ldexp(b0, sb)
        for da in (0, 1, -1):
            aa = a0 if da == 0 else np.nextafter(a0, da * np.inf)
            keep = (aa >= 1.0) & (aa < 4.0)
            _div_ok(L, np.ldexp(aa[keep], sa), b[keep], f"midpoints at 2^{sa} / 2^{sb}")
            _div_ok(L, -np.ldexp(aa[keep], sa), b[keep], f"midpoints at -2^{sa} / 2^{sb}")


def test_div_cr_equals_ieee_division(L):
    rng = np.random.default_rng(1)
    # random pairs: numerators over the stresses' range, positive divisors (q, V of the kernel)
    n = 10_000_000
    _div_ok(L, _rand_doubles(rng, n, -60, 60), _rand_doubles(rng, n, -30, 30, signed=False), "kernel range")
    n = 4_000_000
    # random pairs over the whole window
    A, B0, B1, Q0, Q1 = _window(L)
    ea = rng.integers(A, 1024, size=n)
    eb = np.clip(ea - rng.integers(Q0, Q1 + 1, size=n), B0, B1)
    ok = (ea - eb >= Q0) & (ea - eb <= Q1)
    a = np.ldexp(_mant(rng, n), ea)[ok] * rng.choice([-1.0, 1.0], int(ok.sum()))
    _div_ok(L, a, np.ldexp(_mant(rng, n), eb)[ok], "whole window")
    # exact quotients and zero numerators
    m = 1_000_000
    b3 = _rand_doubles(rng, m, -20, 20, signed=False)
    q3 = (rng.integers(1, 1 << 40, size=m).astype(np.float64)) * np.exp2(rng.integers(-30, 30, m))
    a3 = q3 * b3
    keep = (a3 / b3) == q3
    _div_ok(L, a3[keep], b3[keep], "exact quotients")
    # (+0 only: div_cr(-0, b) is +0 where -0 / b is -0 -- the header says so, and the kernel adds the mean
    # stress or +0 to the quotient, which gives the same bits for either zero)
    _div_ok(L, np.zeros(m), np.ldexp(_mant(rng, m), rng.integers(B0, B1 + 1, size=m)), "zero numerators")
