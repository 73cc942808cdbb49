// hakai_exact_math.hpp -- scalar helpers of the reference-order element kernel (elem_step_exact in
// hakai_elem_exact.hpp): the correctly rounded divisions, the hardening-segment search and the ductile
// table. One source for the device and for the CPU tests: tests/test_div3.py and
// tests/test_exact_chains.py compile THIS file with a host compiler (no contraction, fma enabled)
// and compare it with IEEE division and with the oracle, so an edit here is an edit they see.
// Plain pointers, no device types: nothing in here needs hip_runtime.h.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_HD __host__ __device__ __forceinline__
#else
#define HK_HD static inline
#endif

namespace hk {

// x / 3.0 correctly rounded for EVERY finite double (zeros and subnormals included; an infinite x
// gives NaN where x / 3.0 is x), without an IEEE division sequence: q = RN(x*yh) with
// yh = RN(1/3), r = x - 3q exactly (one fma: 3q lies within 2 ulp of x, so the difference is a
// small multiple of q's last place, and q's last place is never below x's, subnormal q included),
// then RN(q + r*yh). q + r/3 is x/3 itself and r*yh misses r/3 by |r| * 2^-54 <= ulp(q) * 2^-53,
// while x/3 (a multiple of a third of the result's last place) is either representable or at least
// 1/6 ulp from every rounding boundary: both round the same way. No intermediate can underflow
// inexactly: r is exact and r*yh exists only inside the last fma.
// Signed zeros: the residual is taken negated, nr = 3q - x, and multiplied by -yh. The values are
// the same, and for x = -0 (q = -0, nr = -0 + +0 = +0) the last fma is (+0 * -yh) + -0 = -0, as IEEE
// division gives; round 5's fma(fma(-q, 3, x), yh, q) turned -0 into +0 there. (Negating the
// constant and not nr keeps a host compiler from folding the negation into the first fma, which
// changes the sign of a zero.)
//
// Round 6 used RN(x*yh + RN(x*yl)), yl = RN(1/3 - yh), two operations. That is correctly rounded
// only while x*yl is normal or rounds to zero: for 2^-1021 <= |x| < 2^-1019 the product underflows
// to 0 or 2^-1074, an error of up to half of the RESULT's last place (2^-1074 there), and a third
// of the mantissas in those two binades came out one ulp off. tests/test_div3.py sweeps every
// binade from 2^-1074 to 2^1023 against IEEE division. Cost and the alternatives timed: DESIGN.md
// section 2, "div3 over the whole range".
HK_HD double div3(double x) {
    constexpr double yh = 1.0 / 3.0;
    const double q = x * yh;
    const double nr = __builtin_fma(q, 3.0, -x);
    return __builtin_fma(nr, -yh, q);
}

// a / b correctly rounded given rb = RN(1/b) (one IEEE division per divisor): two Newton-Markstein
// corrections of q0 = RN(a*rb). q0 is within 1.5 ulp of a/b, q1 within one ulp, and then
// RN(q1 + (a - b*q1)*rb) is RN(a/b) (Markstein's theorem: the residual is exact for a faithful
// q1, rb is the correctly rounded reciprocal).
// DOMAIN. The theorem needs every step free of underflow and overflow: rb and the quotient normal,
// and the residuals a - b*q (about 2^-52 |a|, bits down to 2^-105 |a|) exactly representable, that
// is at or above 2^-1074. With ea = exponent(a), eb = exponent(b) (|a| in [2^ea, 2^(ea+1))) it
// equals a / b bit for bit on
//     ea >= -969,   -1022 <= eb <= 1021,   -1021 <= ea - eb <= 1022
// (kDivCr* below), and for a = +0 with any such b; a = -0 gives +0 where a / b is -0 (the residual
// -q0*b + a is +0), which the kernel's next operation, adding the mean stress or +0, hides. Swept on the CPU (3e8 pairs over all exponents,
// 4e8 with ea in [-1012, -960], 2e8 each at the other edges): no failure inside; below it the share
// of misrounded pairs halves with every step of ea up from -1074 (a residual rounded at 2^-1075
// matters only for quotients that close to a midpoint) and the last seen was at ea = -998; b
// subnormal and ea - eb outside the bounds (subnormal or overflowing quotient) fail in bulk. With
// eb = 1022 or 1023 (rb subnormal) the sweep found no failure, but the theorem does not cover it.
// tests/test_div3.py checks every edge of the window bit for bit, hard (near-midpoint) cases
// included; DESIGN.md section 2 says why the kernel's operands (q, V, dev*s) lie far inside it.
constexpr int kDivCrMinExpA = -969;
constexpr int kDivCrMinExpB = -1022, kDivCrMaxExpB = 1021;
constexpr int kDivCrMinExpQ = -1021, kDivCrMaxExpQ = 1022;  // bounds of ea - eb
HK_HD double div_cr(double a, double b, double rb) {
    const double q0 = a * rb;
    const double q1 = __builtin_fma(__builtin_fma(-q0, b, a), rb, q0);
    return __builtin_fma(__builtin_fma(-q1, b, a), rb, q1);
}

// Hardening segment of the *Plastic table for a Gauss point at equivalent plastic strain eqp
// (v2/HAKAI_j.jl:1255-1264), 0-based: the first j >= 1 with eqp <= pl_eps[j] gives segment j-1; beyond
// the last row (and for a one-row table's callers, which never get here with npp < 2 segments to
// choose from) the last segment npp-2.
HK_HD int plastic_segment(const double* pl_eps, int npp, double eqp) {
    int p = npp - 2;
    for (int j = 1; j < npp; ++j) {
        if (eqp <= pl_eps[j]) {
            p = j - 1;
            break;
        }
    }
    return p;
}

// Ductile table (:720-733): fracture strain at element triaxiality t_e (t_e >= 0), last row
// outside the bracketing rows.
HK_HD double ductile_fr(const double* du_eps, const double* du_tri, int nd, double t_e) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    double fr = du_eps[nd - 1];
    for (int j = 0; j + 1 < nd; ++j) {
        if (t_e >= du_tri[j] && t_e < du_tri[j + 1]) {
            fr = du_eps[j] + (du_eps[j + 1] - du_eps[j]) / (du_tri[j + 1] - du_tri[j]) * (t_e - du_tri[j]);
            break;
        }
    }
    return fr;
}

}  // namespace hk
