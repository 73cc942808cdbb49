// hakai_elem_history_gp.hpp -- the element-set history's arithmetic (hakai_elem_history_*,
// include/hakai_hip.h): the terms of one Gauss point, the elastic energy density w_e, the plastic
// work density w_p with its walk over the hardening table, and their combination over the 8 Gauss
// points of one C3D8 element. One source for the device (hakai_elem_history.hip, lane k = Gauss
// point k) and for the CPU: tests/test_elem_history_cpu.py compiles THIS file with a host compiler
// (no contraction) and holds it against tests/elem_history_ref.py bit for bit.
// Plain arrays, no device types: nothing in here needs hip_runtime.h. Every translation unit that
// includes it is compiled with -ffp-contract=off; the operation order below IS the definition.
//
// Notation ("Element-set history"): x[i] = coord_i + u_i, X[i] = coord_i; P_k
// the cal_Pusai_hexa table at Gauss point k; a_k = |det(P_k x^T)|, a0_k = |det(P_k X^T)| -- the
// determinants are hakai_stable_dt_elem.hpp's stable_jac, the same bits. sigma, eps (xx, yy, zz, xy,
// yz, zx) and eqps are the stored state of the Gauss point.
//
//   t[0]     a_k                      t[1]      a0_k
//   t[2..7]  a_k sigma[c]             t[8..13]  a_k eps[c]
//   t[14]    a_k eqps                 t[15]     a_k w_e(sigma)         t[16]  a0_k w_p(eqps)
//   t[17]    eqps                     t[18]     q, the Mises stress
//   w_e = q^2 / (6 G) + p^2 / (2 K),  p = tr sigma / 3,  K = (Dn + 2 Do) / 3
//   w_p(e) = the area under the piecewise linear yield curve from pl_eps[0] to e: yield0 at
//            pl_eps[0], slope Hd[j] between rows j and j+1, the last slope continued beyond the last
//            row (slope 0 with a single row), 0 for an elastic material (npp == 0) and for
//            e <= pl_eps[0]. Reference weights a0_k: plastic flow is isochoric.
// Per element the 20 values V, V0, S[6], E[6], EQ, SE, PD (t[0..16] summed over the Gauss points in
// the pairwise tree ((0+1)+(2+3))+((4+5)+(6+7)), allreduce8's order), eqps_max, q_max (the largest
// of t[17], t[18]; a NaN never wins, so both lie in [0, +inf]) and J = V / V0.
//
// SE + PD is not W_int: the radial return takes H from the segment at the start of the increment,
// the stress update carries no rotation, the volume changes, and a deleted element's energy leaves
// the sums (eroded energy is not tracked). The gap is measured (tests/test_elem_history_cpu.py).
#pragma once

#include "hakai_stable_dt_elem.hpp"

namespace hk {

constexpr int kEhMaxPlastic = 64;  // = kMaxPlastic (hakai_device.hpp)
constexpr int kEhTerms = 19;       // per Gauss point
constexpr int kEhSums = 17;        // t[0..16] are summed, t[17], t[18] maximised
constexpr int kEhElem = 20;        // per element

// Per-material constants, formed once per enable / probe on the host by elem_hist_mat from DevMat's.
struct ElemHistMat {
    double G6;      // 6 G
    double K2;      // 2 K, K = (Dn + 2 Do) / 3
    double yield0;
    int npp, pad;
    double pl_eps[kEhMaxPlastic];
    double Hd[kEhMaxPlastic];
};

static inline ElemHistMat elem_hist_mat(double Dn, double Do, double G, double yield0, int npp, const double* pl_eps,
                                        const double* Hd) {
    ElemHistMat m;
    m.G6 = 6.0 * G;
    m.K2 = 2.0 * ((Dn + 2.0 * Do) / 3.0);
    m.yield0 = yield0;
    m.npp = npp;
    m.pad = 0;
    for (int j = 0; j < kEhMaxPlastic; ++j) {
        m.pl_eps[j] = j < npp ? pl_eps[j] : 0.0;
        m.Hd[j] = j + 1 < npp ? Hd[j] : 0.0;
    }
    return m;
}

// q^2 = ((sxx-syy)^2 + (syy-szz)^2 + (szz-sxx)^2) / 2 + 3 (sxy^2 + syz^2 + szx^2)
HK_SD_HD double elem_hist_q2(const double (&s)[6]) {
    const double d0 = s[0] - s[1], d1 = s[1] - s[2], d2 = s[2] - s[0];
    const double n = (d0 * d0 + d1 * d1) + d2 * d2;
    const double t = (s[3] * s[3] + s[4] * s[4]) + s[5] * s[5];
    return 0.5 * n + 3.0 * t;
}

HK_SD_HD double elem_hist_we(double q2, const double (&s)[6], const ElemHistMat& m) {
    const double p = ((s[0] + s[1]) + s[2]) / 3.0;
    return q2 / m.G6 + (p * p) / m.K2;
}

// The segment walk: whole segments below e add their trapezoids 0.5 (y_j + y_j+1) d_j, the one that
// holds e adds 0.5 (y_j + y(e)) (e - pl_eps[j]); y_j+1 = y_j + Hd[j] d_j. e on a breakpoint ends in
// the segment below it with the same operations a whole segment takes.
HK_SD_HD double elem_hist_wp(double e, const ElemHistMat& m) {
    if (m.npp <= 0) return 0.0;
    const int nseg = m.npp > 1 ? m.npp - 1 : 1;
    double w = 0.0, y = m.yield0;
    for (int j = 0; j < nseg; ++j) {
        const double lo = m.pl_eps[j];
        const bool whole = j + 1 < nseg && e > m.pl_eps[j + 1];
        const double d = (whole ? m.pl_eps[j + 1] : e) - lo;
        if (d > 0.0) {
            const double yn = y + m.Hd[j] * d;
            w = w + (0.5 * (y + yn)) * d;
            y = yn;
        }
        if (!whole) break;
    }
    return w;
}

// |det(P_k p^T)| at Gauss point k of the 8 positions p (current: a_k, reference: a0_k).
HK_SD_HD double elem_hist_absdet(int k, const double (&p)[8][3]) {
    double P[3][8], J[3][3];
    stable_pusai(k, P);
    const double det = stable_jac(P, p, J);
    return det < 0.0 ? -det : det;
}

// The terms of a Gauss point from its weights a = a_k, a0 = a0_k and its state.
HK_SD_HD void elem_hist_gp(double a, double a0, const double (&sig)[6], const double (&eps)[6], double eqps,
                           const ElemHistMat& m, double (&t)[kEhTerms]) {
    t[0] = a;
    t[1] = a0;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        t[2 + c] = a * sig[c];
        t[8 + c] = a * eps[c];
    }
    t[14] = a * eqps;
    const double q2 = elem_hist_q2(sig);
    t[15] = a * elem_hist_we(q2, sig, m);
    t[16] = a0 * elem_hist_wp(eqps, m);
    t[17] = eqps;
    t[18] = __builtin_sqrt(q2);
}

// The largest of v[0..7] and 0: `>` lets a NaN never win, any order gives the same value.
HK_SD_HD double elem_hist_max8(const double (&v)[8]) {
    double m = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) m = v[k] > m ? v[k] : m;
    return m;
}

// One element on one thread (the host's form; the kernel spreads the Gauss points over 8 lanes and
// combines them with lane exchanges in the same tree). sig, eps: [8][6], eqps: [8].
static inline void elem_hist_element(const double (&x)[8][3], const double (&X)[8][3], const double (&sig)[8][6],
                                     const double (&eps)[8][6], const double (&eqps)[8], const ElemHistMat& m,
                                     double (&out)[kEhElem]) {
    double t[8][kEhTerms];
    for (int k = 0; k < 8; ++k)
        elem_hist_gp(elem_hist_absdet(k, x), elem_hist_absdet(k, X), sig[k], eps[k], eqps[k], m, t[k]);
    for (int j = 0; j < kEhTerms; ++j) {
        const double v[8] = {t[0][j], t[1][j], t[2][j], t[3][j], t[4][j], t[5][j], t[6][j], t[7][j]};
        out[j] = j < kEhSums ? stable_sum8(v) : elem_hist_max8(v);
    }
    out[19] = out[0] / out[1];
}

}  // namespace hk
