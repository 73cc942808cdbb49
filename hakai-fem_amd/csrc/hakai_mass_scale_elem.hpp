// hakai_mass_scale_elem.hpp -- selective mass scaling of one C3D8 element (hakai_mass_scale,
// include/hakai_hip.h): the mass to add to each of the element's 8 nodes so that the element's
// guaranteed stable step dt_safe reaches a target, and the two results of the stable-step diagnostic
// with that mass in place. On top of hakai_stable_dt_elem.hpp, whose functions are used as they are:
// V, gg, ss, V0 and the material constants are formed exactly as stable_element forms them. One
// source for the device (k_mass_need in hakai_mass_scale.hip, k_stable_dt<true, true> in
// hakai_stable_dt.hip) and for the CPU: tests/test_mass_scale_cpu.py compiles THIS file with a host
// compiler (no contraction) and holds it against tests/mass_scale_ref.py bit for bit. Every
// translation unit that includes it is compiled with -ffp-contract=off; the operation order below IS
// the definition.
//
//   kappa = (Kb * V) * gg + two_mu * ss          stable_finish's expression, restated
//   m0    = rho8 * V0                            the element's share of a node's uploaded mass
//   half  = (0.5 * dt_target) / safety
//   a     = kappa * (half * half) - m0           the added mass that reaches the target
//   cap   = (max_factor - 1.0) * m0              (+inf with max_factor = +inf: no cap)
//   a > cap: a = cap, the element counts as capped
//   added_new = a > added_prev ? a : added_prev  (mass only grows; the same call again changes no bit)
// An element with V0 <= 0, V == 0 or a kappa that is not finite is unfixable and keeps added_prev.
// DESIGN.md section 2, "Selective mass scaling", counts the roundings: for safety <= 1 - 2^-40 an
// element that is neither capped nor unfixable has 2 sqrt((m0 + added_new) / kappa) >= dt_target.
#pragma once

#include "hakai_stable_dt_elem.hpp"

namespace hk {

constexpr int kMassOk = 0, kMassCapped = 1, kMassUnfixable = 2;

// (0.5 * dt_target) / safety: formed once per call on the host.
static inline double mass_half(double dt_target, double safety) { return (0.5 * dt_target) / safety; }

// The rule above: the element's added mass after the call, *status one of kMass*.
HK_SD_HD double mass_need(double V, double gg, double ss, double V0, const StableMat& m, double half,
                          double max_factor, double added_prev, int* status) {
    *status = kMassUnfixable;
    if (V0 <= 0.0 || V == 0.0) return added_prev;
    const double kappa = (m.Kb * V) * gg + m.two_mu * ss;
    if (!(kappa - kappa == 0.0)) return added_prev;  // +inf (a collapsed Gauss point) or NaN
    *status = kMassOk;
    const double m0 = m.rho8 * V0;
    double a = kappa * (half * half) - m0;
    const double cap = (max_factor - 1.0) * m0;
    if (a > cap) {
        a = cap;
        *status = kMassCapped;
    }
    return a > added_prev ? a : added_prev;
}

// (m0 + added) / m0 of an element with V0 > 0: the factor its nodes' shares have grown by.
HK_SD_HD double mass_factor(double V0, const StableMat& m, double added) {
    const double m0 = m.rho8 * V0;
    return (m0 + added) / m0;
}

// stable_finish with the element's added mass: me = rho8 V0 + added in dt_safe, and dt_est, L / c at
// the unscaled density, stretched by sqrt(me / (rho8 V0)). With added == 0 both are stable_finish's
// bits (me is m0, the root is 1).
HK_SD_HD void stable_finish_added(double V, double gg, double ss, double V0, double Amax, const StableMat& m,
                                  double added, double* dt_est, double* dt_safe) {
    if (V0 <= 0.0 || V == 0.0 || Amax == 0.0) {
        *dt_est = 0.0;
        *dt_safe = 0.0;
        return;
    }
    const double L = V / Amax;
    const double kappa = (m.Kb * V) * gg + m.two_mu * ss;
    const double m0 = m.rho8 * V0;
    const double me = m0 + added;
    *dt_est = (L / m.c) * __builtin_sqrt(me / m0);
    *dt_safe = 2.0 * __builtin_sqrt(me / kappa);
}

// One element on one thread (the host's form): the sums of stable_element, then the rule and the
// diagnostic with the new mass.
static inline double mass_element(const double (&x)[8][3], const double (&X)[8][3], const StableMat& m, double half,
                                  double max_factor, double added_prev, int* status, double* factor,
                                  double* dt_est, double* dt_safe) {
    double t[8][kStableTerms], d0[8], S[kStableTerms], p[8];
    for (int k = 0; k < 8; ++k) {
        d0[k] = stable_det0(k, X);
        stable_gp(k, x, t[k]);
    }
    for (int j = 0; j < kStableTerms; ++j) {
        const double v[8] = {t[0][j], t[1][j], t[2][j], t[3][j], t[4][j], t[5][j], t[6][j], t[7][j]};
        S[j] = stable_sum8(v);
    }
    for (int i = 0; i < 8; ++i) p[i] = stable_node_gg(S[1 + i], S[9 + i], S[17 + i], S[0]);
    const double gg = stable_sum8(p), V0 = stable_v0(d0);
    const double added = mass_need(S[0], gg, S[25], V0, m, half, max_factor, added_prev, status);
    *factor = V0 > 0.0 ? mass_factor(V0, m, added) : 0.0;
    stable_finish_added(S[0], gg, S[25], V0, stable_amax(x), m, added, dt_est, dt_safe);
    return added;
}

}  // namespace hk
