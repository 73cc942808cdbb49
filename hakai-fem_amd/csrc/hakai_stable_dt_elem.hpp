// hakai_stable_dt_elem.hpp -- the stable-time-step diagnostic of one C3D8 element
// (hakai_stable_dt, include/hakai_hip.h): material constants, the terms of one Gauss point, their
// pairwise combination, the face areas and the two results. One source for the device
// (k_stable_dt in hakai_stable_dt.hip, lane k = Gauss point k) and for the CPU:
// tests/test_stable_dt_cpu.py compiles THIS file with a host compiler (no contraction) and holds it
// against tests/stable_dt_ref.py bit for bit, so an edit here is an edit the test sees.
// Plain arrays, no device types: nothing in here needs hip_runtime.h. Every translation unit that
// includes it is compiled with -ffp-contract=off; the operation order below IS the definition.
//
// Notation ("Stable time step"): x[i] = coord_i + u_i the current position of
// node i, X[i] = coord_i; P_k the cal_Pusai_hexa table at Gauss point k (v2/HAKAI_j.jl:1895-1943);
// J_k = P_k x^T; a_k = |det J_k|; G_k = J_k^-1 P_k (dN/dx). The code never divides by det J_k where
// it can help it: H_k = sgn(det J_k) adj(J_k) P_k is a_k G_k exactly in real arithmetic and finite
// at a collapsed Gauss point, and a_k sum G_k^2 = sum H_k^2 / a_k is the only division (+inf at a
// collapsed point with a non-zero H_k: the bound then reports 0, which is a lower bound still).
//
//   V      = sum_k a_k                       V0 = sum_k det(P_k X^T), signed (hakai_lumped_mass's)
//   dt_est  = (V / A_max) / c                A_max the largest face area, c = sqrt(M / rho')
//   kappa  = Kb V sum (S / V)^2 + 2mu sum_k s_k,   S = sum_k H_k,  s_k = sum H_k^2 / a_k
//            (sum (S / V)^2: per node (g0^2 + g1^2) + g2^2, then the pairwise tree over the nodes)
//   dt_safe = 2 sqrt(rho8 V0 / kappa)
// dt_safe bounds the critical step of the ELASTIC stiffness from below (the plastic tangent is no
// stiffer); the penalty stiffness of contact is outside it.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_SD_HD __host__ __device__ __forceinline__
#else
#define HK_SD_HD static inline
#endif

namespace hk {

// Per-material constants of the diagnostic, formed once per call on the host by stable_mat.
struct StableMat {
    double c;       // dilatational wave speed sqrt(M / rho'), M = E (1 - nu) / ((1 + nu)(1 - 2 nu))
    double Kb;      // bulk modulus E / (3 (1 - 2 nu))
    double two_mu;  // E / (1 + nu)
    double rho8;    // rho' / 8, rho' = rho * mass_scaling: m_e = rho8 * V0
};

// The one operation order (tests/stable_dt_ref.py stable_mat restates it):
//   rho' = rho * ms;  M = (E * (1 - nu)) / ((1 + nu) * (1 - 2 nu));  c = sqrt(M / rho');
//   Kb = E / (3 * (1 - 2 nu));  two_mu = E / (1 + nu);  rho8 = rho' / 8.
static inline StableMat stable_mat(double young, double poisson, double density, double mass_scaling) {
    StableMat m;
    const double rho = density * mass_scaling;
    const double M = (young * (1.0 - poisson)) / ((1.0 + poisson) * (1.0 - 2.0 * poisson));
    m.c = __builtin_sqrt(M / rho);
    m.Kb = young / (3.0 * (1.0 - 2.0 * poisson));
    m.two_mu = young / (1.0 + poisson);
    m.rho8 = rho / 8.0;
    return m;
}

constexpr int kStableTerms = 26;  // a_k, H_k[3][8] (c-major), s_k: the sums taken over the Gauss points

// cal_Pusai_hexa at Gauss point k (k bits 4, 2, 1 = signs of xi, eta, zeta), pusai_table's expressions.
HK_SD_HD void stable_pusai(int k, double (&P)[3][8]) {
    const double sx[8] = {-1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0, -1.0};
    const double sy[8] = {-1.0, -1.0, 1.0, 1.0, -1.0, -1.0, 1.0, 1.0};
    const double sz[8] = {-1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0, 1.0};
    const double g = 1.0 / __builtin_sqrt(3.0);
    const double gzai = (k & 4) ? g : -g, eta = (k & 2) ? g : -g, tueta = (k & 1) ? g : -g;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        P[0][i] = 1.0 / 8.0 * sx[i] * (1.0 + eta * sy[i]) * (1.0 + tueta * sz[i]);
        P[1][i] = 1.0 / 8.0 * sy[i] * (1.0 + gzai * sx[i]) * (1.0 + tueta * sz[i]);
        P[2][i] = 1.0 / 8.0 * sz[i] * (1.0 + gzai * sx[i]) * (1.0 + eta * sy[i]);
    }
}

// J = P x^T summed in node order, and its determinant: hakai_lumped_mass's expressions.
HK_SD_HD double stable_jac(const double (&P)[3][8], const double (&x)[8][3], double (&J)[3][3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            double acc = P[a][0] * x[0][b];
#pragma unroll
            for (int i = 1; i < 8; ++i) acc = acc + P[a][i] * x[i][b];
            J[a][b] = acc;
        }
    return J[0][0] * J[1][1] * J[2][2] + J[0][1] * J[1][2] * J[2][0] + J[0][2] * J[1][0] * J[2][1] -
           J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] - J[0][2] * J[1][1] * J[2][0];
}

// det(P_k X^T): Gauss point k's share of V0. X is the model's, so V0 is a constant of the element
// (the kernel forms it at a context's first call and keeps it).
HK_SD_HD double stable_det0(int k, const double (&X)[8][3]) {
    double P[3][8], J[3][3];
    stable_pusai(k, P);
    return stable_jac(P, X, J);
}

// Gauss point k at the current positions: t[0] = a_k, t[1 + 8c + i] = H_k[c][i], t[25] = s_k.
HK_SD_HD void stable_gp(int k, const double (&x)[8][3], double (&t)[kStableTerms]) {
    double P[3][8], J[3][3];
    stable_pusai(k, P);
    const double det = stable_jac(P, x, J);
    const double a = det < 0.0 ? -det : det;
    // adj(J): adj[c][r] = cofactor of J[r][c]
    double A[3][3];
    A[0][0] = J[1][1] * J[2][2] - J[1][2] * J[2][1];
    A[0][1] = J[0][2] * J[2][1] - J[0][1] * J[2][2];
    A[0][2] = J[0][1] * J[1][2] - J[0][2] * J[1][1];
    A[1][0] = J[1][2] * J[2][0] - J[1][0] * J[2][2];
    A[1][1] = J[0][0] * J[2][2] - J[0][2] * J[2][0];
    A[1][2] = J[0][2] * J[1][0] - J[0][0] * J[1][2];
    A[2][0] = J[1][0] * J[2][1] - J[1][1] * J[2][0];
    A[2][1] = J[0][1] * J[2][0] - J[0][0] * J[2][1];
    A[2][2] = J[0][0] * J[1][1] - J[0][1] * J[1][0];
    t[0] = a;
    double q = 0.0;
#pragma unroll
    for (int c = 0; c < 3; ++c)
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const double h = (A[c][0] * P[0][i] + A[c][1] * P[1][i]) + A[c][2] * P[2][i];
            const double hs = det < 0.0 ? -h : h;
            t[1 + 8 * c + i] = hs;
            q = q + hs * hs;
        }
    t[25] = q == 0.0 ? 0.0 : q / a;
}

// The sum over the Gauss points of one term, v[k] its value at point k: the pairwise tree
// ((0+1)+(2+3))+((4+5)+(6+7)), which an xor-1/2/4 butterfly over 8 lanes forms on every lane.
HK_SD_HD double stable_sum8(const double (&v)[8]) {
    return ((v[0] + v[1]) + (v[2] + v[3])) + ((v[4] + v[5]) + (v[6] + v[7]));
}

// V0 as hakai_lumped_mass sums it: from 0, Gauss points in order.
HK_SD_HD double stable_v0(const double (&d)[8]) {
    double V = 0.;
#pragma unroll
    for (int k = 0; k < 8; ++k) V = V + d[k];
    return V;
}

// |(x[n2] - x[n0]) x (x[n3] - x[n1])|^2 of the face (n0 n1 n2 n3): its area is half the root.
HK_SD_HD double stable_face2(const double (&x)[8][3], int n0, int n1, int n2, int n3) {
    const double d1x = x[n2][0] - x[n0][0], d1y = x[n2][1] - x[n0][1], d1z = x[n2][2] - x[n0][2];
    const double d2x = x[n3][0] - x[n1][0], d2y = x[n3][1] - x[n1][1], d2z = x[n3][2] - x[n1][2];
    const double cx = d1y * d2z - d1z * d2y, cy = d1z * d2x - d1x * d2z, cz = d1x * d2y - d1y * d2x;
    return (cx * cx + cy * cy) + cz * cz;
}

// The largest of the six face areas, C3D8 faces 1234, 5678, 1265, 2376, 3487, 4158. The correctly
// rounded root is monotone, so one root of the largest squared norm is the largest of the six roots.
HK_SD_HD double stable_amax(const double (&x)[8][3]) {
    double A = stable_face2(x, 0, 1, 2, 3);
    double f = stable_face2(x, 4, 5, 6, 7);
    A = f > A ? f : A;
    f = stable_face2(x, 0, 1, 5, 4);
    A = f > A ? f : A;
    f = stable_face2(x, 1, 2, 6, 5);
    A = f > A ? f : A;
    f = stable_face2(x, 2, 3, 7, 6);
    A = f > A ? f : A;
    f = stable_face2(x, 3, 0, 4, 7);
    A = f > A ? f : A;
    return 0.5 * __builtin_sqrt(A);
}

// Node i's share of sum g~^2: its three summed terms S_c = sum_k H_k[c][i] over V, squared.
HK_SD_HD double stable_node_gg(double S0, double S1, double S2, double V) {
    const double g0 = S0 / V, g1 = S1 / V, g2 = S2 / V;
    return (g0 * g0 + g1 * g1) + g2 * g2;
}

// The two results from V = sum a_k, gg = sum g~^2 (stable_sum8 of the nodes' shares), ss = sum s_k,
// V0 and A_max. An element with V0 <= 0, V == 0 or A_max == 0 reports 0 for both.
HK_SD_HD void stable_finish(double V, double gg, double ss, double V0, double Amax, const StableMat& m,
                            double* dt_est, double* dt_safe) {
    if (V0 <= 0.0 || V == 0.0 || Amax == 0.0) {
        *dt_est = 0.0;
        *dt_safe = 0.0;
        return;
    }
    const double L = V / Amax;
    *dt_est = L / m.c;
    const double kappa = (m.Kb * V) * gg + m.two_mu * ss;
    const double me = m.rho8 * V0;
    *dt_safe = 2.0 * __builtin_sqrt(me / kappa);
}

// One element on one thread (the host's form; the kernel spreads the Gauss points over 8 lanes, sums
// them in the same tree with lane exchanges, leaves node i's sums on lane i and calls the same
// functions).
static inline void stable_element(const double (&x)[8][3], const double (&X)[8][3], const StableMat& m,
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
    stable_finish(S[0], stable_sum8(p), S[25], stable_v0(d0), stable_amax(x), m, dt_est, dt_safe);
}

}  // namespace hk
