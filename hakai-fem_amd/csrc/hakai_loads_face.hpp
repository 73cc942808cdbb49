// hakai_loads_face.hpp -- the arithmetic of the external loads (hakai_set_loads, include/hakai_hip.h):
// the face node lists of a C3D8 element, the amplitude rule and the consistent nodal force of one
// corner of a bilinear pressure face. One source for the device (k_loads in hakai_loads.hip), for
// the host planner and for the CPU: tests/test_loads_cpu.py compiles THIS file with a host compiler
// (no contraction) and holds it against tests/loads_ref.py bit for bit, so an edit here is an edit
// the test sees. Plain arrays, no device types. Every translation unit that includes it is compiled
// with -ffp-contract=off; the operation order below IS the definition.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_LD_HD __host__ __device__ __forceinline__
#else
#define HK_LD_HD static inline
#endif

namespace hk {

// Face k (S1..S6) as 0-based elementmat columns, corners in the order (xi, eta) = (-,-), (+,-),
// (+,+), (-,+) with g1 x g2 pointing INTO a non-inverted element: S1 = 1-2-3-4, S2 = 5-8-7-6,
// S3 = 1-5-6-2, S4 = 2-6-7-3, S5 = 3-7-8-4, S6 = 4-8-5-1.
// loads_face_code packs a face's four columns, 3 bits per corner with corner 0 in the low bits (the
// planner stores the code per pressure entry, so the kernel needs no table); loads_code_node unpacks.
HK_LD_HD unsigned loads_face_code(int face0) {
    const unsigned tab[6] = {0u | 1u << 3 | 2u << 6 | 3u << 9, 4u | 7u << 3 | 6u << 6 | 5u << 9,
                             0u | 4u << 3 | 5u << 6 | 1u << 9, 1u | 5u << 3 | 6u << 6 | 2u << 9,
                             2u | 6u << 3 | 7u << 6 | 3u << 9, 3u | 7u << 3 | 4u << 6 | 0u << 9};
    return tab[face0];
}
HK_LD_HD int loads_code_node(unsigned code, int corner) { return (int)((code >> (3 * corner)) & 7u); }

// Amplitude table value at time ct: the rule of the *Boundary amplitudes (bc_value): the first
// segment j with t[j] <= ct <= t[j+1], else segment 0 extrapolated;
//   v[j] + (v[j+1] - v[j]) * (ct - t[j]) / (t[j+1] - t[j]).   n >= 2 rows.
HK_LD_HD double loads_amp(int n, const double* t, const double* v, double ct) {
    int ti = 0;
    for (int j = 0; j < n - 1; ++j)
        if (ct >= t[j] && ct <= t[j + 1]) {
            ti = j;
            break;
        }
    return v[ti] + (v[ti + 1] - v[ti]) * (ct - t[ti]) / (t[ti + 1] - t[ti]);
}

// a x b, every product and difference rounded once.
HK_LD_HD void loads_cross(const double (&a)[3], const double (&b)[3], double (&o)[3]) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// F_a of corner a (0..3) of the face with corners x[0..3] under pa = p * amp:
//   g1 = ((x1 - x0) + (x2 - x3)) * 0.25,  g2 = ((x3 - x0) + (x2 - x1)) * 0.25,
//   h  = ((x0 - x1) + (x2 - x3)) * 0.25,
//   n0 = g1 x g2,  n1 = g1 x h,  n2 = h x g2,  sx = xi_a * (1.0 / 3.0),  sy = eta_a * (1.0 / 3.0),
//   F[c] = pa * ((n0[c] + sx * n1[c]) + sy * n2[c]).
HK_LD_HD void loads_face_corner(const double (&x)[4][3], int a, double pa, double (&F)[3]) {
    double g1[3], g2[3], h[3], n0[3], n1[3], n2[3];
    for (int c = 0; c < 3; ++c) {
        g1[c] = ((x[1][c] - x[0][c]) + (x[2][c] - x[3][c])) * 0.25;
        g2[c] = ((x[3][c] - x[0][c]) + (x[2][c] - x[1][c])) * 0.25;
        h[c] = ((x[0][c] - x[1][c]) + (x[2][c] - x[3][c])) * 0.25;
    }
    loads_cross(g1, g2, n0);
    loads_cross(g1, h, n1);
    loads_cross(h, g2, n2);
    const double third = 1.0 / 3.0;
    const double sx = (a == 1 || a == 2) ? third : -third;
    const double sy = (a >= 2) ? third : -third;
    for (int c = 0; c < 3; ++c) F[c] = pa * ((n0[c] + sx * n1[c]) + sy * n2[c]);
}

}  // namespace hk
