// hakai_walls_node.hpp -- the arithmetic of the rigid walls (hakai_set_walls, include/hakai_hip.h):
// the wall's normalised normal, its frame at a step (origin and velocity from the two amplitude
// values) and the force of one wall on one node. One source for the device (k_loads in
// hakai_loads.hip), for the host planner and for the CPU: tests/test_walls_cpu.py compiles THIS file
// with a host compiler (no contraction) and holds it against tests/walls_ref.py bit for bit, so an
// edit here is an edit the test sees. Plain arrays, no device types. Every translation unit that
// includes it is compiled with -ffp-contract=off; the operation order below IS the definition.
#pragma once

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_WL_HD __host__ __device__ __forceinline__
#else
#define HK_WL_HD static inline
#endif

namespace hk {

// One wall as the kernel reads it: kWallRow doubles per wall.
//   [0..2] n   [3..5] origin   [6..8] motion   [9] stiffness   [10] scale   [11] zeta   [12] mu
constexpr int kWallRow = 13;

// n = normal / sqrt((nx*nx + ny*ny) + nz*nz), each component divided. Returns the length (the
// planner refuses a length that is not finite and positive).
HK_WL_HD double walls_normalise(const double (&normal)[3], double (&n)[3]) {
    const double len = sqrt((normal[0] * normal[0] + normal[1] * normal[1]) + normal[2] * normal[2]);
    n[0] = normal[0] / len;
    n[1] = normal[1] / len;
    n[2] = normal[2] / len;
    return len;
}

// The wall's frame at a step from s0 = amp(tau0), sm = amp(taum):
//   o[c] = origin[c] + motion[c] * s0,   vw[c] = motion[c] * ((s0 - sm) / dt).
HK_WL_HD void walls_frame(const double* origin, const double* motion, double s0, double sm, double dt,
                          double (&o)[3], double (&vw)[3]) {
    const double rate = (s0 - sm) / dt;
    for (int c = 0; c < 3; ++c) {
        o[c] = origin[c] + motion[c] * s0;
        vw[c] = motion[c] * rate;
    }
}

// The signed distance of the node at x = coord + u from the plane (o, n):
//   g = ((x0 - o0) * n0 + (x1 - o1) * n1) + (x2 - o2) * n2.
HK_WL_HD double walls_gap(const double (&coord)[3], const double (&u)[3], const double (&o)[3], const double* n) {
    const double a0 = ((coord[0] + u[0]) - o[0]) * n[0];
    const double a1 = ((coord[1] + u[1]) - o[1]) * n[1];
    const double a2 = ((coord[2] + u[2]) - o[2]) * n[2];
    return (a0 + a1) + a2;
}

// The force of the wall on a node that penetrates by d = -g > 0 (the caller tests d > 0, strictly):
//   v[c]  = (u[c] - um[c]) / dt - vw[c]
//   k     = stiffness + scale * (m / (dt * dt))
//   vn    = (v0 * n0 + v1 * n1) + v2 * n2
//   cd    = (2.0 * zeta) * sqrt(m * k)
//   N     = max(k * d - cd * vn, 0.0)
//   vt[c] = v[c] - vn * n[c]
//   s     = sqrt((vt0 * vt0 + vt1 * vt1) + vt2 * vt2)
//   T     = min(mu * N, (m * s) / dt)
//   F[c]  = s > 0 ? N * n[c] - (T / s) * vt[c] : N * n[c]
HK_WL_HD void walls_force(double d, const double (&u)[3], const double (&um)[3], double m, double dt,
                          const double (&vw)[3], const double* n, double stiffness, double scale, double zeta,
                          double mu, double (&F)[3]) {
    double v[3], vt[3];
    for (int c = 0; c < 3; ++c) v[c] = (u[c] - um[c]) / dt - vw[c];
    const double k = stiffness + scale * (m / (dt * dt));
    const double vn = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2];
    const double cd = (2.0 * zeta) * sqrt(m * k);
    const double Nr = k * d - cd * vn;
    const double N = Nr > 0.0 ? Nr : 0.0;
    for (int c = 0; c < 3; ++c) vt[c] = v[c] - vn * n[c];
    const double s = sqrt((vt[0] * vt[0] + vt[1] * vt[1]) + vt[2] * vt[2]);
    const double Ta = mu * N, Tb = (m * s) / dt;
    const double T = Ta < Tb ? Ta : Tb;
    if (s > 0.0) {
        const double r = T / s;
        for (int c = 0; c < 3; ++c) F[c] = N * n[c] - r * vt[c];
    } else {
        for (int c = 0; c < 3; ++c) F[c] = N * n[c];
    }
}

}  // namespace hk
