// hakai_contact_cells.hpp -- the cell grid of the contact search (hakai_contact_dev.hpp): the cell index
// of a point and the cull of the 27 neighbour cells by a candidate triangle's bounding sphere. One
// source for the device and for the CPU test: tests/test_reach_mask.py compiles THIS file with a
// host compiler (no contraction) and holds reach_mask against a plain restatement of the
// reference's two tests, so an edit here is an edit it sees.
// Plain pointers, no device types: nothing in here needs hip_runtime.h.
#pragma once

#include <math.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define HK_HD __host__ __device__ __forceinline__
#else
#define HK_HD static inline
#endif

namespace hk {

// Cell index of coordinate p along one axis of a pair's grid (origin amn, cell size ddiv): the
// reference's ceil((p - amn) / ddiv) (v2/HAKAI_j.jl:2333-2346), used alike for the binned i-nodes
// (bin_rec, one GPU and the multi-GPU binning) and for a triangle's first node (tri_geom).
// Compiled without contraction by every includer.
HK_HD long long cell_index(double p, double amn, double ddiv) { return (long long)ceil((p - amn) / ddiv); }

// Which cells dc (0..26: dx fastest, the reference's dz, dy, dx loops) of the 27 around the
// candidate's first-node cell mj can hold an i-node within the candidate's sphere (|p - c| < Rmax,
// :2532-2536)? A node lies in cell m when ceil((p - amn) / ddiv) == m (cell_index), i.e. p in
// (amn + (m-1) ddiv, amn + m ddiv] up to the rounding of that expression. Each box is widened by far
// more than that rounding and the radius by a relative 1e-9, so a cell is dropped only if no node
// in it can pass the sphere test: the search visits fewer cells and finds the same events. The
// squared distance is separable, 3 per axis; NaN geometry keeps every cell. Returns a 27-bit mask.
HK_HD unsigned reach_mask(const long long mj[3], const double c[3], double Rmax, const double amn[3], double ddiv) {
    double t2[3][3];
#pragma unroll
    for (int d = 0; d < 3; ++d)
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double m = (double)(mj[d] + (k - 1));
            const double eps = 1e-9 * ddiv + 1e-12 * (fabs(amn[d]) + fabs(m) * ddiv);
            const double lo = amn[d] + (m - 1.0) * ddiv - eps, hi = amn[d] + m * ddiv + eps;
            const double t = fmax(fmax(lo - c[d], c[d] - hi), 0.0);
            t2[d][k] = t * t;
        }
    const double r = Rmax * (1.0 + 1e-9) + 1e-9 * ddiv;
    const double r2 = r * r * (1.0 + 1e-9);
    unsigned mask = 0;
#pragma unroll
    for (int dc = 0; dc < 27; ++dc)
        if (!(t2[0][dc % 3] + t2[1][(dc / 3) % 3] + t2[2][dc / 9] > r2)) mask |= 1u << dc;
    return mask;
}

}  // namespace hk
