// hakai_stable_dt_dev.hpp -- device helpers shared by the kernels that evaluate
// hakai_stable_dt_elem.hpp with the project's mapping (8 lanes per element, lane k = Gauss point k,
// 32 elements per 256-thread block): k_stable_dt (hakai_stable_dt.hip) and k_mass_need
// (hakai_mass_scale.hip). Needs hip_runtime.h; compiled without contraction by both.
#pragma once
#include <hip/hip_runtime.h>

#include <climits>

#include "hakai_device.hpp"
#include "hakai_stable_dt_elem.hpp"

namespace hk {
namespace sdt {

constexpr int kEPB = 32;        // elements per block
constexpr int kThreads = 256;   // 8 lanes per element
constexpr int kNone = INT_MAX;  // element id of "no active element": loses every tie

template <class I>
__device__ __forceinline__ void take_min(double& v, I& id, double ov, I oid) {
    if (ov < v || (ov == v && oid < id)) {
        v = ov;
        id = oid;
    }
}

template <class I>
__device__ __forceinline__ void take_max(double& v, I& id, double ov, I oid) {
    if (ov > v || (ov == v && oid < id)) {
        v = ov;
        id = oid;
    }
}

// The 24 sums S[c][i] = sum_k H_k[c][i] (t[1 + 8c + i] on lane k), left scattered: lane i gets the
// three of node i. Partners k^1, k^2, k^4 in that order, each lane keeping the nodes whose bit
// matches its own, so every sum is the pairwise tree ((0+1)+(2+3))+((4+5)+(6+7)) of allreduce8 and
// of the header's stable_sum8 (an addition commutes), with 21 exchanges instead of 72.
__device__ __forceinline__ void sum_scatter8(const double (&t)[hk::kStableTerms], double (&out)[3], int k) {
    const bool b0 = (k & 1) != 0, b1 = (k & 2) != 0, b2 = (k & 4) != 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        double w[4], u[2];
#pragma unroll
        for (int s = 0; s < 4; ++s) {  // nodes 2s + b0
            const double lo = t[1 + 8 * c + 2 * s], hi = t[1 + 8 * c + 2 * s + 1];
            w[s] = (b0 ? hi : lo) + hk::dpp<hk::kDppXor1>(b0 ? lo : hi);
        }
#pragma unroll
        for (int s = 0; s < 2; ++s)    // nodes 4s + 2 b1 + b0
            u[s] = (b1 ? w[2 * s + 1] : w[2 * s]) + hk::dpp<hk::kDppXor2>(b1 ? w[2 * s] : w[2 * s + 1]);
        out[c] = (b2 ? u[1] : u[0]) + __shfl_xor(b2 ? u[0] : u[1], 4, 8);
    }
}

// What lane k of an element holds after the gather, the exchanges and the sums: the current positions
// of the 8 nodes and, the same bits on every lane, V0, V = sum a_k, gg = sum g~^2, ss = sum s_k.
struct ElemSums {
    double x[8][3];
    double V0, V, gg, ss;
};

// Lane k gathers node k's coord and u (the 8 lanes of an element read its 8 nodes in one
// instruction), the positions go round the 8-lane group by wave shuffles (no LDS, no barrier), every
// lane forms the 26 terms of its Gauss point and the sums over the Gauss points are the xor-1/2/4
// butterfly. kHaveV0 false: V0 is formed from the lanes' determinants in Gauss-point order and, with
// store set, written to v0[e]; true: read from v0[e] -- the same bits either way.
template <bool kHaveV0>
__device__ __forceinline__ void elem_sums(const double* coord, const double* u, const int* conn, double* v0,
                                          long long ee, int k, bool store, ElemSums& s) {
    const long long n = conn[8 * ee + k];
    double Xk[3], xk[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        Xk[c] = coord[3 * n + c];
        xk[c] = coord[3 * n + c] + u[3 * n + c];
    }
    if constexpr (kHaveV0) {
        s.V0 = v0[ee];
    } else {
        double X[8][3], d0[8];
#pragma unroll
        for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 3; ++c) X[i][c] = __shfl(Xk[c], i, 8);
        const double det0 = hk::stable_det0(k, X);
#pragma unroll
        for (int i = 0; i < 8; ++i) d0[i] = __shfl(det0, i, 8);
        s.V0 = hk::stable_v0(d0);
        if (store && k == 0) v0[ee] = s.V0;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
        for (int c = 0; c < 3; ++c) s.x[i][c] = __shfl(xk[c], i, 8);
    double t[hk::kStableTerms];
    hk::stable_gp(k, s.x, t);
    s.V = hk::allreduce8(t[0]);
    s.ss = hk::allreduce8(t[25]);
    double Sn[3];
    sum_scatter8(t, Sn, k);
    s.gg = hk::allreduce8(hk::stable_node_gg(Sn[0], Sn[1], Sn[2], s.V));
}

}  // namespace sdt
}  // namespace hk
