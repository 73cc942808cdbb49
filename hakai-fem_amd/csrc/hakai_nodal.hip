// hakai_nodal.hip -- the nodal half of the HAKAI explicit time step for gfx950: the central-difference
// update k_nodal with its Q formation, the prescribed displacements k_bc, the graph-mode step slot,
// the hold kernel, and the two download kernels that repeat k_nodal's additions (k_gather_q,
// k_own_q). Every kernel with floating-point arithmetic switches contraction off itself.
#include <hip/hip_runtime.h>

#include "hakai_kernels.hpp"

namespace hk {

// ---------------------------------------------------------------------------------------------
// Nodal kernel: one thread per node. Q is assembled by GATHER over the node's incidences in
// ascending element order, which is exactly the order of the reference's serial scatter
// (v2/HAKAI_j.jl:669-675) -- deterministic, no atomics, bit-identical Q.
// The update expression is the reference's (:564) with diag_C = 0 (:217-218), evaluated without
// contraction so it matches the reference bit for bit.
// Fast path: a padded [nN][8] incidence table (16-B vector loads, all 8 gathers in flight; padding
// points at a zero row of fe, and x + 0.0 == x leaves the sum unchanged). Nodes with more than 8
// incidences (unstructured meshes) use the CSR path.
// ---------------------------------------------------------------------------------------------
// The node's own operands are loaded FIRST, so they are in flight together with the incidence
// indices; loaded after the gather they add a third dependent memory round trip (measured with
// tools/nodal_probe.hip: 0.174 -> 0.141 ms on the C3 node count).
// Prescribed value of resolved BC entry i at the step's time (v2/HAKAI_j.jl:585-617): the entry's
// value times its group's piecewise-linear amplitude, first segment extrapolated.
__device__ __forceinline__ double bc_value(const BCArgs& a, int i) {
#pragma clang fp contract(off)
    const int g = a.grp[i];
    const double ct = a.t_rd ? (*a.t_rd + 1.0) * a.dt : a.ct;  // t * d_time, as on the host
    double amp = 1.0;
    const int na = a.amp_n[g];
    if (na > 0) {
        const double* at = a.amp_t + a.amp_off[g];
        const double* av = a.amp_v + a.amp_off[g];
        int ti = 0;
        for (int j = 0; j < na - 1; ++j)
            if (ct >= at[j] && ct <= at[j + 1]) {
                ti = j;
                break;
            }
        amp = av[ti] + (av[ti + 1] - av[ti]) * (ct - at[ti]) / (at[ti + 1] - at[ti]);
    }
    return a.val[i] * amp;
}

struct NodeIn {
    double m, uc[3], up[3], f[3];
};

template <bool FEXT>
__device__ __forceinline__ void nodal_load(const NodalArgs& a, long long n, NodeIn& in) {
    in.m = a.mass[n];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        in.uc[c] = a.u[3 * n + c];
        in.up[c] = a.u_pre_out[3 * n + c];
        in.f[c] = FEXT ? a.fext[3 * n + c] : 0.0;
    }
}

template <bool BCF>
__device__ __forceinline__ void nodal_update(const NodalArgs& a, long long n, const NodeIn& in, double Q0, double Q1,
                                             double Q2) {
#pragma clang fp contract(off)
    const double m = in.m;
    const double dt = a.dt;
    const double dC = 0.0 * m;  // diag_C .= diag_M * C, C = 0
    const double mdt2 = m / (dt * dt);
    const double inv = 1.0 / (mdt2 + dC / 2.0 / dt);
    const double Q[3] = {Q0, Q1, Q2};
    const int b0 = BCF ? a.bc_of_node[n] : -1;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double up = in.up[c];
        double v = inv * (in.f[c] - Q[c] + mdt2 * (2.0 * in.uc[c] - up) + dC / 2.0 / dt * up);
        if (BCF) {  // what k_bc would overwrite afterwards: the node's entries are consecutive
            const long long dc = 3 * n + c;
            for (int j = b0; j >= 0 && j < a.bc.n && a.bc.dof[j] <= dc; ++j)
                if (a.bc.dof[j] == dc) v = bc_value(a.bc, j);
        }
        a.u_pre_out[3 * n + c] = v;
    }
}

// MODE 0: padded [nN][8] table; 1: CSR; 2: Q from an uploaded buffer; 3: owner-computed Q + rows.
// Compile-time modes keep the kernel branch-free: a runtime branch makes the compiler drain all loads
// (vmcnt(0)) at the join, which serialises the node loads with the gather again. Blocks are dealt
// to XCDs round-robin and each XCD walks its contiguous node chunk from the END (xcd_remap_rev):
// the element kernel wrote each XCD's element range in ascending order, so the forces written last
// (still in the Infinity Cache) are gathered first (C3: 0.180 -> 0.164 ms, DESIGN.md §2 k_nodal).
template <int MODE, bool FEXT, bool BCF>
__global__ __launch_bounds__(kBlock) void k_nodal(NodalArgs a) {
#pragma clang fp contract(off)
    if (poisoned(a.poison)) return;
    const unsigned lb = xcd_remap_rev(blockIdx.x, gridDim.x);
    const long long n = (long long)lb * kBlock + threadIdx.x;
    if (n >= a.nN) return;
    NodeIn in;
    nodal_load<FEXT>(a, n, in);  // in flight with the incidence indices
    double Q0 = 0.0, Q1 = 0.0, Q2 = 0.0;
    if (MODE == 2) {
        Q0 = a.qbuf[3 * n + 0];
        Q1 = a.qbuf[3 * n + 1];
        Q2 = a.qbuf[3 * n + 2];
    } else if (MODE == 3) {  // owner-computed assembly: Q (or prefix partial) + later rows, in order
        Q0 = a.own_q[3 * n + 0];
        Q1 = a.own_q[3 * n + 1];
        Q2 = a.own_q[3 * n + 2];
        const int j0 = a.own_rp[n], j1 = a.own_rp[n + 1];
        for (int j = j0; j < j1; ++j) {
            const long long r = a.own_ridx[j];
            Q0 += a.own_rows[3 * r + 0];
            Q1 += a.own_rows[3 * r + 1];
            Q2 += a.own_rows[3 * r + 2];
        }
    } else if (MODE == 0) {
        const int4 lo = reinterpret_cast<const int4*>(a.inc8)[2 * n];
        const int4 hi = reinterpret_cast<const int4*>(a.inc8)[2 * n + 1];
        const int idx[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
        double f[8][3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const double* p = a.fe + idx[j];
            f[j][0] = p[0];
            f[j][1] = p[1];
            f[j][2] = p[2];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            Q0 += f[j][0];
            Q1 += f[j][1];
            Q2 += f[j][2];
        }
    } else {
        const int j0 = a.inc_ptr[n], j1 = a.inc_ptr[n + 1];
        for (int j = j0; j < j1; ++j) {
            const double* f = a.fe + a.inc[j];
            Q0 += f[0];
            Q1 += f[1];
            Q2 += f[2];
        }
    }
    nodal_update<BCF>(a, n, in, Q0, Q1, Q2);
}

template <bool FEXT, bool BCF>
static void launch_nodal_m(const NodalArgs& a, unsigned grid, hipStream_t s) {
    if (a.qbuf)
        hipLaunchKernelGGL((k_nodal<2, FEXT, BCF>), dim3(grid), dim3(kBlock), 0, s, a);
    else if (a.own_q)
        hipLaunchKernelGGL((k_nodal<3, FEXT, BCF>), dim3(grid), dim3(kBlock), 0, s, a);
    else if (a.inc8)
        hipLaunchKernelGGL((k_nodal<0, FEXT, BCF>), dim3(grid), dim3(kBlock), 0, s, a);
    else
        hipLaunchKernelGGL((k_nodal<1, FEXT, BCF>), dim3(grid), dim3(kBlock), 0, s, a);
}

hipError_t launch_nodal(const NodalArgs& a, hipStream_t s) {
    if (a.nN <= 0) return hipSuccess;
    const unsigned grid = (unsigned)((a.nN + kBlock - 1) / kBlock);
    if (a.bc_of_node) {
        if (a.fext)
            launch_nodal_m<true, true>(a, grid, s);
        else
            launch_nodal_m<false, true>(a, grid, s);
    } else {
        if (a.fext)
            launch_nodal_m<true, false>(a, grid, s);
        else
            launch_nodal_m<false, false>(a, grid, s);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Prescribed displacements (v2/HAKAI_j.jl:585-617). Entries are pre-resolved on the host so that
// each dof appears once with its LAST writer's (group, value), which is what the reference's
// in-order overwrite leaves behind.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void k_bc(BCArgs a) {
    if (poisoned(a.poison)) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    a.out[a.dof[i]] = bc_value(a, i);
}

hipError_t launch_bc(const BCArgs& a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_bc, dim3((a.n + kBlock - 1) / kBlock), dim3(kBlock), 0, s, a);
    return hipGetLastError();
}

__global__ void k_set_step(double* slot, double t_prev) {
    if (threadIdx.x == 0) *slot = t_prev;
}

// Timing aid (hakai_step_group with group_serial 2): one wave sleeps a fixed number of s_sleep
// rounds (no memory access, always exits), so the host can enqueue a whole phase behind it and the
// phase then runs back to back instead of at the host's enqueue pace.
__global__ void k_hold(int rounds) {
    for (int i = 0; i < rounds; ++i) __builtin_amdgcn_s_sleep(127);
}

hipError_t launch_hold(int rounds, hipStream_t s) {
    hipLaunchKernelGGL(k_hold, dim3(1), dim3(64), 0, s, rounds);
    return hipGetLastError();
}

hipError_t launch_set_step(double* slot, double t_prev, hipStream_t s) {
    hipLaunchKernelGGL(k_set_step, dim3(1), dim3(64), 0, s, slot, t_prev);
    return hipGetLastError();
}

// Q of every node from fe (for downloads): the same additions as k_nodal MODE 1, so the same bits.
__global__ void k_gather_q(const int* __restrict__ ptr, const int* __restrict__ inc, const double* __restrict__ fe,
                           double* Q, long long nN) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nN) return;
    double q0 = 0.0, q1 = 0.0, q2 = 0.0;
    for (int j = ptr[n]; j < ptr[n + 1]; ++j) {
        const double* f = fe + inc[j];
        q0 += f[0];
        q1 += f[1];
        q2 += f[2];
    }
    Q[3 * n + 0] = q0;
    Q[3 * n + 1] = q1;
    Q[3 * n + 2] = q2;
}

hipError_t launch_gather_q(const int* inc_ptr, const int* inc, const double* fe, double* Q, long long nN,
                           hipStream_t s) {
    if (nN <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_q, dim3((unsigned)((nN + 255) / 256)), dim3(256), 0, s, inc_ptr, inc, fe, Q, nN);
    return hipGetLastError();
}

// Q of every node from the owner-computed sums (for downloads, and for handing the nodal update
// a Q when owner assembly stops being used): own_q[n] + its exported rows, in element order --
// the same additions as k_nodal MODE 3, so the same bits.
__global__ void k_own_q(const double* __restrict__ own_q, const int* __restrict__ rp, const int* __restrict__ ridx,
                        const double* __restrict__ rows, double* Q, long long nN) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nN) return;
    double q0 = own_q[3 * n + 0], q1 = own_q[3 * n + 1], q2 = own_q[3 * n + 2];
    for (int j = rp[n]; j < rp[n + 1]; ++j) {
        const long long r = ridx[j];
        q0 += rows[3 * r + 0];
        q1 += rows[3 * r + 1];
        q2 += rows[3 * r + 2];
    }
    Q[3 * n + 0] = q0;
    Q[3 * n + 1] = q1;
    Q[3 * n + 2] = q2;
}

hipError_t launch_own_q(const double* own_q, const int* rp, const int* ridx, const double* rows, double* Q,
                        long long nN, hipStream_t s) {
    if (nN <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_own_q, dim3((unsigned)((nN + 255) / 256)), dim3(256), 0, s, own_q, rp, ridx, rows, Q, nN);
    return hipGetLastError();
}

}  // namespace hk
