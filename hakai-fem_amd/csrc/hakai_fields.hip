// hakai_fields.hip -- upload, download and output helpers of the gfx950 kernels, all off the per-step
// path: layout transposes, state reset, stand-alone triaxiality, node averages for output.
// k_triax_aos has no contraction pragma of its own: it is compiled as the Makefile says.
#include <hip/hip_runtime.h>

#include "hakai_kernels.hpp"

namespace hk {

__global__ void k_aos_to_soa6(const double* __restrict__ aos, double* __restrict__ soa, long long n, long long ld) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 6 * n) return;
    const long long g = i / 6, c = i % 6;
    soa[c * ld + g] = aos[i];
}
__global__ void k_soa_to_aos6(const double* __restrict__ soa, double* __restrict__ aos, long long n, long long ld) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 6 * n) return;
    const long long g = i / 6, c = i % 6;
    aos[i] = soa[c * ld + g];
}

hipError_t launch_aos_to_soa6(const double* aos, double* soa, long long nGP, long long ld, hipStream_t s) {
    if (nGP <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_aos_to_soa6, dim3((unsigned)((6 * nGP + 255) / 256)), dim3(256), 0, s, aos, soa, nGP, ld);
    return hipGetLastError();
}
hipError_t launch_soa_to_aos6(const double* soa, double* aos, long long nGP, long long ld, hipStream_t s) {
    if (nGP <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_soa_to_aos6, dim3((unsigned)((6 * nGP + 255) / 256)), dim3(256), 0, s, soa, aos, nGP, ld);
    return hipGetLastError();
}

__global__ void k_reset_gp(double* stress, double* strain, double* eqps, double* yield, double* triax, int* flag,
                           const int* mat, const DevMat* mats, long long nE, long long nEp, long long ld) {
    const long long g = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= 8 * nEp) return;
    const long long e = g >> 3;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        stress[c * ld + g] = 0.0;
        strain[c * ld + g] = 0.0;
    }
    eqps[g] = 0.0;
    triax[g] = 0.0;
    const DevMat* M = mats + mat[e];
    yield[g] = (e < nE && M->npp > 0) ? M->yield0 : 0.0;
    if ((g & 7) == 0) flag[e] = e < nE ? 1 : 0;  // padding elements behave as deleted
}

hipError_t launch_reset_gp(double* stress, double* strain, double* eqps, double* yield, double* triax, int* flag,
                           const int* mat, const DevMat* mats, long long nE, long long nEp, long long ld, hipStream_t s) {
    if (nEp <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_reset_gp, dim3((unsigned)((8 * nEp + 255) / 256)), dim3(256), 0, s, stress, strain, eqps,
                       yield, triax, flag, mat, mats, nE, nEp, ld);
    return hipGetLastError();
}

__global__ void k_triax_aos(const double* __restrict__ st, double* __restrict__ tx, long long n) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* s = st + 6 * i;
    const double mean = (s[0] + s[1] + s[2]) / 3.0;
    const double a01 = s[0] - s[1], a12 = s[1] - s[2], a20 = s[2] - s[0];
    const double oeq = sqrt(0.5 * (a01 * a01 + a12 * a12 + a20 * a20) + 3.0 * (s[3] * s[3] + s[4] * s[4] + s[5] * s[5]));
    tx[i] = (oeq < 1e-10) ? 0.0 : mean / oeq;
}

hipError_t launch_triax_aos(const double* stress_aos, double* triax, long long nGP, hipStream_t s) {
    if (nGP <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_triax_aos, dim3((unsigned)((nGP + 255) / 256)), dim3(256), 0, s, stress_aos, triax, nGP);
    return hipGetLastError();
}

// cal_node_stress_strain (v2/HAKAI_j.jl:3408-3486): element averages (sequential over the 8 GPs),
// summed per node in element order, divided by the incidence count; Mises from the node average.
__global__ void k_node_average(const int* __restrict__ ptr, const int* __restrict__ inc, const double* __restrict__ st,
                               const double* __restrict__ sn, const double* __restrict__ eq,
                               const double* __restrict__ tx, long long ld, long long nN, double* ns, double* nn,
                               double* neq, double* nmis, double* ntx) {
#pragma clang fp contract(off)
    const long long n = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= nN) return;
    double as[6] = {0, 0, 0, 0, 0, 0}, an[6] = {0, 0, 0, 0, 0, 0}, ae = 0.0, at = 0.0;
    const int j0 = ptr[n], j1 = ptr[n + 1];
    for (int j = j0; j < j1; ++j) {
        const long long e = inc[j] >> 3;
        for (int c = 0; c < 6; ++c) {
            double s1 = 0.0, s2 = 0.0;
            for (int k = 0; k < 8; ++k) {
                s1 += st[c * ld + 8 * e + k];
                s2 += sn[c * ld + 8 * e + k];
            }
            as[c] += s1 / 8;
            an[c] += s2 / 8;
        }
        double s1 = 0.0, s2 = 0.0;
        for (int k = 0; k < 8; ++k) {
            s1 += eq[8 * e + k];
            s2 += tx[8 * e + k];
        }
        ae += s1 / 8;
        at += s2 / 8;
    }
    const double cnt = (double)(j1 - j0);
    for (int c = 0; c < 6; ++c) {
        as[c] /= cnt;
        an[c] /= cnt;
    }
    ae /= cnt;
    at /= cnt;
    if (ns)
        for (int c = 0; c < 6; ++c) ns[6 * n + c] = as[c];
    if (nn)
        for (int c = 0; c < 6; ++c) nn[6 * n + c] = an[c];
    if (neq) neq[n] = ae;
    if (ntx) ntx[n] = at;
    if (nmis) {
        const double ox = as[0], oy = as[1], oz = as[2], txy = as[3], tyz = as[4], txz = as[5];
        nmis[n] = sqrt(0.5 * ((ox - oy) * (ox - oy) + (oy - oz) * (oy - oz) + (ox - oz) * (ox - oz) +
                              6 * (txy * txy + tyz * tyz + txz * txz)));
    }
}

hipError_t launch_node_average(const int* inc_ptr, const int* inc, const double* stress, const double* strain,
                               const double* eqps, const double* triax, long long ld, long long nN,
                               double* node_stress, double* node_strain, double* node_eqps, double* node_mises,
                               double* node_triax, hipStream_t s) {
    if (nN <= 0) return hipSuccess;
    hipLaunchKernelGGL(k_node_average, dim3((unsigned)((nN + 255) / 256)), dim3(256), 0, s, inc_ptr, inc, stress,
                       strain, eqps, triax, ld, nN, node_stress, node_strain, node_eqps, node_mises, node_triax);
    return hipGetLastError();
}

}  // namespace hk
