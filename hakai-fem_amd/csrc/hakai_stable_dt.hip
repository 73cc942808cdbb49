// hakai_stable_dt.hip -- the stable-time-step diagnostic (hakai_stable_dt, include/hakai_hip.h): per
// active element the conventional estimate dt_est = L / c and dt_safe, a guaranteed lower bound of
// the critical step of the ELASTIC B-bar stiffness against the lumped mass (the plastic tangent is
// no stiffer; the penalty stiffness of contact is outside it), both at the current configuration,
// reduced on the device to their minima, the elements that attain them and three counts. Off the
// hot path, like k_negjac: a kernel of its own, launched only by hakai_stable_dt; it reads coord,
// the current displacement, the connectivity, the flags and the material ids and writes only its own
// scratch, so nothing a step reads changes and captured graphs stay valid (no graph_invalidate).
// The element's arithmetic is hakai_stable_dt_elem.hpp, compiled here without contraction.
//
// k_stable_dt: the project's mapping -- 8 lanes per element, lane k = Gauss point k, 32 elements per
// 256-thread block. Lane k gathers node k's coord and u (the 8 lanes of an element read its 8 nodes
// in one instruction), the positions go round the 8-lane group by wave shuffles (no LDS, no
// barrier), every lane forms the 26 terms of its Gauss point and the sums over the Gauss points are
// the xor-1/2/4 butterfly, the bits of the header's pairwise tree: V and sum s_k on every lane
// (allreduce8), the 24 gradient sums as a reduce-scatter that leaves node i's three on lane i
// (sum_scatter8), which takes node i's share of sum g~^2 -- 3 divisions per lane instead of 24.
// V0 is summed in Gauss-point order from the lanes' determinants, as hakai_lumped_mass does; it is a
// constant of the model, so a context's first call forms and stores it (k_stable_dt<false>) and the
// later calls read it (k_stable_dt<true>, a fifth less arithmetic), the same bits.
// Materials come from a per-call table in global memory: any number of them.
// The gather, the exchanges and the sums are hakai_stable_dt_dev.hpp's elem_sums, which k_mass_need
// (hakai_mass_scale.hip) shares. On a context with selective mass scaling in force
// (hakai_mass_scale) k_stable_dt<true, true> runs: stable_finish_added with the element's added mass
// instead of stable_finish; without it the two instantiations above, unchanged.
// Per block: the minimum of each quantity with the lowest element id among equal values, and the
// counts, combined over the wave with shuffles and ballots and over the four waves through 4 LDS
// slots; one partial per block. k_stable_dt_finish, one block in a second launch, combines the
// partials: the launch boundary is the only hand-off between workgroups (no atomics, flags or
// spins). A minimum with a lowest-id tie rule and integer counts are exact and order-free: the same
// result for every grid.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <memory>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_device.hpp"
#include "hakai_internal.hpp"
#include "hakai_mass_scale.hpp"
#include "hakai_mass_scale_elem.hpp"
#include "hakai_stable_dt.hpp"
#include "hakai_stable_dt_dev.hpp"
#include "hakai_stable_dt_elem.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace {

using hk::sdt::kEPB;
using hk::sdt::kNone;
using hk::sdt::kThreads;
using hk::sdt::take_min;

// A partial result (a wave's, a block's); element ids local and 0-based.
struct Part {
    double est, safe;
    int e_est, e_safe;
    int n_active, n_est, n_safe, pad;
};

// What the finish kernel leaves for the host.
struct Result {
    double est, safe;
    long long e_est, e_safe;
    long long n_active, n_est, n_safe;
};

struct Args {
    const double* coord;
    const double* u;
    const int* conn;
    const int* flag;
    const int* mat;
    const hk::StableMat* mats;
    long long nE;
    double d_time;       // counts against it (<= 0: none)
    double* est_elem;    // [nE] or null
    double* safe_elem;   // [nE] or null
    Part* part;          // [ceil(nE / 32)]
    double* v0;          // [nE] the elements' V0: written by the first call, read by the later ones
    const double* added; // [nE] selective mass scaling's added mass (k_stable_dt<true, true> only)
};

// kHaveV0 false: a context's first call, which also forms every element's V0 (a constant of the
// model) and stores it; true: the later calls, which read it -- the same bits either way.
// kAdded: selective mass scaling is in force (it has formed V0), the element's mass is m0 + added.
template <bool kHaveV0, bool kAdded>
__global__ __launch_bounds__(kThreads) void k_stable_dt(Args a) {
    const int tid = threadIdx.x, k = tid & 7;
    const long long e = (long long)blockIdx.x * kEPB + (tid >> 3);
    const bool in = e < a.nE;
    const long long ee = in ? e : a.nE - 1;  // lanes past the end compute the last element and drop it
    const bool active = in && a.flag[ee] == 1;
    hk::sdt::ElemSums s;
    hk::sdt::elem_sums<kHaveV0>(a.coord, a.u, a.conn, a.v0, ee, k, in, s);
    double est, safe;
    if constexpr (kAdded)
        hk::stable_finish_added(s.V, s.gg, s.ss, s.V0, hk::stable_amax(s.x), a.mats[a.mat[ee]], a.added[ee], &est,
                                &safe);
    else
        hk::stable_finish(s.V, s.gg, s.ss, s.V0, hk::stable_amax(s.x), a.mats[a.mat[ee]], &est, &safe);
    if (!active) {
        est = HUGE_VAL;
        safe = HUGE_VAL;
    }
    if (in && k == 0) {
        if (a.est_elem) a.est_elem[e] = est;
        if (a.safe_elem) a.safe_elem[e] = safe;
    }
    // the wave's 8 elements: counts from ballots of the elements' first lanes, minima by shuffles
    // (every lane of an element holds the same pair)
    const bool lead = active && k == 0, cnt = lead && a.d_time > 0.0;
    const int n_active = __popcll(__ballot(lead));
    const int n_est = __popcll(__ballot(cnt && est < a.d_time));
    const int n_safe = __popcll(__ballot(cnt && safe < a.d_time));
    int ie = active ? (int)e : kNone, is = ie;
#pragma unroll
    for (int m = 8; m < 64; m <<= 1) {
        const double oe = __shfl_xor(est, m), os = __shfl_xor(safe, m);
        const int oie = __shfl_xor(ie, m), ois = __shfl_xor(is, m);
        take_min(est, ie, oe, oie);
        take_min(safe, is, os, ois);
    }
    __shared__ Part w[kThreads / 64];
    if ((tid & 63) == 0) {
        Part p;
        p.est = est;
        p.safe = safe;
        p.e_est = ie;
        p.e_safe = is;
        p.n_active = n_active;
        p.n_est = n_est;
        p.n_safe = n_safe;
        p.pad = 0;
        w[tid >> 6] = p;
    }
    __syncthreads();
    if (tid == 0) {
        Part p = w[0];
#pragma unroll
        for (int q = 1; q < kThreads / 64; ++q) {
            take_min(p.est, p.e_est, w[q].est, w[q].e_est);
            take_min(p.safe, p.e_safe, w[q].safe, w[q].e_safe);
            p.n_active += w[q].n_active;
            p.n_est += w[q].n_est;
            p.n_safe += w[q].n_safe;
        }
        a.part[blockIdx.x] = p;
    }
}

// One block: thread t takes the partials t, t + 256, ..., then a tree over the 256 threads in LDS.
__global__ __launch_bounds__(kThreads) void k_stable_dt_finish(const Part* part, long long nb, Result* out) {
    __shared__ Result s[kThreads];
    const int tid = threadIdx.x;
    Result r;
    r.est = r.safe = HUGE_VAL;
    r.e_est = r.e_safe = kNone;
    r.n_active = r.n_est = r.n_safe = 0;
    for (long long i = tid; i < nb; i += kThreads) {
        const Part p = part[i];
        take_min(r.est, r.e_est, p.est, (long long)p.e_est);
        take_min(r.safe, r.e_safe, p.safe, (long long)p.e_safe);
        r.n_active += p.n_active;
        r.n_est += p.n_est;
        r.n_safe += p.n_safe;
    }
    s[tid] = r;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            Result o = s[tid + h];
            take_min(s[tid].est, s[tid].e_est, o.est, o.e_est);
            take_min(s[tid].safe, s[tid].e_safe, o.safe, o.e_safe);
            s[tid].n_active += o.n_active;
            s[tid].n_est += o.n_est;
            s[tid].n_safe += o.n_safe;
        }
        __syncthreads();
    }
    if (tid == 0) *out = s[0];
}

}  // namespace

namespace hkc {

// Scratch of the diagnostic, sized for the context's model at the first call: the block partials,
// the result, the material table (filled per call: it depends on mass_scaling) and, once a caller
// asks for them, the per-element arrays.
struct StableDt {
    DevBuf<Part> d_part;
    DevBuf<Result> d_res;
    DevBuf<hk::StableMat> d_mats;
    DevBuf<double> d_v0;                // [nE] V0 of every element, valid once a call has completed
    bool have_v0 = false;
    DevBuf<double> d_est, d_safe;
    std::vector<hk::StableMat> h_mats;  // the table of the call in flight (the copy reads it)
};

void stable_dt_destroy(hakai_ctx* c) {
    if (!c || !c->sdt) return;
    (void)hipSetDevice(c->device);
    delete c->sdt;
    c->sdt = nullptr;
}

// The scratch at the first call, and this call's material table on its way to the device (ordered on
// the context's stream; h_mats holds it until the caller synchronises).
int stable_dt_prepare(hakai_ctx* c, double mass_scaling) {
    const long long nE = c->nE, nb = (nE + kEPB - 1) / kEPB;
    if (!c->sdt) {
        std::unique_ptr<StableDt> s(new StableDt());
        HIPCHK(s->d_part.alloc((size_t)nb));
        HIPCHK(s->d_res.alloc(1));
        HIPCHK(s->d_mats.alloc((size_t)c->nmat));
        HIPCHK(s->d_v0.alloc((size_t)nE));
        c->sdt = s.release();
    }
    StableDt* s = c->sdt;
    s->h_mats.resize((size_t)c->nmat);
    for (int i = 0; i < c->nmat; ++i)
        s->h_mats[i] = hk::stable_mat(c->h_young[i], c->h_poisson[i], c->h_mats[i].density, mass_scaling);
    HIPCHK(hipMemcpyAsync(s->d_mats, s->h_mats.data(), (size_t)c->nmat * sizeof(hk::StableMat), hipMemcpyHostToDevice,
                          c->stream));
    return 0;
}

const hk::StableMat* stable_dt_mats(const hakai_ctx* c) { return c->sdt ? c->sdt->d_mats : nullptr; }
double* stable_dt_v0(const hakai_ctx* c, bool* have) {
    *have = c->sdt && c->sdt->have_v0;
    return c->sdt ? c->sdt->d_v0 : nullptr;
}
void stable_dt_v0_formed(hakai_ctx* c) {
    if (c->sdt) c->sdt->have_v0 = true;
}

}  // namespace hkc

extern "C" int hakai_stable_dt(hakai_ctx* c, double mass_scaling, double d_time, hakai_stable_dt_t* out,
                               double* dt_est_elem, double* dt_safe_elem) {
    if (!c || !out) return fail(HAKAI_ERR_ARG, "stable_dt: null");
    if (!(mass_scaling > 0.0) || std::isinf(mass_scaling))
        return fail(HAKAI_ERR_ARG, "stable_dt: mass_scaling %g (must be positive and finite)", mass_scaling);
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "stable_dt without state");
    HIPCHK(hipSetDevice(c->device));
    const long long nE = c->nE, nb = (nE + kEPB - 1) / kEPB;
    hakai_stable_dt_t r;
    r.dt_est = r.dt_safe = HUGE_VAL;
    r.element_est = r.element_safe = 0;
    r.n_active = r.n_est_below = r.n_safe_below = 0;
    if (nE > 0) {
        if (int rc = hkc::stable_dt_prepare(c, mass_scaling)) return rc;
        hkc::StableDt* s = c->sdt;
        if (dt_est_elem && !s->d_est) HIPCHK(s->d_est.alloc((size_t)nE));
        if (dt_safe_elem && !s->d_safe) HIPCHK(s->d_safe.alloc((size_t)nE));
        hipStream_t st = c->stream;
        Args a;
        a.coord = c->d_coord;
        a.u = c->d_u[c->sv.cur];
        a.conn = c->d_conn;
        a.flag = c->d_flag;
        a.mat = c->d_mat;
        a.mats = s->d_mats;
        a.nE = nE;
        a.d_time = d_time;
        a.est_elem = dt_est_elem ? s->d_est : nullptr;
        a.safe_elem = dt_safe_elem ? s->d_safe : nullptr;
        a.part = s->d_part;
        a.v0 = s->d_v0;
        a.added = hkc::mass_scale_added(c);
        if (a.added && s->have_v0)
            hipLaunchKernelGGL((k_stable_dt<true, true>), dim3((unsigned)nb), dim3(kThreads), 0, st, a);
        else if (a.added)
            return fail(HAKAI_ERR_STATE, "stable_dt: mass scaling in force without the elements' V0");
        else if (s->have_v0)
            hipLaunchKernelGGL((k_stable_dt<true, false>), dim3((unsigned)nb), dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL((k_stable_dt<false, false>), dim3((unsigned)nb), dim3(kThreads), 0, st, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_stable_dt_finish, dim3(1), dim3(kThreads), 0, st, (const Part*)s->d_part, nb, s->d_res);
        HIPCHK(hipGetLastError());
        Result h;
        HIPCHK(hipMemcpyAsync(&h, s->d_res, sizeof h, hipMemcpyDeviceToHost, st));
        if (dt_est_elem)
            HIPCHK(hipMemcpyAsync(dt_est_elem, s->d_est, (size_t)nE * sizeof(double), hipMemcpyDeviceToHost, st));
        if (dt_safe_elem)
            HIPCHK(hipMemcpyAsync(dt_safe_elem, s->d_safe, (size_t)nE * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        s->have_v0 = true;
        r.n_active = h.n_active;
        r.n_est_below = h.n_est;
        r.n_safe_below = h.n_safe;
        if (h.e_est != kNone) {  // (an id is taken with every comparable value, +inf included)
            r.dt_est = h.est;
            r.element_est = h.e_est + 1 + c->elem_offset;
        }
        if (h.e_safe != kNone) {
            r.dt_safe = h.safe;
            r.element_safe = h.e_safe + 1 + c->elem_offset;
        }
    }
    *out = r;
    return 0;
}
