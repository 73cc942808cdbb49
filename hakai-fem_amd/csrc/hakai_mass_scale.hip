// hakai_mass_scale.hip -- selective mass scaling (hakai_mass_scale, include/hakai_hip.h): mass is
// added to the nodes of the elements whose guaranteed stable step dt_safe is below a target, as much
// as brings it there, and to no other element. Off the hot path: three kernels launched only by
// hakai_mass_scale. They write the context's nodal mass d_mass in place -- the buffer every kernel of
// a step reads (the nodal update, the interface fixes, gravity and walls, history, contact) -- so no
// kernel argument and no launch sequence changes and captured step graphs stay valid (no
// graph_invalidate); a step after the call reads the new mass in stream and in graph mode alike.
// The element's rule is hakai_mass_scale_elem.hpp, compiled here without contraction.
//
// k_mass_need: the project's mapping, shared with k_stable_dt through hakai_stable_dt_dev.hpp -- 8
// lanes per element, lane k = Gauss point k, 32 elements per 256-thread block, positions by wave
// shuffles, sums by allreduce8 and the reduce-scatter. V0 comes from the stable-step scratch (formed
// and stored here if no call has yet: k_mass_need<false>). It writes added[e] and one partial per
// block: counts from ballots, the largest mass factor and the smallest dt_safe after the call with
// the lowest element id among equal values, and the block's subtree of mass_added = sum_e 8 added_e.
// That sum is ONE fixed binary tree in element order (neighbours first; a subtree without a sibling
// moves up unchanged): xor-8/16/32 shuffles over a wave's 8 elements, (w0 + w1) + (w2 + w3) over the
// block's waves, elements past the end as +0.0 (x + 0.0 is x for every x >= +0.0, so padding is the
// same bits as "moves up unchanged"). k_mass_need_finish, one block in a second launch, combines the
// partials -- the launch boundary is the only hand-off between workgroups, no atomics, flags or
// spins -- and continues the same tree over the blocks' sums, level by level in place. The result is
// the same bits for every grid.
// k_mass_gather: one thread per node, M_n = M0_n + sum of added_e over the node's incidences in
// ascending (8e + i) order of d_inc_row, every addition rounded once (hakai_lumped_mass's order);
// M0 is the uploaded mass, copied at the context's first call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <memory>

#include "../../include/hakai_hip.h"
#include "hakai_device.hpp"
#include "hakai_history.hpp"
#include "hakai_internal.hpp"
#include "hakai_mass_scale.hpp"
#include "hakai_mass_scale_elem.hpp"
#include "hakai_stable_dt.hpp"
#include "hakai_stable_dt_dev.hpp"

using hkc::fail;
using hkc::hip_fail;

namespace {

using hk::sdt::kEPB;
using hk::sdt::kNone;
using hk::sdt::kThreads;
using hk::sdt::take_max;
using hk::sdt::take_min;

// A partial result (a wave's, a block's); element ids local and 0-based.
struct Part {
    double fac, safe, sum;
    int e_fac, e_safe;
    int n_active, n_scaled, n_changed, n_capped, n_unfix, pad;
};

// What the finish kernel leaves for the host.
struct Result {
    double fac, safe, sum;
    long long e_fac, e_safe;
    long long n_active, n_scaled, n_changed, n_capped, n_unfix;
};

struct Args {
    const double* coord;
    const double* u;
    const int* conn;
    const int* flag;
    const int* mat;
    const hk::StableMat* mats;
    long long nE;
    double half;        // (0.5 * dt_target) / safety
    double max_factor;  // >= 1, +inf: no cap
    double* added;      // [nE] read (added_prev) and written
    Part* part;         // [ceil(nE / 32)]
    double* v0;         // [nE] the stable-step scratch's V0
};

template <bool kHaveV0>
__global__ __launch_bounds__(kThreads) void k_mass_need(Args a) {
    const int tid = threadIdx.x, k = tid & 7;
    const long long e = (long long)blockIdx.x * kEPB + (tid >> 3);
    const bool in = e < a.nE;
    const long long ee = in ? e : a.nE - 1;  // lanes past the end compute the last element and drop it
    const bool active = in && a.flag[ee] == 1;
    hk::sdt::ElemSums s;
    hk::sdt::elem_sums<kHaveV0>(a.coord, a.u, a.conn, a.v0, ee, k, in, s);
    const hk::StableMat m = a.mats[a.mat[ee]];
    const double prev = a.added[ee];
    int status;
    const double need = hk::mass_need(s.V, s.gg, s.ss, s.V0, m, a.half, a.max_factor, prev, &status);
    const double add = active ? need : prev;  // a deleted element is untouched and keeps its mass
    if (in && k == 0) a.added[e] = add;
    double est, safe;
    hk::stable_finish_added(s.V, s.gg, s.ss, s.V0, hk::stable_amax(s.x), m, add, &est, &safe);
    double fac = -HUGE_VAL;
    int ifac = kNone, is = kNone;
    if (active && s.V0 > 0.0) {
        fac = hk::mass_factor(s.V0, m, add);
        ifac = (int)e;
    }
    if (active)
        is = (int)e;
    else
        safe = HUGE_VAL;
    double sum = in ? 8.0 * add : 0.0;
    // the wave's 8 elements: counts from ballots of the elements' first lanes, extrema and the sum's
    // tree by shuffles (every lane of an element holds the same values)
    const bool lead = active && k == 0;
    const int n_active = __popcll(__ballot(lead));
    const int n_scaled = __popcll(__ballot(in && k == 0 && add > 0.0));
    const int n_changed = __popcll(__ballot(lead && add > prev));
    const int n_capped = __popcll(__ballot(lead && status == hk::kMassCapped));
    const int n_unfix = __popcll(__ballot(lead && status == hk::kMassUnfixable));
#pragma unroll
    for (int w = 8; w < 64; w <<= 1) {
        const double of = __shfl_xor(fac, w), os = __shfl_xor(safe, w);
        const int oif = __shfl_xor(ifac, w), ois = __shfl_xor(is, w);
        take_max(fac, ifac, of, oif);
        take_min(safe, is, os, ois);
        sum = sum + __shfl_xor(sum, w);
    }
    __shared__ Part w[kThreads / 64];
    if ((tid & 63) == 0) {
        Part p;
        p.fac = fac;
        p.safe = safe;
        p.sum = sum;
        p.e_fac = ifac;
        p.e_safe = is;
        p.n_active = n_active;
        p.n_scaled = n_scaled;
        p.n_changed = n_changed;
        p.n_capped = n_capped;
        p.n_unfix = n_unfix;
        p.pad = 0;
        w[tid >> 6] = p;
    }
    __syncthreads();
    if (tid == 0) {
        Part p = w[0];
#pragma unroll
        for (int q = 1; q < kThreads / 64; ++q) {
            take_max(p.fac, p.e_fac, w[q].fac, w[q].e_fac);
            take_min(p.safe, p.e_safe, w[q].safe, w[q].e_safe);
            p.n_active += w[q].n_active;
            p.n_scaled += w[q].n_scaled;
            p.n_changed += w[q].n_changed;
            p.n_capped += w[q].n_capped;
            p.n_unfix += w[q].n_unfix;
        }
        p.sum = (w[0].sum + w[1].sum) + (w[2].sum + w[3].sum);
        a.part[blockIdx.x] = p;
    }
}

// One block: thread t takes the partials t, t + 256, ..., then a tree over the 256 threads in LDS
// (extrema with a lowest-id rule and integer counts: exact and order-free). The blocks' sums go up
// the fixed tree in place: at stride st, part[i].sum (i a multiple of 2 st) takes part[i + st].sum if
// that block exists and moves up unchanged if not.
__global__ __launch_bounds__(kThreads) void k_mass_need_finish(Part* part, long long nb, Result* out) {
    __shared__ Result s[kThreads];
    const int tid = threadIdx.x;
    Result r;
    r.fac = -HUGE_VAL;
    r.safe = HUGE_VAL;
    r.sum = 0.0;
    r.e_fac = r.e_safe = kNone;
    r.n_active = r.n_scaled = r.n_changed = r.n_capped = r.n_unfix = 0;
    for (long long i = tid; i < nb; i += kThreads) {
        const Part p = part[i];
        take_max(r.fac, r.e_fac, p.fac, (long long)p.e_fac);
        take_min(r.safe, r.e_safe, p.safe, (long long)p.e_safe);
        r.n_active += p.n_active;
        r.n_scaled += p.n_scaled;
        r.n_changed += p.n_changed;
        r.n_capped += p.n_capped;
        r.n_unfix += p.n_unfix;
    }
    s[tid] = r;
    __syncthreads();
    for (int h = kThreads / 2; h > 0; h >>= 1) {
        if (tid < h) {
            const Result o = s[tid + h];
            take_max(s[tid].fac, s[tid].e_fac, o.fac, o.e_fac);
            take_min(s[tid].safe, s[tid].e_safe, o.safe, o.e_safe);
            s[tid].n_active += o.n_active;
            s[tid].n_scaled += o.n_scaled;
            s[tid].n_changed += o.n_changed;
            s[tid].n_capped += o.n_capped;
            s[tid].n_unfix += o.n_unfix;
        }
        __syncthreads();
    }
    for (long long st = 1; st < nb; st <<= 1) {
        for (long long i = (long long)tid * 2 * st; i + st < nb; i += (long long)kThreads * 2 * st)
            part[i].sum = part[i].sum + part[i + st].sum;
        __syncthreads();
    }
    if (tid == 0) {
        s[0].sum = part[0].sum;
        *out = s[0];
    }
}

__global__ __launch_bounds__(kThreads) void k_mass_gather(const int* inc_ptr, const int* inc_row, const double* added,
                                                          const double* mass0, double* mass, long long nN) {
    const long long n = (long long)blockIdx.x * kThreads + threadIdx.x;
    if (n >= nN) return;
    double m = mass0[n];
    const int j1 = inc_ptr[n + 1];
    for (int j = inc_ptr[n]; j < j1; ++j) m = m + added[inc_row[j] >> 3];
    mass[n] = m;
}

}  // namespace

namespace hkc {

// Allocated at the context's first call, freed with the context, by a new model or by
// hakai_clear_mass_scale.
struct MassScale {
    DevBuf<double> d_added;     // [nE] mass added to each of the element's 8 nodes
    DevBuf<double> d_mass0;     // [nN] the uploaded nodal mass
    DevBuf<Part> d_part;
    DevBuf<Result> d_res;
    long long n_scaled = 0;     // elements with added > 0 after the last call
};

void mass_scale_destroy(hakai_ctx* c) {
    if (!c || !c->msc) return;
    (void)hipSetDevice(c->device);
    delete c->msc;
    c->msc = nullptr;
}

const double* mass_scale_added(const hakai_ctx* c) {
    return c->msc && c->msc->n_scaled > 0 ? c->msc->d_added : nullptr;
}

}  // namespace hkc

extern "C" int hakai_mass_scale(hakai_ctx* c, double mass_scaling, double dt_target, double safety,
                                double max_factor, hakai_mass_scale_t* out) {
    if (!c || !out) return fail(HAKAI_ERR_ARG, "mass_scale: null");
    if (!(mass_scaling > 0.0) || std::isinf(mass_scaling))
        return fail(HAKAI_ERR_ARG, "mass_scale: mass_scaling %g (must be positive and finite)", mass_scaling);
    if (!(dt_target > 0.0) || std::isinf(dt_target))
        return fail(HAKAI_ERR_ARG, "mass_scale: dt_target %g (must be positive and finite)", dt_target);
    if (!(safety > 0.0 && safety <= 1.0)) return fail(HAKAI_ERR_ARG, "mass_scale: safety %g (must be in (0, 1])", safety);
    if (!(max_factor >= 1.0)) return fail(HAKAI_ERR_ARG, "mass_scale: max_factor %g (must be >= 1)", max_factor);
    if (!c->state_ok) return fail(HAKAI_ERR_STATE, "mass_scale without state");
    if (c->comm)
        return fail(HAKAI_ERR_STATE, "mass_scale: a context with a communicator is refused (a shared node needs the "
                                     "neighbour rank's elements)");
    HIPCHK(hipSetDevice(c->device));
    const long long nE = c->nE, nN = c->nN, nb = (nE + kEPB - 1) / kEPB;
    hakai_mass_scale_t r;
    r.n_active = r.n_scaled = r.n_changed = r.n_capped = r.n_unfixable = 0;
    r.max_factor_reached = 1.0;
    r.element_factor = 0;
    r.mass_added = 0.0;
    r.dt_safe = HUGE_VAL;
    r.element_safe = 0;
    if (nE > 0) {
        hipStream_t st = c->stream;
        if (int rc = hkc::stable_dt_prepare(c, mass_scaling)) return rc;
        if (!c->msc) {
            std::unique_ptr<hkc::MassScale> s(new hkc::MassScale());
            HIPCHK(s->d_added.alloc((size_t)nE));
            HIPCHK(s->d_mass0.alloc((size_t)nN));
            HIPCHK(s->d_part.alloc((size_t)nb));
            HIPCHK(s->d_res.alloc(1));
            HIPCHK(hipMemsetAsync(s->d_added, 0, (size_t)nE * sizeof(double), st));
            HIPCHK(hipMemcpyAsync(s->d_mass0, c->d_mass, (size_t)nN * sizeof(double), hipMemcpyDeviceToDevice, st));
            c->msc = s.release();
        }
        hkc::MassScale* s = c->msc;
        bool have_v0 = false;
        Args a;
        a.coord = c->d_coord;
        a.u = c->d_u[c->sv.cur];
        a.conn = c->d_conn;
        a.flag = c->d_flag;
        a.mat = c->d_mat;
        a.mats = hkc::stable_dt_mats(c);
        a.nE = nE;
        a.half = hk::mass_half(dt_target, safety);
        a.max_factor = max_factor;
        a.added = s->d_added;
        a.part = s->d_part;
        a.v0 = hkc::stable_dt_v0(c, &have_v0);
        if (have_v0)
            hipLaunchKernelGGL(k_mass_need<true>, dim3((unsigned)nb), dim3(kThreads), 0, st, a);
        else
            hipLaunchKernelGGL(k_mass_need<false>, dim3((unsigned)nb), dim3(kThreads), 0, st, a);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_mass_need_finish, dim3(1), dim3(kThreads), 0, st, s->d_part, nb, s->d_res);
        HIPCHK(hipGetLastError());
        hipLaunchKernelGGL(k_mass_gather, dim3((unsigned)((nN + kThreads - 1) / kThreads)), dim3(kThreads), 0, st,
                           (const int*)c->d_inc_ptr, (const int*)c->d_inc_row, (const double*)s->d_added,
                           (const double*)s->d_mass0, c->d_mass, nN);
        HIPCHK(hipGetLastError());
        Result h;
        HIPCHK(hipMemcpyAsync(&h, s->d_res, sizeof h, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        hkc::stable_dt_v0_formed(c);
        s->n_scaled = h.n_scaled;
        r.n_active = h.n_active;
        r.n_scaled = h.n_scaled;
        r.n_changed = h.n_changed;
        r.n_capped = h.n_capped;
        r.n_unfixable = h.n_unfix;
        r.mass_added = h.sum;
        if (h.e_fac != kNone) {
            r.max_factor_reached = h.fac;
            r.element_factor = h.e_fac + 1 + c->elem_offset;
        }
        if (h.e_safe != kNone) {
            r.dt_safe = h.safe;
            r.element_safe = h.e_safe + 1 + c->elem_offset;
        }
    }
    *out = r;
    // the mass of some node has grown: the kinetic energy and the momentum of the history change
    // their meaning, so it starts again like after a state upload (a call that changed nothing
    // leaves the records alone)
    return r.n_changed > 0 ? hkc::history_restart(c) : 0;
}

extern "C" int hakai_mass_scale_get(hakai_ctx* c, double* elem_added, double* diag_M) {
    if (!c) return fail(HAKAI_ERR_ARG, "mass_scale_get: null");
    if (!c->model_ok) return fail(HAKAI_ERR_STATE, "mass_scale_get before upload_model");
    HIPCHK(hipSetDevice(c->device));
    const long long nE = c->nE, nN = c->nN;
    if (elem_added && nE > 0) {
        if (c->msc)
            HIPCHK(hipMemcpyAsync(elem_added, c->msc->d_added, (size_t)nE * sizeof(double), hipMemcpyDeviceToHost,
                                  c->stream));
        else
            for (long long e = 0; e < nE; ++e) elem_added[e] = 0.0;
    }
    if (diag_M)  // the nodes' masses first, then each spread over its three dofs from the back
        HIPCHK(hipMemcpyAsync(diag_M, c->d_mass, (size_t)nN * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (diag_M)
        for (long long n = nN - 1; n >= 0; --n) {
            const double m = diag_M[n];
            diag_M[3 * n + 2] = m;
            diag_M[3 * n + 1] = m;
            diag_M[3 * n] = m;
        }
    return 0;
}

extern "C" int hakai_clear_mass_scale(hakai_ctx* c) {
    if (!c) return fail(HAKAI_ERR_ARG, "clear_mass_scale: null");
    if (!c->msc) return 0;
    HIPCHK(hipSetDevice(c->device));
    const bool scaled = c->msc->n_scaled > 0;
    HIPCHK(hipMemcpyAsync(c->d_mass, c->msc->d_mass0, (size_t)c->nN * sizeof(double), hipMemcpyDeviceToDevice,
                          c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    hkc::mass_scale_destroy(c);
    return scaled ? hkc::history_restart(c) : 0;
}
