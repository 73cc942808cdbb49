// hakai_step.cpp -- the step driver of libhakai_hip.so: one explicit step (step_once), its capture
// into hipGraphs and their replay, the end-of-call contact overflow check with the rollback of the
// host's view (hkc::StepView, hakai_step_view.hpp), and the retry loops of hakai_step and
// hakai_step_group. Compiled without contraction, like hakai_capi.cpp.
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/hakai_hip.h"
#include "hakai_elem_history.hpp"
#include "hakai_history.hpp"
#include "hakai_internal.hpp"
#include "hakai_kernels.hpp"
#include "hakai_loads.hpp"

using hkc::fail;
using hkc::hip_fail;
using hkc::QSrc;

namespace hkc {
void graph_invalidate(hakai_ctx* c) {
    c->epoch++;
    c->tdev_next = -1;
}
void graph_free(hakai_ctx* c) {
    for (int g = 0; g < 2; ++g)
        for (int p = 0; p < 2; ++p)
            if (c->gr.exec[g][p]) {
                (void)hipGraphExecDestroy(c->gr.exec[g][p]);
                c->gr.exec[g][p] = nullptr;
                c->gr.epoch[g][p] = -1;
            }
}
}  // namespace hkc

// One explicit step (the loop body :497-764). With c->gr.trd set (graph capture) the kernels take
// the step number from the device counter and the element kernel advances it. Phase bits: the
// contact search parts A1, A2, A3 (hkc::contact_phase; one GPU: all of it in A1) and the rest
// (contact phase B, nodal, BCs, element, exchange). An in-process group with multi-GPU contact runs
// each part on every rank before the next (hakai_step_group).
enum { kPhaseA1 = 1, kPhaseRest = 2, kPhaseA2 = 4, kPhaseA3 = 8, kPhaseAll = 15 };
static int step_once(hakai_ctx* c, double t, double d_time, bool last, int phase = kPhaseAll) {
    hipStream_t s = c->stream;
    EventPair ep;
    if (c->contact) {  // contact force into external_force (:500-560), search parts
        const int part_bit[3] = {kPhaseA1, kPhaseA2, kPhaseA3};
        for (int part = 1; part <= 3; ++part) {
            if (!(phase & part_bit[part - 1]) || (part > 1 && !hkc::contact_multi(c))) continue;
            hkc::prof_begin(c, HAKAI_K_CONTACT, &ep);
            const int rc = hkc::contact_phase(c, part, t, d_time);
            hkc::prof_end(c, &ep);
            if (rc) return rc;
        }
    }
    if (!(phase & kPhaseRest)) return 0;
    const int par = c->sv.cur;  // graph mode: this step reads counter slot 1-par, writes slot par
    // owner-computed assembly: Q from the previous element step's sums (else the fe gather)
    const bool own = hkc::own_prepare(c);
    if (c->sv.q == QSrc::Own && !own) {  // switched off (or the lists could not be rebuilt)
        if (int r = hkc::own_materialize(c)) return r;
    }
    // nodal update (:562-567), Q from the previous step's element forces (:668-675)
    hk::NodalArgs na = hkc::nodal_args(c, d_time);
    const hk::BCArgs ba = hkc::bc_args(c, t, d_time);
    // one GPU, small mesh: the nodal kernel applies the BCs (multi-GPU redoes interface nodes
    // after the nodal kernel, so the BCs must come after that)
    // (fuse_bc 2: at any size; large meshes measured slower with the fe gather, see kFuseBcMaxNodes)
    const bool fuse_bc = c->bc.n > 0 && c->bc.d_of_node && c->fuse_bc && !c->comm &&
                         (c->nN <= kFuseBcMaxNodes || c->fuse_bc == 2);
    if (fuse_bc) {
        na.bc_of_node = c->bc.d_of_node;
        na.bc = ba;
    }
    int rc = 0;
    if (c->contact) {  // multi-GPU search: event exchange and force sums
        if (hkc::contact_multi(c)) {
            hkc::prof_begin(c, HAKAI_K_CONTACT_SUM, &ep);
            rc = hkc::contact_step_b(c);
            hkc::prof_end(c, &ep);
            if (rc) return rc;
        }
        na.fext = c->d_fext;
    }
    if (c->loads) {  // external loads, rigid walls: contact force + loads + walls -> the step's total external force
        if ((rc = hkc::loads_step(c, t, d_time, na.fext))) return rc;
        na.fext = c->d_ftot;  // = hkc::step_fext(c), what the interface fix takes too
    }
    rc = hkc::comm_pre_nodal(c);
    if (rc) return rc;
    if (c->hist && (rc = hkc::history_seed(c, na, s))) return rc;  // first step after a (re)start
    hkc::prof_begin(c, HAKAI_K_NODAL, &ep);
    HIPCHK(hk::launch_nodal(na, s));
    hkc::prof_end(c, &ep);
    // multi-GPU: interface nodes are redone with the cross-rank assembled Q
    hkc::CommFix fix;  // what the fix read: the history hook forms the same Q at the nodes this rank owns
    rc = hkc::comm_post_nodal(c, d_time, &fix);
    if (rc) return rc;
    // boundary conditions (:585-617)
    if (c->bc.n > 0 && !fuse_bc) {
        hkc::prof_begin(c, HAKAI_K_BC, &ep);
        HIPCHK(hk::launch_bc(ba, s));
        hkc::prof_end(c, &ep);
    }
    // history output: this step's sums, from the Q the nodal update consumed (still intact)
    if (c->hist && (rc = hkc::history_step(c, na, fix, t, c->gr.trd, s))) return rc;
    // element-set history: the record of state k = t - 1 (d_u[cur] and the Gauss-point state are still its)
    if (c->ehist && (rc = hkc::elem_history_step(c, t, c->gr.trd, s))) return rc;
    // element update (:662-667) + triaxiality (:677) + ductile deletion (:684-764), on the new
    // displacements: disp <- disp_new, disp_pre <- disp (:626-627)
    hk::ElemArgs ea = hkc::elem_args(c, 1 - par);
    ea.step_i = (int)t;
    if (own) hkc::own_elem_args(c, ea);
    if (c->gr.trd) {
        ea.t_rd = c->gr.trd;
        ea.t_wr = c->d_tstep + par;
    }
    hkc::prof_begin(c, HAKAI_K_ELEMENT, &ep);
    HIPCHK(hk::launch_element(ea, c->has_ductile, last, s));
    hkc::prof_end(c, &ep);
    c->sv.advance(own, last);
    c->own.steps += own ? 1 : 0;
    c->last_dt = d_time;
    rc = hkc::comm_post_element(c, (long long)t);
    if (rc) return rc;
    return hkc::contact_post_step(c);
}

// A run of steps starting at t can come from a graph: same launch sequence every step, nothing
// host-side that depends on the step (no multi-GPU exchange, no profiling events, no uploaded Q),
// and contact in its steady state. The step number comes from a device counter; every pointer
// argument is fixed for a given starting parity (cur), so one graph per parity serves the whole
// run. A failed capture leaves the context's host state advanced: the call returns the error.
static bool graph_eligible(const hakai_ctx* c, double t) {
    // (owner-computed assembly: only once the previous step left its sums, so every captured nodal
    // update reads them. own_wanted is current here: step_call ran own_prepare for this grid and
    // these tuning values, and nothing that changes either -- a tuning key, a model or interface
    // upload -- can run inside the call; an unprepared context reads as not wanted, and a live
    // sum then sends the step through step_once, which prepares)
    return c->graph && !c->comm && !c->prof && c->sv.q != QSrc::Buf && c->nE > 0 && hkc::contact_graph_ok(c, t) &&
           !hkc::history_needs_seed(c) && (c->sv.q == QSrc::Own) == hkc::own_wanted(c);
}

static int step_graph(hakai_ctx* c, double t, double d_time, int len) {
    hipStream_t s = c->stream;
    const int p0 = c->sv.cur;
    const int gi = len == 2 ? 1 : 0;
    hipGraphExec_t& ge = c->gr.exec[gi][p0];
    if (!c->d_tstep) HIPCHK(c->d_tstep.alloc(2));
    if (c->tdev_next != (long long)t) HIPCHK(hk::launch_set_step(c->d_tstep + (1 - p0), t - 1.0, s));
    if (ge && (c->gr.epoch[gi][p0] != c->epoch || c->gr.dt[gi][p0] != d_time || c->gr.len[gi][p0] != len)) {
        HIPCHK(hipStreamSynchronize(s));
        (void)hipGraphExecDestroy(ge);
        ge = nullptr;
    }
    if (!ge) {
        // capture the steps; their host-side state changes happen here, as in stream mode
        hipGraph_t g = nullptr;
        HIPCHK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
        int rc = 0;
        for (int k = 0; k < len && !rc; ++k) {
            c->gr.trd = c->d_tstep + (1 - c->sv.cur);
            rc = step_once(c, t + k, d_time, false);
        }
        c->gr.trd = nullptr;
        hipError_t e = hipStreamEndCapture(s, &g);
        if (rc) {
            if (g) (void)hipGraphDestroy(g);
            return rc;
        }
        if (e != hipSuccess) return hip_fail(e, "hipStreamEndCapture (step graph)");
        e = hipGraphInstantiate(&ge, g, nullptr, nullptr, 0);
        (void)hipGraphDestroy(g);
        if (e != hipSuccess) {
            ge = nullptr;
            return hip_fail(e, "hipGraphInstantiate (step graph)");
        }
        c->gr.epoch[gi][p0] = c->epoch;
        c->gr.dt[gi][p0] = d_time;
        c->gr.len[gi][p0] = len;
    } else {  // replay the host-side state changes of the captured steps
        hkc::contact_graph_advance(c, t + len - 1);
        // captured in the steady state: every step with owner assembly or none, never a call's last
        const bool own = c->sv.q == QSrc::Own;
        for (int k = 0; k < len; ++k) c->sv.advance(own, false);
        c->own.steps += own ? len : 0;
        c->last_dt = d_time;
    }
    HIPCHK(hipGraphLaunch(ge, s));
    c->tdev_next = (long long)t + len;
    c->graph_steps += len;
    return 0;
}

// The host's view of a context before a stepping call's first step (after any owner-assembly
// re-plan, which hands the last sums over unchanged): what an overflow on that step rolls back to.
struct CallSnap {
    hkc::StepView sv;
    bool comm_pending = false;  // the interface exchange the call's first nodal update consumes
    int comm_par = 0;
};
static CallSnap call_snap(const hakai_ctx* c) {
    CallSnap s;
    hkc::comm_pending_get(c, &s.comm_pending, &s.comm_par);
    s.sv = c->sv;
    return s;
}

// End of a stepping call: the contact overflow check. An overflow poisoned step p: the device's
// state-writing kernels of steps p.. were no-ops, so the device holds the state after step p-1;
// bring the host's view back to that step.
static int finish_call(hakai_ctx* c, double t_first, int64_t n_steps, const CallSnap& s0) {
    const int rc = hkc::contact_check(c);
    if (rc && c->contact) {
        int pz[2] = {0, 0};
        HIPCHK(hipMemcpy(pz, c->d_poison, sizeof pz, hipMemcpyDeviceToHost));
        if (pz[0]) {
            c->poison_step = pz[1];
            const long long good = (long long)pz[1] - (long long)t_first;  // steps of this call that ran
            const bool rolled = good >= 0 && good <= n_steps;
            if (rolled) {
                c->sv.rollback(s0.sv, good);
                hkc::comm_rollback(c, good > 0, (long long)pz[1] - 1, s0.comm_pending, s0.comm_par);
            }
            hkc::graph_invalidate(c);
            hkc::contact_after_overflow(c, c->sv.steps_done);
            // a poison step outside this call rolled nothing back: never run the call again from it
            if (!rolled) (void)hkc::contact_exchange_retry(c);
            HIPCHK(hipMemset(c->d_poison, 0, 2 * sizeof(int)));
            const std::string msg = hakai_last_error();
            return fail(rc, "%s; step %d was not applied: the state is that after step %d", msg.c_str(), pz[1],
                        pz[1] - 1);
        }
    }
    return rc;
}

static int step_call(hakai_ctx* c, double t_first, int64_t n_steps, double d_time) {
    (void)hkc::own_prepare(c);  // owner-assembly lists are built here, never inside a graph capture
    const CallSnap s0 = call_snap(c);
    int64_t it = 0;
    while (it < n_steps) {
        const double t = t_first + (double)it;
        int rc;
        // the call's last step stays in stream mode: it also stores triaxiality for downloads
        // (eligibility of step t implies it for the steps after it: step t clears every one-off
        // condition)
        const int len = (c->graph > 2 && it + c->graph < n_steps) ? c->graph : 2;
        if (c->graph && it + len < n_steps && graph_eligible(c, t)) {
            rc = step_graph(c, t, d_time, len);
            it += len;
        } else {
            rc = step_once(c, t, d_time, it == n_steps - 1);
            c->tdev_next = -1;
            ++it;
        }
        if (rc) return rc;
    }
    return finish_call(c, t_first, n_steps, s0);
}

static int step_group_call(hakai_ctx** ctxs, int32_t n, double t_first, int64_t n_steps, double d_time) {
    std::vector<CallSnap> s0(n);
    for (int r = 0; r < n; ++r) {
        (void)hkc::own_prepare(ctxs[r]);  // (re-plans here, as hakai_step does, not inside the first step)
        s0[r] = call_snap(ctxs[r]);
    }
    // per step: each contact part on every rank before the next part on any, then the rest
    const int phases[4] = {kPhaseA1, kPhaseA2, kPhaseA3, kPhaseRest};
    for (int64_t it = 0; it < n_steps; ++it) {
        const double t = t_first + (double)it;
        const bool last = it == n_steps - 1;
        for (int ph : phases)
            for (int r = 0; r < n; ++r) {
                // group_serial 2: the phase is enqueued behind a fixed sleep (≈0.3 ms), so its kernels
                // run back to back as in a pipelined run, not at the host's enqueue pace
                if (ctxs[0]->group_serial == 2) HIPCHK(hk::launch_hold(96, ctxs[r]->stream));
                if (int rc = step_once(ctxs[r], t, d_time, last, ph)) return rc;
                if (ph == kPhaseRest) ctxs[r]->tdev_next = -1;
                if (ctxs[0]->group_serial) HIPCHK(hipStreamSynchronize(ctxs[r]->stream));
            }
    }
    int first = 0;
    for (int r = 0; r < n; ++r) {
        const int rc = finish_call(ctxs[r], t_first, n_steps, s0[r]);
        if (rc && !first) first = rc;
    }
    return first;
}

static constexpr int kExchangeRetries = 8;

extern "C" {

int hakai_step(hakai_ctx* c, double t_first, int64_t n_steps, double d_time) {
    if (!c) return fail(HAKAI_ERR_ARG, "null");
    if (!c->model_ok || !c->state_ok) return fail(HAKAI_ERR_STATE, "step before upload_model/reset_state");
    if (n_steps < 0 || !(d_time > 0)) return fail(HAKAI_ERR_ARG, "step: n_steps=%lld d_time=%g", (long long)n_steps, d_time);
    if (n_steps > 1 && hkc::comm_is_local(c))
        return fail(HAKAI_ERR_ARG, "step: an in-process group is stepped one step per call, rank by rank");
    // a contact rank of an in-process group needs its peers' phases between its own: refused before
    // any work, so its contact state (tsel parity, touched lists, bin headers) stays in step with them
    if (hkc::comm_is_local(c) && hkc::contact_multi(c) && hkc::comm_size(c) > 1)
        return fail(HAKAI_ERR_STATE, "step: rank %d of an in-process group with multi-GPU contact is stepped by "
                    "hakai_step_group only", hkc::comm_rank(c));
    HIPCHK(hipSetDevice(c->device));
    // a step that overflowed a multi-GPU contact exchange runs again once its capacity has grown
    // (every rank takes the same decision from the same gathered counts)
    for (int attempt = 0;; ++attempt) {
        const int rc = step_call(c, t_first, n_steps, d_time);
        if (!rc || attempt >= kExchangeRetries || !hkc::contact_exchange_retry(c)) return rc;
        ++c->exchange_retries;
        n_steps -= (int64_t)(c->poison_step - (long long)t_first);
        t_first = (double)c->poison_step;
    }
}

int hakai_step_group(hakai_ctx** ctxs, int32_t n, double t_first, int64_t n_steps, double d_time) {
    if (!ctxs || n <= 0) return fail(HAKAI_ERR_ARG, "step_group: no contexts");
    if (n_steps < 0 || !(d_time > 0)) return fail(HAKAI_ERR_ARG, "step_group: n_steps=%lld d_time=%g",
                                                  (long long)n_steps, d_time);
    for (int r = 0; r < n; ++r) {
        hakai_ctx* c = ctxs[r];
        if (!c) return fail(HAKAI_ERR_ARG, "step_group: null context %d", r);
        if (!c->model_ok || !c->state_ok) return fail(HAKAI_ERR_STATE, "step_group: rank %d has no model/state", r);
        if (n > 1 && (!c->comm || hkc::comm_rank(c) != r || hkc::comm_size(c) != n ||
                      hkc::comm_peer_ctx(c, r) != c))
            return fail(HAKAI_ERR_ARG, "step_group: context %d is not rank %d of an in-process group of %d", r, r, n);
        hkc::graph_invalidate(c);
    }
    HIPCHK(hipSetDevice(ctxs[0]->device));
    for (int attempt = 0;; ++attempt) {
        const int rc = step_group_call(ctxs, n, t_first, n_steps, d_time);
        if (!rc || attempt >= kExchangeRetries) return rc;
        bool retry = true;  // (the same on every rank: they read the same headers)
        for (int r = 0; r < n; ++r) retry = hkc::contact_exchange_retry(ctxs[r]) && retry;
        if (!retry) return rc;
        const long long p = ctxs[0]->poison_step;
        for (int r = 1; r < n; ++r)  // every rank read the same headers: the same step, or no retry
            if (ctxs[r]->poison_step != p)
                return fail(rc, "step_group: ranks disagree on the poisoned step (rank 0: %lld, rank %d: %lld)", p, r,
                            ctxs[r]->poison_step);
        for (int r = 0; r < n; ++r) ++ctxs[r]->exchange_retries;
        n_steps -= (int64_t)(p - (long long)t_first);
        t_first = (double)p;
    }
}

int hakai_graph_steps(hakai_ctx* c, int64_t* n) {
    if (!c || !n) return fail(HAKAI_ERR_ARG, "null");
    *n = c->graph_steps;
    return 0;
}

}  // extern "C"
