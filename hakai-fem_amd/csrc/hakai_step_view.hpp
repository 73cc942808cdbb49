// hakai_step_view.hpp -- the host's view of the stepping state (no HIP: tools/step_view_check.cpp
// compiles this header alone). These member functions are the only code that changes the fields; the
// step driver (hakai_step.cpp), the state upload and reset (hakai_capi.cpp) and owner-computed
// assembly (hakai_own.cpp) call them and otherwise only read.
#pragma once

namespace hkc {

// Where the next nodal update's Q comes from: the gather over the element forces fe, the uploaded-Q
// buffer (an uploaded state, or owner sums handed over by own_materialize), or the last element
// step's owner-computed node sums.
enum class QSrc { Fe, Buf, Own };

struct StepView {
    int cur = 0;  // d_u[cur] = disp, d_u[1-cur] = disp_pre
    long long steps_done = 0;
    // fe / triax hold the current state's element forces / triaxiality. With owner-computed assembly
    // the element kernel stores fe (and, in both modes, triax) only on a call's last step, so after
    // a call whose later steps a contact overflow turned into no-ops they are stale: the Qe and
    // triaxiality downloads then fail (HAKAI_ERR_STATE) until a step has run (Q stays available).
    bool fe_ok = true, triax_ok = true;
    QSrc q = QSrc::Fe;

    // One step's launches are enqueued; `own`: its element kernel summed the node forces itself,
    // `last`: it was a call's last step (the one that stores fe and triax).
    void advance(bool own, bool last) {
        cur = 1 - cur;  // disp <- disp_new, disp_pre <- disp (:626-627)
        q = own ? QSrc::Own : QSrc::Fe;
        fe_ok = !own || last;  // owner assembly stores fe on a call's last step only
        triax_ok = last;
        steps_done++;
    }
    // A contact overflow poisoned a call that started at s0 after `good` of its steps: the device
    // holds the state after those. With good > 0 the Q source is the one the call's steps left (every
    // step of a call takes the same).
    void rollback(const StepView& s0, long long good) {
        cur = (good & 1) ? 1 - s0.cur : s0.cur;
        steps_done = s0.steps_done + good;
        if (good == 0) {  // nothing of the call ran: where the Q of the next nodal update is
            fe_ok = s0.fe_ok;
            triax_ok = s0.triax_ok;
            q = s0.q;
        } else {  // the call's last step (the one that stores fe and triax) did not run
            fe_ok = q != QSrc::Own;
            triax_ok = false;
        }
    }
    // A reset (cur = 0, Q from the zeroed fe) or an uploaded state (buffers and an uploaded Q kept):
    // the next nodal update gathers fe unless the uploaded-Q buffer is live.
    void restart(bool keep_cur) {
        if (!keep_cur) {
            cur = 0;
            q = QSrc::Fe;
        }
        own_dropped();
        fe_ok = triax_ok = true;
        steps_done = 0;
    }
    void q_uploaded() { q = QSrc::Buf; }                           // Q now lies in the uploaded-Q buffer
    void own_dropped() { if (q == QSrc::Own) q = QSrc::Fe; }       // the owner sums are gone or void
};

}  // namespace hkc
