// step_view_check.cpp -- CPU enumeration of hkc::StepView (csrc/hakai_step_view.hpp, the only header
// this program includes from the product): the host's view of the stepping state through stepping
// calls, graph replays and contact-overflow rollbacks. tests/test_step_view_cpu.py compares every
// line with a restatement of the two-flag bookkeeping the struct replaced.
//
// For every start state (cur 0/1 x fe_ok x triax_ok x Q source Fe/Buf/Own, steps_done 5), own 0/1
// and call length n = 1..4 (the n-th step is the call's last) it prints one JSON line for the state
// after the call ("run") and one per rollback point good = 0..n ("rollback"); for every start state
// a graph can replay from (Q source not Buf; owner assembly as the source says) and len = 2, 4 the
// state after a replay ("replay" = len non-last steps). q: 0 Fe, 1 Buf, 2 Own.
#include <cstdio>

#include "../hakai-fem_amd/csrc/hakai_step_view.hpp"

using hkc::QSrc;
using hkc::StepView;

static void fields(const StepView& v) {
    std::printf("{\"cur\": %d, \"steps_done\": %lld, \"fe_ok\": %d, \"triax_ok\": %d, \"q\": %d}", v.cur, v.steps_done,
                v.fe_ok ? 1 : 0, v.triax_ok ? 1 : 0, (int)v.q);
}

static void line(const char* kind, const StepView& s0, int own, int n, int steps, const StepView& out) {
    std::printf("{\"kind\": \"%s\", \"s0\": ", kind);
    fields(s0);
    std::printf(", \"own\": %d, \"n\": %d, \"steps\": %d, \"out\": ", own, n, steps);
    fields(out);
    std::printf("}\n");
}

int main() {
    const QSrc srcs[3] = {QSrc::Fe, QSrc::Buf, QSrc::Own};
    for (int bits = 0; bits < 8; ++bits)
        for (QSrc q : srcs) {
            StepView s0;
            s0.cur = bits & 1;
            s0.fe_ok = (bits & 2) != 0;
            s0.triax_ok = (bits & 4) != 0;
            s0.q = q;
            s0.steps_done = 5;
            for (int own = 0; own < 2; ++own)
                for (int n = 1; n <= 4; ++n) {
                    StepView v = s0;
                    for (int k = 0; k < n; ++k) v.advance(own != 0, k == n - 1);
                    line("run", s0, own, n, n, v);
                    for (int good = 0; good <= n; ++good) {
                        StepView r = v;
                        r.rollback(s0, good);
                        line("rollback", s0, own, n, good, r);
                    }
                }
            if (q == QSrc::Buf) continue;
            for (int len = 2; len <= 4; len += 2) {
                StepView v = s0;
                for (int k = 0; k < len; ++k) v.advance(q == QSrc::Own, false);
                line("replay", s0, q == QSrc::Own ? 1 : 0, len, len, v);
            }
        }
    return 0;
}
