"""The host's view of the stepping state (csrc/hakai_step_view.hpp hkc::StepView), enumerated on the CPU.

tools/step_view_check.cpp prints, for every start state, owner-assembly mode, call length and rollback
point, the fields StepView ends with. This test restates the bookkeeping that StepView replaced -- the
two flags q_from_buf / own_valid and the field-by-field writes of the step, of the graph-replay branch
and of the rollback after a contact overflow, as they stood in hakai_capi.cpp before the split -- and
compares every line with it. No GPU.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "step_view_check")

FE, BUF, OWN = 0, 1, 2


def _from_q(s):
    """A printed state as the earlier fields: one Q source -> the flag pair."""
    return dict(cur=s["cur"], steps_done=s["steps_done"], fe_ok=bool(s["fe_ok"]), triax_ok=bool(s["triax_ok"]),
                q_from_buf=s["q"] == BUF, own_valid=s["q"] == OWN)


def _to_q(c):
    assert not (c["q_from_buf"] and c["own_valid"]), c  # no path leaves both flags set
    return dict(cur=c["cur"], steps_done=c["steps_done"], fe_ok=int(c["fe_ok"]), triax_ok=int(c["triax_ok"]),
                q=BUF if c["q_from_buf"] else OWN if c["own_valid"] else FE)


def _step_once(c, own, last):
    """What one step did to the host's fields."""
    c["cur"] = 1 - c["cur"]
    c["q_from_buf"] = False
    c["own_valid"] = own
    c["fe_ok"] = (not own) or last
    c["triax_ok"] = last
    c["steps_done"] += 1


def _replay(c, length):
    """What the graph-replay branch did for `length` captured steps (cur untouched: length is even)."""
    c["q_from_buf"] = False
    c["fe_ok"] = not c["own_valid"]
    c["triax_ok"] = False
    c["steps_done"] += length


def _rollback(c, s0, good):
    """What the end of a poisoned call did with the snapshot s0 of the call's start."""
    c["cur"] = 1 - s0["cur"] if good & 1 else s0["cur"]
    c["steps_done"] = s0["steps_done"] + good
    if good == 0:
        for k in ("fe_ok", "triax_ok", "own_valid", "q_from_buf"):
            c[k] = s0[k]
    else:
        c["fe_ok"] = not c["own_valid"]
        c["triax_ok"] = False


@pytest.fixture(scope="module")
def lines():
    if not os.path.exists(EXE):
        pytest.skip("tools/_build/step_view_check not built (__graft_entry__.build())")
    out = subprocess.run([EXE], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    return [json.loads(ln) for ln in out.stdout.splitlines() if ln.strip()]


def test_every_case_is_enumerated(lines):
    kinds = {}
    for r in lines:
        kinds[r["kind"]] = kinds.get(r["kind"], 0) + 1
    starts = 2 * 2 * 2 * 3
    assert kinds == {"run": starts * 2 * 4, "rollback": starts * 2 * (2 + 3 + 4 + 5), "replay": 2 * 2 * 2 * 2 * 2}, kinds
    seen = {json.dumps([r["kind"], r["s0"], r["own"], r["n"], r["steps"]], sort_keys=True) for r in lines}
    assert len(seen) == len(lines)


def test_step_view_matches_the_flag_bookkeeping(lines):
    for r in lines:
        s0 = _from_q(r["s0"])
        c = dict(s0)
        own, n = bool(r["own"]), r["n"]
        if r["kind"] == "replay":
            assert n % 2 == 0 and own == s0["own_valid"] and not s0["q_from_buf"], r
            _replay(c, n)
        else:
            for k in range(n):
                _step_once(c, own, k == n - 1)
            if r["kind"] == "rollback":
                _rollback(c, s0, r["steps"])
        assert r["out"] == _to_q(c), r
        assert r["out"]["cur"] == r["s0"]["cur"] ^ (r["steps"] & 1), r


def test_replay_equals_non_last_steps(lines):
    """An even run of non-last steps, step by step, ends where the replay branch's shortcut did."""
    n = 0
    for r in lines:
        if r["kind"] != "replay":
            continue
        c = _from_q(r["s0"])
        for _ in range(r["n"]):
            _step_once(c, c["own_valid"], False)
        assert r["out"] == _to_q(c), r
        n += 1
    assert n == 32
