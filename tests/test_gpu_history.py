"""History output on the GPU (hakai_history_*, csrc/hakai_history.hip) against its NumPy
restatement (history_ref).

The comparison is the same throughout. Solver A has history on and runs the whole span in ONE step
call, so captured graphs are replayed. Solver B has no history and is stepped one step at a time;
its disp, disp_pre and Q before each step (for contact also contact_force(t)) and its disp after
it feed history_ref, whose values are exactly rounded sums. With u = 2^-53 and sum|term| from
history_ref:
  * fields 0-9 and 13-15: |x - fsum| <= 48 u sum|term| (8 tree levels in a 256-node chunk, at most
    32 over chunks, 8 for the few roundings inside a term);
  * the works: that bound summed over the steps so far, plus T u max|W| for the running sum.
A's final state equals B's bit for bit: history perturbs nothing.
"""
import os

import numpy as np
import pytest

import hakai
from hakai import _abi, mesh
from hakai.solver import Solver, read_history_csv
from history_ref import HistoryRef, U, balance, prescribed_mask
from util import bitwise_equal, fast_deletion_bar, same_state, small_bar

pytestmark = pytest.mark.gpu

PLAIN = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15]
WORKS = [10, 11, 12]


def tuned(m, tune):
    sv = Solver(m)
    for k, v in (tune or {}).items():
        sv.set_tuning(k, v)
    return sv


def run_b(m, n_steps, sets, tune=None, t0=1):
    """Solver B: no history, one step at a time; history_ref on its arrays. Returns the reference
    records (n, S, 16), their magnitudes, (ke_seed, its magnitude), the final state, the deletions."""
    contact = getattr(m, "contact_flag", 0) >= 1
    recs, mags = [], []
    with tuned(m, tune) as sv:
        ref = HistoryRef(sv.diag_M, prescribed_mask(m), sets, m.dt)
        st = sv.download(disp=True, disp_pre=True, Q=True)
        seed = ref.seed(st.disp, st.disp_pre)
        for t in range(t0, t0 + n_steps):
            f = sv.contact_force(t) if contact else None
            sv.step(t, 1)
            nx = sv.download(disp=True, disp_pre=True, Q=True)
            v, g = ref.step(nx.disp, st.disp, st.Q, f)
            recs.append(v)
            mags.append(g)
            st = nx
        final = sv.download()
        dels = sv.deleted()
    return np.array(recs), np.array(mags), seed, final, dels


def run_a(m, n_steps, sets, tune=None, stride=1, capacity=1 << 12):
    """Solver A: history on, the whole span in one step call."""
    with tuned(m, tune) as sv:
        sv.history_enable(sets, stride=stride, capacity=capacity)
        sv.step(1, n_steps)
        h = sv.history()
        h["count"] = sv.history_count()
        final = sv.download()
        dels = sv.deleted()
        gs = sv.graph_steps()
    return h, final, dels, gs


def check_records(h, recs, mags, seed=None, k0=0):
    """A's records against the restatement of B's arrays, within the module docstring's bounds."""
    cum = np.cumsum(48 * U * mags[:, :, WORKS], axis=0)
    wmax = np.maximum.accumulate(np.abs(recs[:, :, WORKS]), axis=0)
    assert len(h["steps"]) > 0
    for i, k in enumerate(h["steps"] - k0):
        x, r, g = h["values"][i], recs[k], mags[k]
        err, bound = np.abs(x[:, PLAIN] - r[:, PLAIN]), 48 * U * g[:, PLAIN]
        assert np.all(err <= bound), (k, "plain fields", float(np.max(err / np.maximum(bound, 1e-300))))
        err, bound = np.abs(x[:, WORKS] - r[:, WORKS]), cum[k] + (k + 1) * U * wmax[k]
        assert np.all(err <= bound), (k, "works", float(np.max(err / np.maximum(bound, 1e-300))))
    if seed is not None:
        assert np.all(np.abs(h["ke_seed"] - seed[0]) <= 48 * U * seed[1])


def same_records(a, b):
    assert np.array_equal(a["steps"], b["steps"])
    assert bitwise_equal(a["values"], b["values"])
    assert bitwise_equal(a["ke_seed"], b["ke_seed"])


# ---- 1. small_bar -----------------------------------------------------------------------------------
@pytest.mark.parametrize("exact", [0, 1])
def test_small_bar_records_match_restatement(exact):
    m = small_bar()
    nN = m.nNode
    sets = [np.arange(1, nN + 1), mesh.plane_nodes(3, 2, 0), mesh.plane_nodes(3, 2, 6), np.array([17]),
            np.array([nN]), np.zeros(0, np.int64)]
    tune = {"elem_exact": exact}
    h, fa, _, gs = run_a(m, 60, sets, tune)
    recs, mags, seed, fb, _ = run_b(m, 60, sets, tune)
    assert np.array_equal(h["steps"], np.arange(60)) and h["count"] == (60, 60)
    check_records(h, recs, mags, seed)
    same_state(fa, fb)
    assert gs > 0
    assert np.all(h["values"][:, 6, :] == 0.0)                      # the empty set
    assert bitwise_equal(h["values"][:, 0, :], h["values"][:, 1, :])  # set 0 = the set of all nodes
    assert np.any(h["F_int"][:, 2, 2] != 0.0)                       # the clamped plane's reaction
    assert np.all(h["W_ext"] == 0.0) and np.all(h["F_ext"] == 0.0)  # no contact
    assert np.any(h["KE"][:, 4] > 0.0)


# ---- 2. reduction edges -----------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 2, 6), (2, 4, 16), (3, 3, 15), (1, 2, 42), (3, 3, 128),
                                   (3, 3, 257)])
def test_reduction_edges_both_forms(shape):
    """8, 84, 255, 256 and 258 nodes (257 is prime: no box mesh has it), then 2064 nodes (two
    groups of chunks) and 4128 (three: a tree with a childless right branch). Both launch forms give
    the same bits."""
    m = small_bar(*shape)
    nN = m.nNode
    assert nN == (shape[0] + 1) * (shape[1] + 1) * (shape[2] + 1)
    one_wave = np.arange(1, min(nN, 5) + 1) if nN < 72 else np.arange(66, 72)  # lanes of one wave only
    # a single node in every 256-node chunk, on a different lane in each
    per_chunk = np.array([min(c * 256 + (37 * c) % 256 + 1, nN) for c in range((nN + 255) // 256)])
    sets = [one_wave, per_chunk]
    recs, mags, seed, fb, _ = run_b(m, 3, sets)
    got = []
    for form in (0, 1):
        h, fa, _, _ = run_a(m, 3, sets, {"history_one_block": form})
        check_records(h, recs, mags, seed)
        same_state(fa, fb)
        got.append(h)
    same_records(got[0], got[1])
    assert np.any(got[0]["F_int"][:, 0, :] != 0.0)


# ---- 3. contact -------------------------------------------------------------------------------------
def test_contact_external_force_and_work():
    m = mesh.two_body_model()
    n1 = 9 * 9 * 3
    sets = [np.arange(1, n1 + 1), np.arange(n1 + 1, m.nNode + 1), mesh.plane_nodes(8, 8, 0)]
    h, fa, _, gs = run_a(m, 40, sets)
    recs, mags, seed, fb, _ = run_b(m, 40, sets)
    check_records(h, recs, mags, seed)
    same_state(fa, fb)
    assert gs > 0
    late = h["steps"] >= 20  # the 0.1 mm gap closes near step 10
    assert np.all(h["F_ext"][:5] == 0.0) and np.all(h["W_ext"][:5] == 0.0)
    for s in (1, 2):  # each body feels the other (their sum, set 0, cancels to rounding)
        assert np.any(h["F_ext"][late][:, s, :] != 0.0)
    assert np.all(h["W_ext"][late][:, 0] != 0.0) and np.all(h["W_ext"][late][:, 2] != 0.0)
    tot, parts = h["F_ext"][:, 0, :], h["F_ext"][:, 1, :] + h["F_ext"][:, 2, :]
    bound = 48 * U * (mags[:, 0, 3:6] + mags[:, 1, 3:6] + mags[:, 2, 3:6]) + \
        U * (np.abs(h["F_ext"][:, 1, :]) + np.abs(h["F_ext"][:, 2, :]))
    assert np.all(np.abs(tot - parts) <= bound)


# ---- 4. deletion and amplitude BC ---------------------------------------------------------------------
def test_deletion_bar_balance():
    m = fast_deletion_bar()
    h, fa, da, gs = run_a(m, 3000, [], stride=50, capacity=64)
    recs, mags, seed, fb, db = run_b(m, 3000, [])
    assert np.array_equal(h["steps"], np.arange(0, 3000, 50)) and h["count"] == (60, 60)
    check_records(h, recs, mags, seed)
    same_state(fa, fb)
    assert len(db) == 4 and np.array_equal(da, db) and gs > 2500
    res = [balance(v[0], h["ke_seed"][0]) for v in h["values"]]
    worst = max(abs(r) for r, _ in res) / max(big for _, big in res)
    print(f"deletion bar: worst balance residual of the device records {worst:.3e} of the largest energy term")
    assert worst <= 64 * 1.3e-14  # 64 x the oracle's residual for this model (tests/test_history_cpu.py)
    assert h["W_bc"][-1, 0] != 0.0 and h["W_int"][-1, 0] > 0.0


# ---- 5. invariance -----------------------------------------------------------------------------------
def test_records_invariant_under_tuning():
    m = fast_deletion_bar(4, 4, 40)  # 20 batches of elements, 1025 nodes: five chunks
    base = {"elem_pipe_min": 0, "elem_pipe_blocks": 3, "own_assembly": 1, "graph": 16, "nodal_padded": 1,
            "fuse_bc": 1}
    sets = [mesh.plane_nodes(4, 4, 0), mesh.plane_nodes(4, 4, 40)]

    def run(**chg):
        with tuned(m, {**base, **chg}) as sv:
            sv.history_enable(sets, stride=3, capacity=64)
            sv.step(1, 100)
            return sv.history(), sv.graph_steps(), sv.stat("own_steps")

    h0, gs0, own0 = run()
    assert gs0 > 0 and own0 > 0 and len(h0["steps"]) == 34
    for chg in ({"own_assembly": 0}, {"graph": 0}, {"nodal_padded": 0}, {"fuse_bc": 0}, {"elem_pipe_blocks": 0}, {},
                {"history_one_block": 0}, {"history_one_block": 1}):
        h, gs, own = run(**chg)
        same_records(h, h0)
        if chg.get("graph") == 0:
            assert gs == 0
        if chg.get("own_assembly") == 0 or chg.get("elem_pipe_blocks") == 0:
            assert own == 0


# ---- 6. ring and stride --------------------------------------------------------------------------------
def test_ring_stride_restart_and_reenable():
    m = small_bar()
    sets = [mesh.plane_nodes(3, 2, 6)]
    with Solver(m) as sv:
        sv.history_enable(sets, stride=7, capacity=4)
        assert sv.history_count() == (0, 0)
        sv.step(1, 60)
        assert sv.history_count() == (9, 4)  # states 0, 7, .. 56
        h = sv.history()
        assert list(h["steps"]) == [35, 42, 49, 56]
        one = sv.history(first=6, n=2)
        assert list(one["steps"]) == [42, 49] and bitwise_equal(one["values"], h["values"][1:3])
        for first, n in ((4, 1), (0, 9), (8, 2), (-1, 1)):  # overwritten, or not yet written
            with pytest.raises(hakai.HakaiError) as ei:
                sv.history(first=first, n=n)
            assert ei.value.code == _abi.HAKAI_ERR_ARG
        # an uploaded state restarts the count and seeds again
        st = sv.download()
        sv.upload(st)
        assert sv.history_count() == (0, 0)
        sv.step(61, 10)  # states 60 .. 69: one multiple of 7
        h = sv.history()
        assert list(h["steps"]) == [63] and sv.history_count() == (1, 1)
        ref = HistoryRef(sv.diag_M, prescribed_mask(m), sets, m.dt)
        ke, mag = ref.seed(st.disp, st.disp_pre)
        assert np.all(np.abs(h["ke_seed"] - ke) <= 48 * U * mag) and np.all(ke > 0)
        # a reset does the same, from the initial velocity
        sv.reset()
        assert sv.history_count() == (0, 0)
        st0 = sv.download(disp=True, disp_pre=True)
        sv.step(1, 8)
        h = sv.history()
        assert list(h["steps"]) == [0, 7]
        ke, mag = ref.seed(st0.disp, st0.disp_pre)
        assert np.all(np.abs(h["ke_seed"] - ke) <= 48 * U * mag) and np.all(ke > 0)
        first_run = h
        # disable, enable again
        sv.history_disable()
        with pytest.raises(hakai.HakaiError) as ei:
            sv.history_count()
        assert ei.value.code == _abi.HAKAI_ERR_STATE
        sv.step(9, 4)  # without history
        sv.reset()
        sv.history_enable(sets, stride=7, capacity=4)
        sv.step(1, 8)
        same_records(sv.history(), first_run)


# ---- 7. refusals -------------------------------------------------------------------------------------
def test_refusals():
    m = small_bar()
    nN = m.nNode
    with Solver(m) as sv:
        sv.comm_init_local(0, 1, 424201)
        with pytest.raises(hakai.HakaiError) as ei:
            sv.history_enable([])
        assert ei.value.code == _abi.HAKAI_ERR_STATE
    with Solver(m) as sv:
        sv.history_enable([np.array([1, 2])], stride=2, capacity=8)
        with pytest.raises(hakai.HakaiError) as ei:
            sv.comm_init_local(0, 1, 424202)
        assert ei.value.code == _abi.HAKAI_ERR_STATE
        bad = [dict(sets=[np.array([0])]), dict(sets=[np.array([nN + 1])]), dict(sets=[np.array([3, 3])]),
               dict(sets=[np.array([1])] * 16), dict(sets=[], stride=0), dict(sets=[], capacity=0)]
        for kw in bad:
            with pytest.raises(hakai.HakaiError) as ei:
                sv.history_enable(**kw)
            assert ei.value.code == _abi.HAKAI_ERR_ARG, kw
        sv.step(1, 6)  # the refused calls changed nothing: two sets, stride 2
        h = sv.history()
        assert list(h["steps"]) == [0, 2, 4] and h["values"].shape == (3, 2, 16)
        sv.history_enable([np.array([1])] * 15)  # 15 sets are allowed


# ---- 8. poisoned step -----------------------------------------------------------------------------------
def test_poisoned_step_leaves_no_record():
    """The contact_event_cap recipe of test_gpu_contact.test_event_cap_overflow_is_reported: an error
    return, the state stays the last applied step's. The records stop there too, and after raising
    the cap and stepping on they equal an undisturbed run's bit for bit."""
    import re
    m = mesh.two_body_model(plate=(12, 12, 1), impactor=(8, 8, 1), v=-1e5, perturb=0.03, seed=4, n_steps=60)
    n1 = 13 * 13 * 2
    sets = [np.arange(1, n1 + 1), np.arange(n1 + 1, m.nNode + 1)]

    def solver(cap):
        sv = tuned(m, {"elem_pipe_min": 0, "elem_pipe_blocks": 3, "contact_event_cap": cap})
        sv.history_enable(sets, stride=1, capacity=128)
        return sv

    with solver(1 << 12) as sv:
        sv.step(1, m.n_steps)
        full = sv.history()
        final = sv.download()
    assert list(full["steps"]) == list(range(m.n_steps)) and np.any(full["W_ext"][-1] != 0.0)
    with solver(1) as sv:
        with pytest.raises(hakai.HakaiError) as ei:
            sv.step(1, m.n_steps)
        p = int(re.search(r"step (\d+) was not applied", str(ei.value)).group(1))
        assert 1 < p < m.n_steps
        part = sv.history()
        assert list(part["steps"]) == list(range(p - 1))  # steps 1 .. p-1 ran: states 0 .. p-2
        assert bitwise_equal(part["values"], full["values"][:p - 1])
        sv.set_tuning("contact_event_cap", 1 << 12)
        sv.step(p, m.n_steps - p + 1)
        same_records(sv.history(), full)
        same_state(sv.download(), final)


# ---- 9. driver ----------------------------------------------------------------------------------------
def test_driver_writes_history_csv(tmp_path, monkeypatch):
    from inp_writer import write_inp
    m0 = mesh.two_body_model(plate=(5, 5, 2), impactor=(3, 3, 2), v=-1e5, n_steps=300)
    deck = write_inp(str(tmp_path / "impact.inp"), m0)
    monkeypatch.delenv("HAKAI_HISTORY", raising=False)
    hakai.hakai(deck, str(tmp_path / "plain"), verbose=False)
    assert not os.path.exists(tmp_path / "plain" / "history.csv")
    monkeypatch.setenv("HAKAI_HISTORY", "5")
    hakai.hakai(deck, str(tmp_path / "hist"), verbose=False)
    monkeypatch.delenv("HAKAI_HISTORY")
    files = sorted(os.listdir(tmp_path / "plain"))
    assert len(files) == 101 and sorted(os.listdir(tmp_path / "hist")) == files + ["history.csv"]
    for f in files:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "hist" / f, "rb").read(), f
    csv = read_history_csv(str(tmp_path / "hist" / "history.csv"))
    assert csv["sets"] == ["all", "inst1", "inst2", "bc1"]
    m = hakai.read_inp(deck)
    inst = [np.unique(m.elementmat[m.element_instance == i]) for i in (1, 2)]
    assert inst[0][0] == 1 and inst[1][-1] == m.nNode and len(inst[0]) + len(inst[1]) == m.nNode
    bc_nodes = np.unique((np.concatenate([d for d, _ in m.bc[0].entries]) - 1) // 3 + 1)
    with tuned(m, {"elem_exact": 1}) as sv:  # the driver's element arithmetic
        sv.history_enable(inst + [bc_nodes], stride=5, capacity=100)
        sv.step(1, m.n_steps)
        h = sv.history()
    assert np.array_equal(csv["steps"], h["steps"]) and len(h["steps"]) == 60
    assert bitwise_equal(csv["values"], h["values"])
    assert np.array_equal(csv["time"], h["steps"] * m.dt)
    assert np.any(h["F_ext"] != 0.0) and h["W_ext"][-1, 0] != 0.0  # the bodies met during the run
