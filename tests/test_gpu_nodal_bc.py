"""The nodal update (k_nodal), the boundary conditions (k_bc, the BCs fused into k_nodal) and the
amplitudes (bc_value) on the device, on the crafted decks and operands of tests/nodal_cases.py
(tests/test_nodal_bc_cpu.py proves on the CPU that they hit every branch and that the oracle equals
the restatement of tests/nodal_ref.py on them). The element kernel runs in reference order
(elem_exact 1), so whole states equal the oracle's; every comparison is bit for bit."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import hakai
import nodal_cases as C
import nodal_ref as R
import oracle as O
from hakai import dist
from hakai._abi import check
from hakai.model import BCGroup, Model
from hakai.solver import Solver, State, step_group
from util import STATE, bitwise_equal, same_state

pytestmark = pytest.mark.gpu


def _snap(o):
    return SimpleNamespace(**{k: v.copy() for k, v in o.s.items()})


@pytest.fixture(scope="module")
def deck():
    """bc_deck and the oracle's state after every step (index 0: the initial state)."""
    m = C.bc_deck()
    o = O.Oracle(m)
    snaps = [_snap(o)]
    for t in range(1, C.N_STEPS + 1):
        o.run(t, 1)
        snaps.append(_snap(o))
    assert not o.deletions
    return m, snaps


def _solver(m, tune, **kw):
    sv = Solver(m, **kw)
    sv.set_tuning("elem_exact", 1)
    for k, v in tune.items():
        sv.set_tuning(k, v)
    return sv


def _chunks_to(stops):
    out, t = [], 1
    for s in stops:
        out.append((t, s - t + 1))
        t = s + 1
    return out


TRAJECTORIES = {
    "default": ({}, _chunks_to(C.CHECK_STEPS)),
    "k_bc": ({"fuse_bc": 0}, _chunks_to(C.CHECK_STEPS)),
    "stream": ({"graph": 0}, _chunks_to(C.CHECK_STEPS)),
    "k_bc_stream": ({"fuse_bc": 0, "graph": 0}, _chunks_to(C.CHECK_STEPS)),
    "split": ({}, [(1, 7), (8, 1), (9, 40), (49, 32)]),   # both start parities, graph chunks and remainders
    "fours": ({}, [(t, 4) for t in range(1, C.N_STEPS, 4)]),      # a short graph and a stream tail per call
    "single_steps": ({}, [(t, 1) for t in range(1, C.N_STEPS + 1)]),  # every step against the oracle
}
CHECKED_STOPS = ("default", "k_bc", "stream", "k_bc_stream")


@pytest.mark.parametrize("case", list(TRAJECTORIES))
def test_bc_deck_trajectory_bitexact(deck, case):
    """After every call the whole state equals the oracle's: the BCs fused into k_nodal or through
    k_bc, the time from the host or from the device slot inside replayed graphs."""
    m, snaps = deck
    tune, chunks = TRAJECTORIES[case]
    with _solver(m, tune) as sv:
        for t0, n in chunks:
            sv.step(t0, n)
            same_state(sv.download(), snaps[t0 + n - 1], triax=False)
        gs = sv.graph_steps()
    assert chunks[-1][0] + chunks[-1][1] - 1 == C.N_STEPS
    if case != "single_steps":
        assert (gs > 0) == (tune.get("graph", 1) != 0)
    if case in CHECKED_STOPS:
        assert [t0 + n - 1 for t0, n in chunks] == list(C.CHECK_STEPS)


def _upload(sv, s):
    sv.upload(State(s.disp.copy(), s.disp_pre.copy(), s.velo.copy(), s.Q.copy(), s.integ_stress.copy(),
                    s.integ_strain.copy(), s.integ_yield_stress.copy(), s.integ_eq_plastic_strain.copy(),
                    s.integ_triax_stress.copy(), s.element_flag.copy(), s.Qe.copy()))


@pytest.mark.parametrize("tune", [{}, {"fuse_bc": 0}], ids=["fused", "k_bc"])
def test_bc_deck_one_step_fused_element_kernel(deck, tune):
    """elem_exact 0: the nodal update and the BCs are the same kernels, so disp one step after the
    oracle's uploaded state equals the oracle's, at every checked step."""
    m, snaps = deck
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", 0)
        for k, v in tune.items():
            sv.set_tuning(k, v)
        for t in C.CHECK_STEPS:
            _upload(sv, snaps[t - 1])
            sv.step(t, 1)
            assert bitwise_equal(sv.download(disp=True).disp, snaps[t].disp), t


@pytest.mark.parametrize("fuse", [1, 0])
def test_bc_deck_wide_bitexact(fuse):
    """More than 256 resolved dofs: k_bc runs a full and a partial block."""
    m = C.bc_deck_wide()
    n = len(C.resolved(m))
    assert n > 256 and n % 256
    o = O.Oracle(m)
    o.run(1, 40)
    with _solver(m, {"fuse_bc": fuse}) as sv:
        sv.step(1, 40)
        same_state(sv.download(), _snap(o), triax=False)


def test_bc_deck_two_ranks_bitexact():
    """Two in-process ranks of the 12-layer deck: MID's roller plane lies on the interface and COLUMN
    crosses it, so k_bc overwrites what the interface fix has just redone."""
    glob = C.bc_deck(nz=12)
    o = O.Oracle(glob)
    o.run(1, C.N_STEPS)
    parts = [dist.slab_partition(glob, r, 2, 3, 2) for r in range(2)]
    svs = []
    for r, (loc, diag, iface) in enumerate(parts):
        sv = _solver(loc, {}, diag_M=diag)
        sv.set_element_offset(loc.global_element_offset)
        sv.comm_init_local(r, 2, 4242)
        sv.set_interface(*iface)
        svs.append(sv)
    try:
        step_group(svs, 1, C.N_STEPS)
        for sv, (loc, _, iface) in zip(svs, parts):
            st = sv.download()
            n0, nl = loc.global_node_offset, loc.nNode
            e0, el = loc.global_element_offset, loc.nElement
            sl, gp = slice(3 * n0, 3 * (n0 + nl)), slice(8 * e0, 8 * (e0 + el))
            on_iface = {3 * int(n) + c for n in iface[0] for c in range(3)}
            assert on_iface & {int(d) - 1 for g in loc.bc for dofs, _ in g.entries for d in dofs}
            for k in ("disp", "disp_pre"):
                assert bitwise_equal(getattr(st, k), o.s[k][sl]), k
            for k in ("integ_stress", "integ_strain", "integ_yield_stress", "integ_eq_plastic_strain"):
                assert bitwise_equal(getattr(st, k), o.s[k][gp]), k
            assert bitwise_equal(st.element_flag, o.s["element_flag"][e0:e0 + el])
            assert bitwise_equal(st.Qe, o.s["Qe"][e0:e0 + el])
    finally:
        for sv in svs:
            sv.close()


def _set_bc(sv, model):
    bc, keep = model.c_bc()
    check(sv.L.hakai_set_bc(sv.ctx, ctypes.byref(bc)))
    del keep


@pytest.mark.parametrize("blocks,m", C.probe_bars(), ids=[f"{b}_blocks" for b in C.PROBE_BLOCKS])
def test_one_step_probes(blocks, m):
    """k_nodal's uploaded-Q path alone, one step from crafted operands, without BCs (the plain
    instantiation), with them fused into k_nodal and with them through k_bc, at block counts on both sides of xcd_remap_rev's
    switch at 16 and with nwg & 7 = 0, 1, 7. Every dof of the random set has its own expected
    value: a block the permutation leaves out keeps u_pre and fails."""
    nN = m.nNode
    assert (nN + 255) // 256 == blocks and nN % 256
    states = C.probe_states(nN, seed=blocks)
    diag = states[0][1]
    mb = Model(m.coordmat, m.elementmat, m.element_material, m.materials, bc=C.probe_bc(m), d_time=m.d_time,
               end_time=m.end_time)
    none = State(None, None, None, None, None, None, None, None, None, None, None)
    with _solver(m, {}, diag_M=diag) as sv:
        for model, fuse in ((m, 1), (mb, 1), (mb, 0)):
            _set_bc(sv, model)
            sv.set_tuning("fuse_bc", fuse)
            for name, mass, u, up, q in states:
                assert mass is diag
                st = State(**{**none.__dict__, "disp": u.copy(), "disp_pre": up.copy(), "Q": q.copy()})
                sv.upload(st)
                sv.step(1, 1)
                got = sv.download(disp=True).disp
                want = R.nodal_step(diag, m.dt, u, up, q, np.zeros(3 * nN))
                R.apply_bc(model, 1.0 * m.dt, want)
                bad = np.flatnonzero(got.view(np.uint64) != want.view(np.uint64))
                assert bad.size == 0, (name, len(model.bc), "blocks of the first mismatches", bad[:8] // 768)
                o = O.Oracle(model)
                o.diag_M[:] = diag
                o.s["disp"][:], o.s["disp_pre"][:], o.s["Q"][:] = u, up, q
                o.run(1, 1)
                assert bitwise_equal(got, o.s["disp"]), (name, len(model.bc))


def test_history_records_same_bits_across_bc_paths(deck):
    """History on the top plane (prescribed dofs, so W_bc is live): the records do not depend on how
    the BCs reach memory or on where the time comes from."""
    m, snaps = deck
    top = C.top_nodes(m)
    recs = {}
    for name, tune in (("base", {"fuse_bc": 1, "graph": 16}), ("k_bc", {"fuse_bc": 0, "graph": 16}),
                       ("stream", {"fuse_bc": 1, "graph": 0})):
        with _solver(m, tune) as sv:
            sv.history_enable([top])
            sv.step(1, C.N_STEPS)
            recs[name] = sv.history()
            same_state(sv.download(), snaps[C.N_STEPS], triax=False)
    base = recs["base"]
    assert len(base["steps"]) == C.N_STEPS and np.any(base["W_bc"][:, 1] != 0.0)
    for name in ("k_bc", "stream"):
        assert np.array_equal(base["steps"], recs[name]["steps"]), name
        assert bitwise_equal(base["values"], recs[name]["values"]), name
        assert bitwise_equal(base["ke_seed"], recs[name]["ke_seed"]), name


def test_one_point_amplitude_rejected(deck):
    """hakai_set_bc refuses a one-point amplitude (the reference raises BoundsError at :598). The
    call queues nothing: the state is untouched and the context goes on as one without BCs does."""
    m, _ = deck
    free = Model(m.coordmat, m.elementmat, m.element_material, m.materials, bc=[], ic_dofs=m.ic_dofs,
                 ic_values=m.ic_values, d_time=m.d_time, end_time=m.end_time)
    bad = Model(m.coordmat, m.elementmat, m.element_material, m.materials,
                bc=list(m.bc[:3]) + [BCGroup([(np.array([120], np.int64), 1.0)], np.array([C.T(3)]), np.array([1.0]))],
                d_time=m.d_time, end_time=m.end_time)
    with pytest.raises(hakai.HakaiError):
        Solver(bad)
    with _solver(free, {}) as a, _solver(free, {}) as b:
        for sv in (a, b):
            sv.step(1, 4)
        before = a.download()
        with pytest.raises(hakai.HakaiError):
            _set_bc(a, bad)
        same_state(a.download(), before)
        for sv in (a, b):
            sv.step(5, 6)
        same_state(a.download(), b.download())
        assert all(np.isfinite(getattr(a.download(), k)).all() for k in STATE)
