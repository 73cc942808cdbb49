"""Contact-force probes of the device (hakai_contact.hip) at the crafted states of
tests/contact_cases.py, each against the oracle and, where it is fast enough, the exact-rational
restatement (tests/contact_ref.py), which tests/test_contact_edges_cpu.py holds against each other
on the CPU. Every case is one contact step (Solver.contact_force) on an uploaded state of at most
4608 hex: the full 3 nN force vector must equal the reference's and the event count its count.

What fails here if the code is wrong:
  * constants: the damping term (BVel::mq, PairParam::Cr), the self / other selection of kc and Cr
    and the uploaded velocity -- test_constants, test_self_pair;
  * the event-buffer spill of tri_cell (more than kEvLocal = 4 events in one search thread), fused
    and unfused small-deck paths, and the event capacity -- test_spill_path, test_event_cap;
  * the large-deck search (k_ct_tri, search items, reach_mask), also far from the origin --
    test_large_deck_search;
  * the decision boundaries x1 == 0, x2 == 0, x1 + x2 == 1, d == d_lim, d == 0, the range box, the
    ceil cell boundary and dpc == Rmax -- test_decision_boundaries;
  * zero-area triangles -- test_zero_area_triangle;
  * the velocity formed from disp - disp_pre after real steps -- test_velocity_from_displacements.
"""
import functools
import re

import numpy as np
import pytest

from hakai._abi import HakaiError
from hakai.solver import Solver, State
import oracle as O
import contact_cases as cc
from contact_ref import ContactRef

pytestmark = pytest.mark.gpu

CONTROL = (0.25, 1.0, 1.0, 0.0, 0.0)


def _upload(o, sv):
    s = o.s
    sv.upload(State(s["disp"].copy(), s["disp_pre"].copy(), s["velo"].copy(), s["Q"].copy(), s["integ_stress"].copy(),
                    s["integ_strain"].copy(), s["integ_yield_stress"].copy(), s["integ_eq_plastic_strain"].copy(),
                    s["integ_triax_stress"].copy(), s["element_flag"].copy(), s["Qe"].copy()))


@functools.lru_cache(maxsize=None)
def _restatement(key):
    """ContactRef of a small deck (its O(F^2) surface scan runs once per deck)."""
    name, params = key
    return ContactRef(cc.mixed_two_body(**dict(cc.SMALL_DECKS[name], **({"params": params} if params else {}))))


def _reference(m, position=None, velo=None, ref=None, indexed=False, mass=None):
    """(oracle with the crafted state, its force, its event count); with ref, the restatement must
    agree with the oracle first."""
    o = O.Oracle(m, contact_indexed=indexed)
    if mass is not None:
        o.diag_M[:] = mass
    cc.set_state(o, position, cc.noisy_velocity(m) if velo is None else velo)
    f, n = o.contact_force()
    if ref is not None:
        fr, nr = ref.force(o.s["position"].reshape(-1, 3), o.s["velo"], o.diag_M, o.s["element_flag"])
        assert nr == n and np.array_equal(fr, f, equal_nan=True)
    return o, f, n


def _probe(sv, o, f, n, what=""):
    _upload(o, sv)
    g = sv.contact_force(1)
    ev = sv.contact_stats()["events"]
    bad = np.flatnonzero(~((g == f) | (np.isnan(g) & np.isnan(f))))
    print(f"{what}: events {ev} (reference {n}), differing dofs {bad.size}"
          + (f", max |diff| {np.max(np.abs(g[bad] - f[bad])):.3e} of {np.max(np.abs(f)):.3e}" if bad.size else ""))
    assert np.array_equal(g, f, equal_nan=True), f"{what}: {bad.size} dofs differ, first {bad[:5]}"
    assert ev == n, what
    return g


# ---- 1. constants --------------------------------------------------------------------------------
@pytest.mark.parametrize("params,flag", [(cc.PARAMS, 1), (CONTROL, 1), ((0.5, 2.0, 0.5, 0.0625, 0.375), 2),
                                         (cc.PARAMS, 2)])
def test_constants(params, flag):
    """Damping, stiffness factors and friction live, with a velocity that differs on every dof."""
    name = "h4" if flag == 1 else "h4_flag2"
    m = cc.mixed_two_body(**dict(cc.SMALL_DECKS[name], params=params))
    o, f, n = _reference(m, ref=_restatement((name, params)))
    assert n == 85
    with Solver(m) as sv:
        g = _probe(sv, o, f, n, f"constants {params} flag {flag}")
    if params != CONTROL:   # the constants reach the force at all
        mc = cc.mixed_two_body(**dict(cc.SMALL_DECKS[name], params=CONTROL))
        assert not np.array_equal(g, _reference(mc)[1])


def test_constants_set_after_a_probe():
    """hakai_set_contact_params between probes reaches the pair table the search reads (d_par)."""
    ma, mb = cc.mixed_two_body(params=CONTROL), cc.mixed_two_body(params=cc.PARAMS)
    oa, fa, na = _reference(ma)
    ob, fb, nb = _reference(mb)
    with Solver(ma) as sv:
        _probe(sv, oa, fa, na, "control")
        sv.L.hakai_set_contact_params(sv.ctx, *[float(x) for x in cc.PARAMS])
        _probe(sv, ob, fb, nb, "after set_contact_params")


# ---- 2. spill path -------------------------------------------------------------------------------
@pytest.mark.parametrize("fuse", [0, 1])
@pytest.mark.parametrize("name", ["h4", "h8", "small"])
def test_spill_path(name, fuse):
    """h4: 6 events in one (triangle, cell), h8: 28 (36 on one triangle); `small` (4) stays within
    the registers, the control."""
    m = cc.mixed_two_body(**cc.SMALL_DECKS[name])
    o, f, n = _reference(m, ref=_restatement((name, None)))
    assert n == {"h4": 85, "h8": 293, "small": 26}[name]
    with Solver(m) as sv:
        sv.set_tuning("contact_fuse_small", fuse)
        _probe(sv, o, f, n, f"{name} fuse_small {fuse}")
        assert sv.contact_stats()["hash_buckets"] <= 32768   # the small-deck path


def test_event_cap():
    """The h8 deck at the smallest event buffer that holds it, below it, and raised again. The
    buffer is 64 shards of cap / 64 slots and a wave's events all go to one shard, so the smallest
    sufficient buffer is 64 times the fullest shard, which the overflow report states (the counters
    run on past the capacity). A 1-slot probe must fail loudly and return no force; a probe at
    exactly the reported size holds every event and gives the reference's bits. (Which candidates
    share a wave follows the order of the prefilter's atomics, so a probe may meet a fuller shard
    than the last one reported: it then fails loudly again and reports that one.)"""
    m = cc.mixed_two_body(**cc.SMALL_DECKS["h8"])
    o, f, n = _reference(m, ref=_restatement(("h8", None)))
    with Solver(m) as sv:
        _probe(sv, o, f, n, "h8 default buffer")
        assert sv.contact_stats()["max_events"] == n
        cap, held = 1, False
        for attempt in range(4):
            sv.set_tuning("contact_event_cap", cap)
            _upload(o, sv)
            try:
                g = sv.contact_force(1)
            except HakaiError as e:
                mo = re.search(r"(\d+) events in one step \((\d+) in one of 64 shards\)", str(e))
                assert mo and int(mo.group(1)) == n, str(e)
                fullest = int(mo.group(2))
                assert 28 <= fullest <= n and 64 * fullest > cap   # one search thread alone has 28
                cap = 64 * fullest
                continue
            assert attempt > 0, "a one-slot buffer must overflow"
            print(f"h8 at {cap} slots ({cap // 64} per shard)")
            assert np.array_equal(g, f) and sv.contact_stats()["events"] == n
            held = True
            break
        assert held
        sv.set_tuning("contact_event_cap", 1 << 14)
        _probe(sv, o, f, n, "h8 buffer raised again")


# ---- 3. self pair --------------------------------------------------------------------------------
def test_self_pair():
    """One instance: a single (1,1) pair with ddiv = 0.6 max_size, the own-element skip, kc_s and
    Cr_s, 60 events, 5 in one search thread."""
    m = cc.mixed_two_body(**cc.SMALL_DECKS["self"])
    o, f, n = _reference(m, ref=_restatement(("self", None)))
    assert n == 60 and [(p["i_instance"], p["j_instance"]) for p in o.contact_pairs()] == [(1, 1)]
    with Solver(m) as sv:
        g = _probe(sv, o, f, n, "self pair")
    # kc_o / Cr_o in the self constants' place would give these bits instead
    swapped = cc.mixed_two_body(one_instance=True, params=(0.25, 0.75, 1.5, 0.25, 0.125))
    assert not np.array_equal(g, _reference(swapped)[1])


# ---- 4. large-deck search ------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _large_unshifted():
    m = cc.mixed_two_body(**cc.LARGE)
    o, f, n = _reference(m, indexed=True)
    assert n == 295
    return o.diag_M.copy(), f


@pytest.mark.parametrize("shift", [(0, 0, 0)] + cc.SHIFTS, ids=["origin", "2^20", "2^30"])
@pytest.mark.parametrize("binfilter", [0, 1])
def test_large_deck_search(binfilter, shift):
    """64x64x1 plate: more than 32768 buckets, so k_ct_tri, the search items and reach_mask run.
    Shifted by (2^20, -2^20, 2^10) and (-2^30, 2^30, 2^30) -- the exponents asked for: the fine
    mesh's coordinates (multiples of 2^-7 below 64) stay exact -- the force must be the unshifted
    deck's bit for bit: positions differ by an exact shift, so every contact expression sees the
    same differences. The lumped mass does move with the shift (integrated from the absolute
    coordinates, 1e-9 .. 1e-6 relative), so both sides of the shifted cases are given the unshifted
    deck's mass; tests/test_contact_edges_cpu.py checks that the oracle then keeps its bits."""
    mass0, f0 = _large_unshifted()
    m = cc.mixed_two_body(**cc.LARGE, shift=shift)
    o, f, n = _reference(m, indexed=True, mass=mass0)
    assert n == 295 and np.array_equal(f, f0)
    with Solver(m, diag_M=mass0) as sv:
        sv.set_tuning("contact_fuse_binfilter", binfilter)
        _probe(sv, o, f0, n, f"large deck shift {shift} binfilter {binfilter}")
        assert sv.contact_stats()["hash_buckets"] > 32768


# ---- 5. decision boundaries ----------------------------------------------------------------------
@pytest.mark.parametrize("name", list(cc.SWEEPS))
def test_decision_boundaries(name):
    """Every point of the sweep: the reference decides, the device must agree in bits and count."""
    m, k, pts = cc.SWEEPS[name]()
    ref = ContactRef(m)
    with Solver(m) as sv:
        for label, pos in pts:
            o, f, n = _reference(m, pos, ref=ref)
            _probe(sv, o, f, n, f"{name} {label}")


# ---- 6. zero-area triangle -----------------------------------------------------------------------
def test_zero_area_triangle():
    """mag_n == 0: a NaN normal, which no comparison of the event test passes. No event from the
    degenerate triangles, events from the others, a finite force. (The restatement divides with
    IEEE semantics there, contact_ref._ieee_div.)"""
    m, pos, _ = cc.degenerate_plate()
    o, f, n = _reference(m, pos, ref=_restatement(("h4", None)))
    assert n > 0 and np.all(np.isfinite(f))
    with Solver(m) as sv:
        g = _probe(sv, o, f, n, "zero-area triangle")
    assert np.all(np.isfinite(g))


# ---- 7. velocity sources -------------------------------------------------------------------------
def test_velocity_from_displacements():
    """After real steps the device forms the velocity as (disp - disp_pre) / d_time. The element
    update of the device agrees with the oracle to rounding, not in bits, so the reference is
    evaluated at the device's own downloaded state with that same expression; the oracle's run
    must be the same trajectory to 1e-9."""
    m = cc.mixed_two_body()
    o = O.Oracle(m)
    o.run(1, 3)
    with Solver(m) as sv:
        sv.step(1, 3)
        st = sv.download()
        g = sv.contact_force(4)
        ev = sv.contact_stats()["events"]
    scale = np.max(np.abs(o.s["disp"]))
    assert np.max(np.abs(st.disp - o.s["disp"])) < 1e-9 * scale
    o2 = O.Oracle(m)
    o2.s["disp"][:] = st.disp
    o2.s["disp_pre"][:] = st.disp_pre
    o2.s["velo"][:] = (st.disp - st.disp_pre) / m.dt
    o2.s["position"][:] = m.coordmat + st.disp.reshape(-1, 3)
    o2.s["element_flag"][:] = st.element_flag
    f, n = o2.contact_force()
    fr, nr = _restatement(("h4", None)).force(o2.s["position"], o2.s["velo"], o2.diag_M, o2.s["element_flag"])
    assert n == nr and n > 0 and np.array_equal(f, fr)
    print(f"after 3 steps: events {ev} (reference {n})")
    assert np.array_equal(g, f) and ev == n
