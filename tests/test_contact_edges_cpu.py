"""The crafted contact states of tests/contact_cases.py on the CPU: the C oracle against the literal
exact-rational restatement (tests/contact_ref.py), bit for bit, with contact constants that make
the damping term and the stiffness factors live (Cr != 0, kc != 1, kc_o != kc_s), mixed element
sizes and points placed on the decision boundaries of the event test. tests/test_gpu_contact_edges.py
probes the device at exactly these states; here the reference side is pinned, and the conditions that
make those probes meaningful are asserted on the reference alone:
  * the spill decks put more than four events (kEvLocal, hakai_contact.hip) into one
    (pair, triangle, i-cell), i.e. one search thread;
  * the one-instance deck has events on its self pair;
  * every boundary sweep crosses its boundary: the probe node's set of (pair, triangle) events is
    not the same at every point of the sweep;
  * the shifted large decks have the unshifted deck's event count and force bits.
"""
from collections import Counter

import numpy as np
import pytest

import oracle as O
import contact_cases as cc
from contact_ref import ContactRef

# events, max events per (pair, triangle, i-cell): measured once with this builder, fixed since
EXPECT = {"h4": (85, 6), "h4_flag2": (85, 6), "h8": (293, 28), "small": (26, 4), "self": (60, 5)}
LARGE_EVENTS = 295


def _both(m, position=None, velo=None, log=None):
    o = O.Oracle(m)
    cc.set_state(o, position, velo)
    f, n = o.contact_force()
    fr, nr = ContactRef(m).force(o.s["position"].reshape(-1, 3), o.s["velo"], o.diag_M, o.s["element_flag"], log=log)
    return f, n, fr, nr


@pytest.mark.parametrize("name", list(cc.SMALL_DECKS))
def test_small_decks_oracle_equals_restatement(name):
    m = cc.mixed_two_body(**cc.SMALL_DECKS[name])
    log = []
    f, n, fr, nr = _both(m, velo=cc.noisy_velocity(m), log=log)
    assert n == nr == len(log)
    assert np.array_equal(f, fr), f"max |diff| {np.max(np.abs(f - fr))}"
    per_thread = max(Counter((p, t, cell) for p, t, cell, _ in log).values())
    assert (n, per_thread) == EXPECT[name]
    if name in ("h4", "h4_flag2", "h8", "self"):
        assert per_thread >= 5, "the deck must overflow a search thread's four event registers"
    o = O.Oracle(m)
    pairs = [(p["i_instance"], p["j_instance"]) for p in o.contact_pairs()]
    if name == "self":
        assert pairs == [(1, 1)] and n >= 1
    if name == "h4_flag2":
        assert pairs == [(1, 1), (1, 2), (2, 1), (2, 2)]


@pytest.mark.parametrize("params", [(0.25, 1.0, 1.0, 0.0, 0.0), cc.PARAMS, (0.5, 2.0, 0.5, 0.0625, 0.375)])
@pytest.mark.parametrize("flag", [1, 2])
def test_constants_oracle_equals_restatement(params, flag):
    """The constants reach the force: each set gives its own bits, and the oracle follows."""
    m = cc.mixed_two_body(params=params, flag=flag)
    f, n, fr, nr = _both(m, velo=cc.noisy_velocity(m))
    assert n == nr == 85 and np.array_equal(f, fr)
    m0 = cc.mixed_two_body(params=(0.25, 1.0, 1.0, 0.0, 0.0), flag=flag)
    f0, _, _, _ = _both(m0, velo=cc.noisy_velocity(m0))
    assert np.array_equal(f, f0) == (params == (0.25, 1.0, 1.0, 0.0, 0.0))


def test_self_pair_constants_are_the_self_ones():
    """On the one-instance deck only kc_s and Cr_s matter: changing kc_o / Cr_o leaves the bits,
    changing kc_s or Cr_s does not."""
    def run(params):
        m = cc.mixed_two_body(one_instance=True, params=params)
        f, n, fr, nr = _both(m, velo=cc.noisy_velocity(m))
        assert n == nr == 60 and np.array_equal(f, fr)
        return f
    base = run(cc.PARAMS)
    assert np.array_equal(base, run((0.25, 7.0, 0.75, 0.5, 0.25)))
    assert not np.array_equal(base, run((0.25, 1.5, 0.5, 0.125, 0.25)))
    assert not np.array_equal(base, run((0.25, 1.5, 0.75, 0.125, 0.5)))


@pytest.mark.parametrize("name", list(cc.SWEEPS))
def test_sweeps_cross_their_boundary(name):
    m, k, pts = cc.SWEEPS[name]()
    velo = cc.noisy_velocity(m)
    seen = set()
    for label, pos in pts:
        log = []
        f, n, fr, nr = _both(m, pos, velo, log)
        assert n == nr, label
        assert np.array_equal(f, fr, equal_nan=True), label
        assert np.all(np.isfinite(f)), label
        seen.add(frozenset((p, t) for p, t, _, i in log if i == k + 1))
    assert len(seen) >= 2, "the probe's events are the same at every point: the boundary is not crossed"
    assert any(s for s in seen), "the probe has no event anywhere in the sweep"


def test_sweep_points_hit_the_boundaries_exactly():
    """The crafted equalities hold in double, with the reference's own expressions."""
    import math
    m, k, pts = cc.sweep_cell()
    pos = dict(pts)["cell_x+0"]
    amn = pos[:, 0].min()
    assert amn == -1.0 and (pos[k, 0] - amn) / (1.0 * 1.1) == 1.0
    up = dict(pts)["cell_x+1"]
    assert math.ceil((up[k, 0] - amn) / (1.0 * 1.1)) == 2
    m, k, pts = cc.sweep_range_box()
    assert dict(pts)["rmx_x+0"][k, 0] == 3.0 == m.coordmat[:16, 0].max()
    m, k, pts = cc.sweep_sphere()
    q = [[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [2.0, 2.0, 1.0]]
    c = [(q[0][d] + q[1][d] + q[2][d]) / 3.0 for d in range(3)]
    norm = lambda a, b, z: math.sqrt(a * a + b * b + z * z)  # noqa: E731
    Rmax = max(norm(*(v[d] - c[d] for d in range(3))) for v in q)
    dpc = [norm(*(p[k] - c)) for _, p in pts]
    assert dict(zip((l for l, _ in pts), dpc))["sphere+0"] == Rmax and min(dpc) < Rmax < max(dpc)
    m, k, pts = cc.sweep_d_lim()
    d = [0.0 - p[k, 2] for _, p in pts]
    assert cc_d_lim(m) in d and min(d) < cc_d_lim(m) < max(d)
    m, k, pts = cc.sweep_edges()
    g = dict(pts)
    assert g["diagonal_y+0"][k, 0] == g["diagonal_y+0"][k, 1] == 1.25 and g["edge_y+0"][k, 1] == 1.0


def cc_d_lim(m):
    return ContactRef(m).min_size * 0.3


def test_zero_area_triangles_give_no_event_and_finite_force():
    m, pos, (a, b) = cc.degenerate_plate()
    log = []
    f, n, fr, nr = _both(m, pos, cc.noisy_velocity(m), log)
    assert n == nr and n > 0
    assert np.all(np.isfinite(f)) and np.array_equal(f, fr)
    ref = ContactRef(m)
    for p, t, _, _ in log:
        tri = ref.ct[p]["tri"][t]
        assert not (a + 1 in tri and b + 1 in tri), "an event on a zero-area triangle"
    assert any(a + 1 in t and b + 1 in t for c in ref.ct for t in c["tri"])


def test_large_deck_literal_equals_indexed_and_shifts_keep_the_bits():
    """The 64x64 plate (8450 plate i-nodes: the device's large-deck search). ContactRef's O(F^2)
    surface scan is too slow here, so the literal oracle is held against the indexed one. Under an
    exact shift of every coordinate all the differences the contact expressions form are the same,
    so the event count is the unshifted deck's, and so are the force bits once the damping term
    reads the same mass: the lumped mass itself is integrated from the absolute coordinates and
    moves by 1e-9 (2^20) to 1e-6 (2^30) relative under the shift, which is the element side's
    business, so the shifted runs are given the unshifted deck's mass."""
    out = []
    mass0 = None
    for shift in [(0, 0, 0)] + cc.SHIFTS:
        m = cc.mixed_two_body(**cc.LARGE, shift=shift)
        assert m.nElement == 4608
        # the shift is exact: the shifted coordinates minus the shift are the unshifted ones
        m0 = cc.mixed_two_body(**cc.LARGE)
        assert np.array_equal(m.coordmat - np.asarray(shift, np.float64), m0.coordmat)
        v = cc.noisy_velocity(m)
        a, b = O.Oracle(m), O.Oracle(m, contact_indexed=True)
        if mass0 is None:
            mass0 = a.diag_M.copy()
        for o in (a, b):
            o.diag_M[:] = mass0
            cc.set_state(o, velo=v)
        fa, na = a.contact_force()
        fb, nb = b.contact_force()
        assert na == nb == LARGE_EVENTS and np.array_equal(fa, fb)
        out.append(fa)
    assert np.array_equal(out[0], out[1]) and np.array_equal(out[0], out[2])


def test_velocity_sources_after_steps():
    """After three steps the oracle's state (the device then forms the velocity from disp -
    disp_pre) still agrees with the restatement, with events."""
    m = cc.mixed_two_body()
    o = O.Oracle(m)
    o.run(1, 3)
    f, n = o.contact_force()
    fr, nr = ContactRef(m).force(o.s["position"].reshape(-1, 3), o.s["velo"], o.diag_M, o.s["element_flag"])
    assert n == nr and n > 0 and np.array_equal(f, fr)
