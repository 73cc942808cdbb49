"""The nodal update, the boundary conditions and the amplitudes on the CPU: the restatement of
tests/nodal_ref.py against exact rationals under its derived rounding bound, the oracle against the
restatement bit for bit, and the proof that the crafted decks of tests/nodal_cases.py hit every
branch they are meant to (tests/test_gpu_nodal_bc.py runs the same decks on the device)."""
from fractions import Fraction

import numpy as np
import pytest

import nodal_cases as C
import nodal_ref as R
import oracle as O
from hakai.model import BCGroup, read_inp
from util import bits, bitwise_equal

NN0 = C.probe_bars()[0][1].nNode


@pytest.fixture(scope="module")
def states():
    return C.probe_states(NN0, seed=1)


def test_probe_states_hold_what_they_claim(states):
    by = {s[0]: s for s in states}
    assert tuple(by) == C.PROBE_SETS
    for name, m, u, up, q in states:
        assert all(np.isfinite(x).all() for x in (m, u, up, q)) and np.all(m != 0.0), name
        assert np.any(m < 0) and np.any(m > 0)
        assert np.array_equal(m.reshape(-1, 3)[:, 0], m.reshape(-1, 3)[:, 1])
    _, _, u, up, q = by["cancel"]
    assert np.any(2.0 * u - up == 0.0) and np.any(np.abs(2.0 * u - up) == np.spacing(np.abs(2.0 * u)))
    assert np.any((2.0 * u - up == 0.0) & (q == 0.0))
    _, _, u, up, q = by["subnormal_q"]
    assert np.all((q != 0) & (np.abs(q) < 2.0 ** -1022)) and np.any(u == 0.0) and np.any(u != 0.0)
    _, _, u, up, q = by["huge_tiny"]
    for x in (u, up, q):
        assert np.any(np.abs(x) > 1e149) and np.any(np.abs(x) < 1e-149)
    _, _, u, up, q = by["zeros"]
    for x in (u, up, q):
        assert np.any((x == 0) & np.signbit(x)) and np.any((x == 0) & ~np.signbit(x)) and np.any(x != 0)
    # every dof of the random set has its own expected value, different from what the buffer held
    _, m, u, up, q = by["random"]
    x = R.nodal_step(m, C.D_TIME, u, up, q, np.zeros_like(u))
    assert np.unique(x).size == x.size and np.all(x != up) and np.all(x != u)


@pytest.mark.parametrize("k", range(len(C.PROBE_SETS)), ids=C.PROBE_SETS)
def test_restatement_within_derived_bound_of_exact(states, k):
    """nodal_step against the unrounded value, dof by dof, in exact rationals: at most COUNT = 8
    roundings of 2^-53 relative to the dof's magnitude sum (nodal_ref's docstring)."""
    name, m, u, up, q = states[k]
    f = np.zeros_like(u)
    x = R.nodal_step(m, C.D_TIME, u, up, q, f)
    assert np.isfinite(x).all()
    X, S, inv_A = R.nodal_terms(m, C.D_TIME, u, up, q, f)
    bound = R.nodal_bound(S, inv_A)
    worst = Fraction(0)
    for i in range(x.size):
        err = abs(Fraction(float(x[i])) - X[i])
        assert err <= bound[i], f"{name} dof {i}: {float(err):.3e} > {float(bound[i]):.3e}"
        if S[i]:
            worst = max(worst, err / (R.U * S[i]))
    print(f"{name}: worst error {float(worst):.3f} x 2^-53 x S (bound {R.COUNT})")
    # the once-rounded exact value lies within the same bound of the restatement, and is what the
    # restatement returns wherever nothing cancels
    xe = R.nodal_exact(m, C.D_TIME, u, up, q, f)
    assert np.isfinite(xe).all()
    assert np.all(np.abs(xe - x) <= np.array([float(b) for b in bound]) * (1 + 2.0 ** -50) + np.spacing(np.abs(xe)))


def test_nodal_step_with_a_force_term():
    """f enters as f - Q: the restatement with f, Q equals the one with 0, Q - f where that
    difference is exact, and stays within the bound of the exact value."""
    rng = np.random.default_rng(5)
    n = 60
    m = np.repeat(rng.uniform(1e-9, 1e-8, n // 3), 3)
    u, up = rng.normal(0, 1e-2, n), rng.normal(0, 1e-2, n)
    f, q = rng.integers(-2 ** 20, 2 ** 20, n) / 64.0, rng.integers(-2 ** 20, 2 ** 20, n) / 64.0
    x = R.nodal_step(m, C.D_TIME, u, up, q, f)
    assert bitwise_equal(x, R.nodal_step(m, C.D_TIME, u, up, q - f, np.zeros(n)))
    X, S, inv_A = R.nodal_terms(m, C.D_TIME, u, up, q, f)
    for xi, Xi, b in zip(x, X, R.nodal_bound(S, inv_A)):
        assert abs(Fraction(float(xi)) - Xi) <= b


def test_amplitude_rules():
    """:588-599 on a table small enough to evaluate by hand."""
    t, v = [1.0, 2.0, 2.0, 4.0], [0.0, 1.0, 0.5, 0.25]
    assert R.amplitude(t, v, 1.5) == 0.5
    assert R.amplitude(t, v, 2.0) == 1.0          # on a breakpoint: the first matching segment
    assert R.amplitude(t, v, 3.0) == 0.375        # the last segment (the zero-length one holds 2.0 only)
    assert R.amplitude(t, v, 0.0) == -1.0         # before the table: the first segment, extrapolated
    assert R.amplitude(t, v, 5.0) == 4.0          # after it: the first segment again
    assert R.amplitude([0.0, 3.0, 1.0, 6.0], [0.0, 1.0, -1.0, 2.0], 2.0) == 2.0 / 3.0  # non-monotonic: break
    with pytest.raises(IndexError):
        R.amplitude([1.0], [1.0], 1.0)


def test_bc_deck_self_check():
    m = C.bc_deck()
    C.check_deck(m)
    assert [g.amp_time is None for g in m.bc] == [True, False, True, False, True, False, False]
    m12 = C.bc_deck(nz=12)
    C.check_deck(m12)
    npl = 12
    iface = set(range(6 * npl, 7 * npl))          # the two-rank cut of the 12-layer deck
    on_iface = {d // 3 for d in C.resolved(m12)} & iface
    assert len(on_iface) == npl, "prescribed dofs on every interface node"
    assert {g for d, (g, _) in C.resolved(m12).items() if d // 3 in iface} >= {2, 5}
    w = C.bc_deck_wide()
    C.check_deck(w, subsets=False, writers_differ=False)
    n = len(C.resolved(w))
    assert n > 256 and n % 256 != 0, n
    # the rollers and every later group share dofs, so alternating groups with and without amplitude
    # are all live in the resolved list
    assert {g for g, _ in C.resolved(w).values()} == set(range(8))
    assert {g for g, _ in C.resolved(m).values()} == set(range(7))


def _oracle_step_equals_restatement(o, m, t):
    s = o.s
    x = R.nodal_step(o.diag_M, m.dt, s["disp"], s["disp_pre"], s["Q"], np.zeros(3 * m.nNode))
    R.apply_bc(m, float(t) * m.dt, x)
    o.run(t, 1)
    assert np.array_equal(bits(s["disp"]), bits(x)), f"step {t}: {np.flatnonzero(bits(s['disp']) != bits(x))[:8]}"
    return x


@pytest.mark.parametrize("deck", ["bc_deck", "bc_deck_12", "bc_deck_wide"])
def test_oracle_equals_restatement_every_step(deck):
    """The oracle's :564 and :585-617 against nodal_ref, from the oracle's own state before each
    step, bit for bit, signed zeros included."""
    m = {"bc_deck": C.bc_deck, "bc_deck_12": lambda: C.bc_deck(nz=12), "bc_deck_wide": C.bc_deck_wide}[deck]()
    o = O.Oracle(m)
    neg0 = 0
    for t in range(1, (C.N_STEPS if deck != "bc_deck_wide" else 40) + 1):
        x = _oracle_step_equals_restatement(o, m, t)
        neg0 += int(np.sum((x == 0) & np.signbit(x)))
    assert neg0 > 0, "no -0.0 displacement"
    for k, a in o.s.items():
        assert np.isfinite(a).all(), k


@pytest.mark.parametrize("bc", [False, True], ids=["free", "bc"])
@pytest.mark.parametrize("k", range(len(C.PROBE_SETS)), ids=C.PROBE_SETS)
def test_oracle_equals_restatement_on_probe_states(states, k, bc):
    name, mass, u, up, q = states[k]
    m = C.probe_bars()[0][1]
    if bc:
        m.bc = C.probe_bc(m)
    o = O.Oracle(m)
    o.diag_M[:] = mass
    o.s["disp"][:], o.s["disp_pre"][:], o.s["Q"][:] = u, up, q
    x = _oracle_step_equals_restatement(o, m, 1)
    assert np.isfinite(x).all()
    if bc:
        res = C.resolved(m)
        per_node = {}
        for d in res:
            per_node.setdefault(d // 3, set()).add(d % 3)
        assert len({frozenset(s) for s in per_node.values()}) == 7 and {0, m.nNode - 1} <= set(per_node)


def test_oracle_rejects_one_point_amplitude():
    m = C.bc_deck()
    m.bc.insert(3, BCGroup([(np.array([40 * 3], np.int64), 1.0)], np.array([C.T(3)]), np.array([1.0])))
    with pytest.raises(ValueError):
        O.Oracle(m)


def test_inp_round_trip_keeps_groups_tables_and_order(tmp_path):
    from inp_writer import write_inp
    m = C.bc_deck()
    r = read_inp(write_inp(str(tmp_path / "bc_deck.inp"), m))
    assert len(r.bc) == len(m.bc)
    for a, b in zip(m.bc, r.bc):
        assert (a.amp_time is None) == (b.amp_time is None)
        if a.amp_time is not None:
            assert bitwise_equal(np.asarray(a.amp_time), b.amp_time) and bitwise_equal(np.asarray(a.amp_value), b.amp_value)
        assert len(a.entries) == len(b.entries)
        for (da, va), (db, vb) in zip(a.entries, b.entries):
            assert np.array_equal(np.asarray(da, np.int64), db) and bitwise_equal(np.float64(va), np.float64(vb))
    assert r.dt == m.dt and r.n_steps == m.n_steps
    assert C.resolved(r) == C.resolved(m)
