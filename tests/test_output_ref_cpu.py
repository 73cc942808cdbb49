"""The output node averages on the CPU: output_ref.node_average (written from
cal_node_stress_strain, v2/HAKAI_j.jl:3408-3486) against the oracle's hko_node_stress_strain bit for
bit on every case of output_cases.py, against the exact rational value within the derived rounding
bound, and the rules of the reference on this path stated one by one. tests/test_gpu_output.py
runs the same cases on the device. Host code only, no GPU."""
from fractions import Fraction

import numpy as np
import pytest

import oracle as O
import output_cases as C
import output_ref as R
from oracle import _p
from ctypes import c_int64

FINITE_CASES = ("n8", "n255", "n256", "n257", "n513", "dup16", "shuffled", "shuffled_dup257", "deleted", "cancel",
                "zeros", "subnormal", "mises")


def oracle_average(nN, em, stress, strain, eqps, triax):
    em = np.ascontiguousarray(em, np.int64)
    a = [np.ascontiguousarray(x, np.float64) for x in (stress, strain, eqps, triax)]
    out = dict(node_stress=np.zeros((nN, 6)), node_strain=np.zeros((nN, 6)), node_eq_plastic_strain=np.zeros(nN),
               node_mises_stress=np.zeros(nN), node_triax_stress=np.zeros(nN))
    O.lib().hko_node_stress_strain(nN, em.shape[0], _p(em, c_int64), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]),
                                   _p(out["node_stress"]), _p(out["node_strain"]),
                                   _p(out["node_eq_plastic_strain"]), _p(out["node_mises_stress"]),
                                   _p(out["node_triax_stress"]))
    return out


@pytest.fixture(scope="module")
def ref():
    """name -> node_average of the case, computed once."""
    return {c.name: R.node_average(*C.args(c)) for c in C.cases()}


def test_case_list():
    assert set(FINITE_CASES) | {"huge", "nan_gp", "inf_pair"} == set(C.names())
    for c in C.cases():
        finite = all(np.isfinite(a).all() for a in (c.stress, c.strain, c.eqps, c.triax))
        assert finite == (c.name not in ("nan_gp", "inf_pair")), c.name
    assert np.bincount(C.case("dup16").model.elementmat.ravel()).max() == 16
    assert np.bincount(C.case("shuffled_dup257").model.elementmat.ravel()).max() == 16
    assert np.bincount(C.case("n513").model.elementmat.ravel()).max() == 8


@pytest.mark.parametrize("name", C.names())
def test_restatement_equals_oracle_bit_for_bit(name, ref):
    c = C.case(name)
    o = oracle_average(*C.args(c))
    for k in R.FIELDS:
        assert R.same_bits(ref[name][k], o[k]), (name, k)


@pytest.mark.parametrize("name", FINITE_CASES)
def test_restatement_within_the_rounding_bound_of_the_exact_value(name, ref):
    c = C.case(name)
    X, S, m, cnt = R.node_average_exact(*C.args(c))
    worst, checked = Fraction(0), 0
    for k in R.LINEAR:
        got = ref[name][k].reshape(c.model.nNode, -1)
        for n in range(c.model.nNode):
            if cnt[n] == 0:
                assert np.isnan(got[n]).all()
                continue
            for j in range(got.shape[1]):
                assert X[k][n, j] is not None and np.isfinite(got[n, j]), (name, k, n, j)
                err = abs(Fraction(float(got[n, j])) - X[k][n, j])
                bound = R.average_bound(S[k][n, j], m[n], cnt[n])
                assert err <= bound, (name, k, n, j, float(err), float(bound))
                worst = max(worst, err / bound)
                checked += 1
    assert checked == 14 * int(np.count_nonzero(cnt))
    print(f"{name}: worst error / bound = {float(worst):.3f} over {checked} values")


def test_overflow_is_outside_the_bound_and_shows(ref):
    """huge: every input is finite, the sums are not: +Inf where one sign overflows, NaN where an
    Inf meets the other sign, and the ordinary elements' nodes stay finite only where no huge
    element touches them."""
    r = ref["huge"]
    assert np.isposinf(r["node_stress"]).any() and np.isnan(r["node_stress"]).any()
    assert np.isfinite(r["node_stress"]).any()
    assert np.isnan(r["node_mises_stress"]).any() or np.isposinf(r["node_mises_stress"]).any()


def test_mises_known_answers(ref):
    for t, want in C.MISES_KNOWN:
        assert R.same_bits(R.mises(t), np.float64(want)), t
    c = C.case("mises")
    r = ref["mises"]
    for e, (t, want) in enumerate(C.MISES_KNOWN):
        nodes = c.model.elementmat[e] - 1
        assert R.same_bits(r["node_stress"][nodes], np.tile(np.array(t), (8, 1)))
        assert R.same_bits(r["node_strain"][nodes], np.tile(np.array(t)[::-1], (8, 1)))
        assert R.same_bits(r["node_mises_stress"][nodes], np.full(8, want)), (t, want)
        assert R.same_bits(r["node_eq_plastic_strain"][nodes], np.full(8, float(e)))
        assert R.same_bits(r["node_triax_stress"][nodes], np.full(8, 0.0 - e))   # the scatter's 0.0 + -0.0 is +0.0
    # the (ox - oz) term: a tensor that only differs there
    assert R.mises((1., 1., 3., 0., 0., 0.)) == 2.0


def test_unused_node_is_nan_in_all_five(ref):
    for name in ("n257", "shuffled_dup257"):
        c = C.case(name)
        last = c.model.nNode - 1
        assert last + 1 not in c.model.elementmat
        for k in R.FIELDS:
            a = ref[name][k]
            assert np.isnan(a[last]).all(), (name, k)
            assert np.isfinite(a[:last]).all(), (name, k)


def test_deleted_elements_count_in_the_divisor(ref):
    c = C.case("deleted")
    em, nN = c.model.elementmat, c.model.nNode
    assert np.array_equal(R.divisor(nN, em), np.bincount(em.ravel() - 1, minlength=nN))
    active = R.node_average(nN, em[c.flag == 1], *(a.reshape(-1, 8, *a.shape[1:])[c.flag == 1].reshape(-1, *a.shape[1:])
                                                   for a in (c.stress, c.strain, c.eqps, c.triax)))
    touched = np.zeros(nN, bool)
    touched[em[c.flag == 0].ravel() - 1] = True
    assert touched.any() and not touched.all()
    r = ref["deleted"]
    # a node of a deleted element: its stress average is the active elements' sum over ALL its elements
    shared = [n for n in np.nonzero(touched)[0] if np.isfinite(active["node_stress"][n]).all()]
    assert shared and all(not R.same_bits(r["node_stress"][n], active["node_stress"][n]) for n in shared)
    # and the deleted elements' eqps is in the average
    assert np.any(r["node_eq_plastic_strain"][touched] != active["node_eq_plastic_strain"][touched])
    assert R.same_bits(r["node_stress"][~touched], active["node_stress"][~touched])


def test_a_node_listed_twice_counts_once_in_the_divisor():
    """The literal form of :3458. The oracle and the kernel divide by the number of incidences
    instead; the two differ only for an element that lists a node twice (none of the committed decks
    has one)."""
    em = np.array([[1, 2, 3, 4, 5, 6, 7, 7]], np.int64)
    st = np.ones((8, 6))
    r = R.node_average(7, em, st, st, np.ones(8), np.ones(8))
    assert np.array_equal(R.divisor(7, em), np.ones(7))
    assert r["node_eq_plastic_strain"][6] == 2.0 and np.all(r["node_eq_plastic_strain"][:6] == 1.0)
    assert oracle_average(7, em, st, st, np.ones(8), np.ones(8))["node_eq_plastic_strain"][6] == 1.0


def test_the_sum_depends_on_element_order(ref):
    """shuffled is not vacuous: visiting the same elements in the reverse order changes bits, so a
    device incidence list in any order but the ascending one shows."""
    c = C.case("shuffled")
    nE = c.model.nElement
    rev = lambda a: a.reshape(nE, 8, *a.shape[1:])[::-1].reshape(a.shape)  # noqa: E731
    r2 = R.node_average(c.model.nNode, c.model.elementmat[::-1], rev(c.stress), rev(c.strain), rev(c.eqps),
                        rev(c.triax))
    for k in R.FIELDS:
        assert not R.same_bits(ref["shuffled"][k], r2[k]), k
    em = c.model.elementmat
    assert not np.array_equal(em, np.sort(em, axis=0))  # the numbering is not the structured one


def test_non_finite_values_reach_exactly_their_elements_nodes(ref):
    em = C.case("nan_gp").model.elementmat
    nN = C.case("nan_gp").model.nNode

    def nodes(e):
        x = np.zeros(nN, bool)
        x[em[e] - 1] = True
        return x
    r = ref["nan_gp"]
    a, b = C.NAN_ELEMENTS
    assert np.array_equal(np.isnan(r["node_stress"][:, 0]), nodes(a))
    assert np.array_equal(np.isnan(r["node_mises_stress"]), nodes(a))
    assert np.array_equal(np.isnan(r["node_eq_plastic_strain"]), nodes(b))
    assert np.isfinite(r["node_stress"][:, 1:]).all() and np.isfinite(r["node_strain"]).all()
    assert np.isfinite(r["node_triax_stress"]).all()
    r = ref["inf_pair"]
    a, b = C.INF_ELEMENTS
    assert np.array_equal(np.isnan(r["node_strain"][:, 1]), nodes(a))          # +Inf + -Inf in one sum
    assert np.isfinite(np.delete(r["node_strain"], 1, axis=1)).all()
    assert np.array_equal(np.isposinf(r["node_stress"][:, 0]), nodes(b))
    assert np.array_equal(np.isneginf(r["node_stress"][:, 2]), nodes(b))
    assert np.array_equal(np.isposinf(r["node_mises_stress"]), nodes(b))       # (Inf - -Inf)^2, no NaN
    assert np.isfinite(r["node_mises_stress"][~nodes(b)]).all()


def test_driver_decks_step_counts_and_deletions_on_output_steps(tmp_path):
    """The decks tests/test_gpu_output.py runs through the driver, read back by the reader: 100
    outputs of d_out = floor(time_num / 100) steps each; the mass-scaled bar steps 200 times with
    twice the deck's increment; the contact deck has outputs that land on deletion steps, each with a
    zero-stress, non-zero-triaxiality element behind it."""
    import hakai
    from hakai import mesh
    from inp_writer import write_inp
    want = {"tensile5e": (20000, 200), "contact": (400, 4), "scaled": (200, 2)}
    built = {"tensile5e": mesh.tensile5e_model(), "contact": C.contact_deck(), "scaled": C.mass_scaled_bar()}
    read = {}
    for k, model in built.items():
        m = hakai.read_inp(write_inp(str(tmp_path / (k + ".inp")), model))
        assert (m.n_steps, int(np.floor(m.time_num / 100))) == want[k], k
        assert np.bincount(m.elementmat.ravel(), minlength=m.nNode + 1)[1:].min() >= 1, k  # no unused node
        read[k] = m
    m = read["scaled"]
    assert m.mass_scaling == 4.0 and m.d_time == 1e-7 and m.dt == 2e-7
    assert len(set(m.ic_values)) > 4 and np.max(np.abs(m.ic_values)) > 1e5
    m = read["contact"]
    o = O.Oracle(m)
    hits = 0
    for i in range(1, 101):
        o.run(4 * (i - 1) + 1, 4)
        dead = np.array([int(e) - 1 for t, e in o.deletions if t == 4 * i], np.int64)
        if dead.size:
            hits += 1
            assert np.all(o.s["integ_stress"].reshape(-1, 8, 6)[dead] == 0.0)
            assert np.all(np.any(o.s["integ_triax_stress"].reshape(-1, 8)[dead] != 0.0, axis=1))
    assert hits >= 1, o.deletions
    print("contact deck deletions:", o.deletions)


def test_committed_decks_list_no_node_twice_and_use_every_node(ref_decks):
    """Where the reference's divisor and the incidence count agree (include/hakai_hip.h): none of the
    committed decks has an element that lists a node twice. None has an unused node either, so the
    0/0 = NaN rule shows in crafted meshes only."""
    import glob
    import os
    import hakai
    decks = sorted(glob.glob(os.path.join(ref_decks, "**", "*.inp"), recursive=True))
    assert len(decks) == 20
    for d in decks:
        m = hakai.read_inp(d)
        em = np.sort(m.elementmat, axis=1)
        assert not np.any(em[:, 1:] == em[:, :-1]), d
        assert np.array_equal(R.divisor(m.nNode, m.elementmat), np.bincount(m.elementmat.ravel() - 1, minlength=m.nNode)), d
        assert np.bincount(m.elementmat.ravel() - 1, minlength=m.nNode).min() >= 1, d
