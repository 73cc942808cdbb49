"""The output chain on the device -- k_node_average, hakai_node_stress_strain, the driver's fill of the
writer's buffers, the files -- against references that share nothing with it:

a. the kernel alone on the crafted cases of output_cases.py against output_ref.node_average (written
   from v2/HAKAI_j.jl:3408-3486; tests/test_output_ref_cpu.py ties it to the oracle and to the exact
   value), and the C entry's optional outputs and state check;
b. the device's own state on, one step after and forty steps after a deletion step -- three code
   paths of the triaxiality store -- and that an output between two calls changes nothing;
c. hakai_negative_jacobians as a count;
d. every file HAKAI(fname) writes against vtk_ref.serial_vtk of the oracle's state at that output.

Comparisons are bit or byte equality, except the triaxiality: the device forms it from the
invariants, the reference from closed-form eigenvalues (tests/test_gpu_exact.py), so the Gauss-point
array is held to that file's 1e-12 and the printed block to one unit of the last printed digit.
"""
import ctypes
import functools
import os
from decimal import Decimal

import numpy as np
import pytest

import hakai
from hakai import _abi, mesh
from hakai._abi import check, ptr
from hakai.model import Model
from hakai.solver import Solver, State
import oracle as O
import output_cases as C
import output_ref as R
from inp_writer import write_inp
from util import fast_deletion_bar, rel_err, same_state, small_bar
from vtk_ref import TRIAX_HEADER, serial_vtk

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _ref(name):
    return R.node_average(*C.args(C.case(name)))


def _case_state(c) -> State:
    st = State.empty(c.model.nNode, c.model.nElement)
    st.integ_stress[:] = c.stress
    st.integ_strain[:] = c.strain
    st.integ_eq_plastic_strain[:] = c.eqps
    st.integ_triax_stress[:] = c.triax
    st.element_flag[:] = c.flag
    return st


def _case_solver(c) -> Solver:
    sv = Solver(c.model, diag_M=np.ones(3 * c.model.nNode))  # (a node no element uses has no mass of its own)
    sv.upload(_case_state(c))
    return sv


def _assert_fields(got, want, what, fields=R.FIELDS):
    for k in fields:
        assert R.same_bits(got[k], want[k]), (what, k)


# ---- a. the kernel alone ------------------------------------------------------------------------
@pytest.mark.parametrize("name", C.names())
def test_node_average_equals_restatement(name):
    c = C.case(name)
    with _case_solver(c) as sv:
        g = sv.node_stress_strain()
    _assert_fields(g, _ref(name), name)


def test_node_stress_strain_optional_outputs_and_repeat():
    """Each output pointer alone (Mises alone needs the stress average internally), none at all,
    and the same bits from a second call. shuffled_dup257: two blocks, CSR incidences, a NaN node."""
    name = "shuffled_dup257"
    c = C.case(name)
    nN = c.model.nNode
    want = _ref(name)
    L = hakai.lib()
    shapes = [(nN, 6), (nN, 6), (nN,), (nN,), (nN,)]
    order = ("node_stress", "node_strain", "node_eq_plastic_strain", "node_mises_stress", "node_triax_stress")
    with _case_solver(c) as sv:
        for i, k in enumerate(order):
            a = np.full(shapes[i], 123.0)
            args = [None] * 5
            args[i] = ptr(a)
            check(L.hakai_node_stress_strain(sv.ctx, *args))
            assert R.same_bits(a, want[k]), k
        check(L.hakai_node_stress_strain(sv.ctx, None, None, None, None, None))
        g1, g2 = sv.node_stress_strain(), sv.node_stress_strain()
    _assert_fields(g1, want, "first call")
    _assert_fields(g2, want, "second call")


def test_node_stress_strain_before_any_state():
    L = hakai.lib()
    ctx = ctypes.c_void_p()
    check(L.hakai_create(ctypes.byref(ctx), 0))
    try:
        a = np.zeros(8)
        assert L.hakai_node_stress_strain(ctx, None, None, ptr(a), None, None) == _abi.HAKAI_ERR_STATE
        assert L.hakai_node_stress_strain(ctx, None, None, None, None, None) == _abi.HAKAI_ERR_STATE
    finally:
        L.hakai_destroy(ctx)


# ---- b. the device's own state at the three deletion moments ---------------------------------------
LATER = 40


@functools.lru_cache(maxsize=None)
def _deletion_moments():
    """fast_deletion_bar: s, the oracle's first deletion step, the 0-based elements deleted at s, and
    copies of the oracle's state after s, s + 1 and s + LATER steps."""
    m = fast_deletion_bar()
    probe = O.Oracle(m)
    probe.run(1, m.n_steps)
    assert probe.deletions
    s = min(int(t) for t, _ in probe.deletions)
    dead = np.array(sorted(int(e) - 1 for t, e in probe.deletions if t == s))
    assert 100 < s and s + LATER < m.n_steps
    o = O.Oracle(m)
    states, t = {}, 0
    for upto in (s, s + 1, s + LATER):
        o.run(t + 1, upto - t)
        t = upto
        states[upto] = {k: v.copy() for k, v in o.s.items()}
    assert o.deletions == [d for d in probe.deletions if d[0] <= s + LATER]
    return m, s, dead, states


def _average_of(m, s):
    """The restatement on a state given as the oracle's dict or a downloaded State."""
    get = (lambda k: s[k]) if isinstance(s, dict) else (lambda k: getattr(s, k))
    return R.node_average(m.nNode, m.elementmat, get("integ_stress"), get("integ_strain"),
                          get("integ_eq_plastic_strain"), get("integ_triax_stress"))


def _gp(a, dead):
    return a.reshape(-1, 8, *a.shape[1:])[dead]


def _check_moment(m, sv, os_, dead, at_deletion, exact, what):
    g = sv.download()
    avg = sv.node_stress_strain()
    own = _average_of(m, g)
    if exact:
        _assert_fields(avg, _average_of(m, os_), what, ("node_stress", "node_strain", "node_eq_plastic_strain",
                                                         "node_mises_stress"))
        assert R.same_bits(avg["node_triax_stress"], own["node_triax_stress"]), what
        assert rel_err(g.integ_triax_stress, os_["integ_triax_stress"]) < 1e-12, what
    else:
        _assert_fields(avg, own, what)
    assert np.all(g.element_flag[dead] == 0), what
    assert np.all(_gp(g.integ_stress, dead) == 0.0) and np.all(_gp(g.integ_strain, dead) == 0.0), what
    assert np.any(_gp(g.integ_eq_plastic_strain, dead) != 0.0), what
    tri = _gp(g.integ_triax_stress, dead)
    if at_deletion:
        assert np.all(tri != 0.0), (what, tri)
    else:
        assert np.all(tri == 0.0), (what, tri)


@pytest.mark.parametrize("exact", [1, 0])
def test_node_averages_on_and_after_a_deletion_step(exact):
    """On the deletion step the deleted elements' stress is zero and their triaxiality is still the
    step's (v2/HAKAI_j.jl:701-746); one step later it is zero; forty steps later, reached in ONE call
    with the deletion inside captured graphs, it is zero as well. elem_exact = 1: the averages are
    the restatement's on the oracle's state, the triaxiality average the restatement's on the
    device's own triaxiality. elem_exact = 0 (the fused kernel): all five are the restatement's on
    the device's own download."""
    m, s, dead, states = _deletion_moments()
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", exact)
        sv.step(1, s)
        assert [tuple(int(v) for v in d) for d in sv.deleted()] == [(s, int(e) + 1) for e in dead]
        _check_moment(m, sv, states[s], dead, True, exact, "at s")
        sv.step(s + 1, 1)
        _check_moment(m, sv, states[s + 1], dead, False, exact, "at s + 1")
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", exact)
        sv.step(1, s + LATER)
        assert sv.graph_steps() > 0
        _check_moment(m, sv, states[s + LATER], dead, False, exact, "at s + %d" % LATER)


@pytest.mark.parametrize("exact", [1, 0])
def test_output_does_not_disturb_the_run(exact):
    m = fast_deletion_bar()
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", exact)
        sv.step(1, 100)
        sv.node_stress_strain()
        sv.step(101, 100)
        a = sv.download()
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", exact)
        sv.step(1, 200)
        b = sv.download()
    same_state(a, b)
    assert np.array_equal(a.velo, b.velo)


# ---- c. hakai_negative_jacobians as a count ----------------------------------------------------------
@pytest.mark.parametrize("nE", [31, 32, 33])
def test_negative_jacobians_counts_gauss_points(nE):
    """k_negjac runs blocks of 256 over 8 nE Gauss points: 248, 256, and 264 with the last element
    alone in a second block. The last element is the mirrored one."""
    base = small_bar(1, 1, nE, n_steps=1)
    mirror = [4, 5, 6, 7, 0, 1, 2, 3]

    def solver(em):
        m = Model(base.coordmat.copy(), em, base.element_material.copy(), base.materials, d_time=base.d_time,
                  end_time=base.end_time)
        return Solver(m, diag_M=np.ones(3 * m.nNode))
    with solver(base.elementmat[:, mirror].copy()) as sv:
        assert sv.negative_jacobians() == 8 * nE
    with solver(base.elementmat.copy()) as sv:
        assert sv.negative_jacobians() == 0
    em = base.elementmat.copy()
    em[nE - 1] = em[nE - 1, mirror]
    with solver(em) as sv:
        assert sv.negative_jacobians() == 8
        st = sv.download()
        st.element_flag[nE - 1] = 0
        sv.upload(st)
        assert sv.negative_jacobians() == 0


# ---- d. whole files from the driver ------------------------------------------------------------------
def _split(b: bytes):
    i = b.index(TRIAX_HEADER) + len(TRIAX_HEADER)
    assert b.count(TRIAX_HEADER) == 1 and b.endswith(b"\n")
    return b[:i], b[i:].decode().split("\n")[:-1]


def _assert_file(got: bytes, want: bytes, nN: int, what):
    """Byte for byte outside the TRIAX_STRESS block (the file's last); inside it every value within
    one unit of the last digit "%1.6e" prints of the rendering, and no NaN or Inf (every node of
    these decks has an element)."""
    gh, gt = _split(got)
    wh, wt = _split(want)
    assert gh == wh, what
    assert len(gt) == len(wt) == nN, what
    for n, (a, b) in enumerate(zip(gt, wt)):
        if a == b:
            continue
        assert "N" not in a + b and "I" not in a + b, (what, n, a, b)
        unit = Decimal(1).scaleb(int(b[b.index("e") + 1:]) - 6)
        assert abs(Decimal(a) - Decimal(b)) <= unit, (what, n, a, b)
    assert not any("N" in x or "I" in x for x in gt + wt), what


def _drive_both(tmp_path, model):
    """HAKAI(fname) on the deck written from `model`, and the oracle in the driver's own chunks
    (v2/HAKAI_j.jl:471-472, :932-942: state 0, then every d_out = floor(time_num / 100) steps).
    Returns the read model, the oracle, [(step, oracle state copy)] per output and the files'
    bytes; every file is compared here."""
    deck = write_inp(str(tmp_path / "deck.inp"), model)
    out = tmp_path / "out"
    hakai.hakai(deck, str(out), verbose=False)
    m = hakai.read_inp(deck)
    n_steps, d_out = m.n_steps, int(np.floor(m.time_num / 100))
    assert d_out >= 1 and n_steps // d_out == 100
    files = sorted(os.listdir(out))
    assert files == ["file%03d.vtk" % i for i in range(101)]
    o = O.Oracle(m)
    outputs, got = [], []
    for i in range(101):
        if i:
            o.run((i - 1) * d_out + 1, d_out)
        r = o.node_stress_strain()
        s = o.s
        want = serial_vtk(m.coordmat, m.elementmat, s["element_flag"], s["disp"], s["velo"], r["node_stress"],
                          r["node_strain"], r["node_eq_plastic_strain"], r["node_mises_stress"],
                          r["node_triax_stress"])
        b = (out / files[i]).read_bytes()
        _assert_file(b, want, m.nNode, files[i])
        outputs.append((i * d_out, {k: s[k].copy() for k in ("element_flag", "integ_stress", "integ_triax_stress")}))
        got.append(b)
    return m, o, outputs, got


def test_driver_files_tensile5e(tmp_path):
    """Tensile5e: one deletion, at step 15153, between the outputs of steps 15000 and 15200."""
    m, o, outputs, got = _drive_both(tmp_path, mesh.tensile5e_model())
    assert o.deletions == [(15153, 3)] and outputs[76][0] == 15200
    assert b"\nCELLS 5 45\n" in got[75] and b"\nCELLS 4 36\n" in got[76]


def test_driver_files_contact_deck_with_outputs_on_deletion_steps(tmp_path):
    m, o, outputs, got = _drive_both(tmp_path, C.contact_deck())
    d_out = outputs[1][0]
    del_steps = {int(t) for t, _ in o.deletions}
    on = [(i, t) for i, (t, _) in enumerate(outputs) if t in del_steps]
    assert on, (sorted(del_steps), d_out)
    for i, t in on:
        s = outputs[i][1]
        dead = np.array([int(e) - 1 for tt, e in o.deletions if tt == t])
        assert np.all(s["element_flag"][dead] == 0)
        assert np.all(_gp(s["integ_stress"], dead) == 0.0)
        assert np.any(_gp(s["integ_triax_stress"], dead) != 0.0, axis=1).all(), (i, t)
        assert b"\nCELLS %d " % int(s["element_flag"].sum()) in got[i]


def test_driver_files_mass_scaled_bar(tmp_path):
    """The Vx-Vz blocks pin velo = d_disp / (increment * sqrt(mass_scaling)) (v2/HAKAI_j.jl:114, :628)."""
    m, o, outputs, got = _drive_both(tmp_path, C.mass_scaled_bar())
    assert m.mass_scaling == 4.0 and m.dt == 2e-7 and m.n_steps == 200
    # not vacuous: a velocity formed with the deck's increment would print differently
    lines = got[100].decode().split("\n")
    i = lines.index("SCALARS Vz float 1")
    vz = np.array([float(x) for x in lines[i + 2:i + 2 + m.nNode]])
    assert np.max(np.abs(vz)) > 1e3
