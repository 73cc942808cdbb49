"""The element-set history on the GPU (hakai_elem_history_*, csrc/hakai_elem_history.hip) against the
host-compiled header (csrc/hakai_elem_history_gp.hpp) and its NumPy restatement (elem_history_ref).

Per element the probe's 20 values equal the header's bit for bit. A set record is then checked from
per-element values (check_record):
  * counts, extremes, ids and J_min exactly;
  * fields 2-18 within d u sum|term| of the exactly rounded sum (math.fsum) of the per-element
    values, u = 2^-53. d: the kernel's tree over the element numbers adds 3 times inside a wave (8
    elements), twice over the 4 waves of a 32-element chunk and ceil(log2(chunks)) times over the
    chunks, so a value passes through depth = 5 + ceil(log2(ceil(nE / 32))) additions, each with a
    relative rounding of at most u on a partial sum that sum|term| bounds; d = depth + 2, one for the
    reference's own rounding and one for the second-order terms. small_bar (36 elements): d = 8; 2049
    elements: d = 14. The combination of R ranks adds R - 1 more.
"""
import ctypes
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import edge_cases
import elem_history_ref as R
import hakai
from hakai import _abi, dist, mesh
from hakai.model import Material, Model
from hakai.solver import Solver, State, elem_history_combine, elem_history_group, read_elem_history_csv
from history_ranks import build_group, close_group, step as group_step
from test_elem_history_cpu import CXXFLAGS, PKG, SRC, Header
from util import bitwise_equal, fast_deletion_bar, random_state, same_state, small_bar

pytestmark = pytest.mark.gpu
U = R.U


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    d = tmp_path_factory.mktemp("elem_history_gpu")
    c, so = d / "elem_history.cpp", d / "elem_history.so"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", os.path.join(PKG, "csrc"), "-o", str(so), str(c),
                    os.path.join(PKG, "host", "hakai_elem_history_host.cpp")], check=True)
    return Header(ctypes.CDLL(str(so)))


def tuned(m, tune=None, **kw):
    sv = Solver(m, **kw)
    for k, v in (tune or {}).items():
        sv.set_tuning(k, v)
    return sv


def restate(m, st):
    """Per-element values (nE, 20) of a downloaded / crafted state, zeros for inactive elements, and
    the flags."""
    pe = R.model_elements(m, st.disp, st.integ_stress, st.integ_strain, st.integ_eq_plastic_strain)
    flag = np.asarray(st.element_flag)
    pe[flag != 1] = 0.0
    return pe, flag


def check_record(val, pe, flag, sets, nE, extra=0, elem_offset=0, deleted=None):
    """One record (S, 24) against the restatement's per-element values (module docstring)."""
    ref, mag = R.record(pe, flag, (flag != 1) if deleted is None else deleted, sets, elem_offset)
    assert val.shape == ref.shape
    assert bitwise_equal(val[:, R.EXACT], ref[:, R.EXACT]), (val[:, R.EXACT], ref[:, R.EXACT])
    d = R.tree_depth(nE) + 2 + extra
    err, bound = np.abs(val[:, R.SUMS] - ref[:, R.SUMS]), d * U * mag[:, R.SUMS]
    assert np.all(err <= bound), float(np.max(err / np.maximum(bound, 1e-300)))


def crafted_state(m, seed, disp_scale=0.03, pos=None):
    """A random state with the edge values of check 1: -0.0, a subnormal stress, eqps exactly on a
    breakpoint, an inactive element that still carries stress."""
    rng = np.random.default_rng(seed)
    nN, nE = m.nNode, m.nElement
    st = State.empty(nN, nE)
    st.disp[:] = (rng.normal(0, disp_scale, size=(nN, 3)) if pos is None else pos - m.coordmat).ravel()
    st.disp_pre[:] = st.disp
    s, e, q, y = random_state(rng, nE)
    q[::5] = mesh.STEEL_PLASTIC[1 + (np.arange(len(q[::5])) % 7), 1]
    s[1, 2] = -0.0
    s[2, 0] = 5e-310
    st.integ_stress[:], st.integ_strain[:], st.integ_eq_plastic_strain[:], st.integ_yield_stress[:] = s, e, q, y
    if nE > 2:
        st.element_flag[nE // 2] = 0
    return st


def many_materials(n=11):
    """small_bar with n materials, cycled over the elements (more than the 8 staged in LDS elsewhere)."""
    m = small_bar()
    mats = []
    for i in range(n):
        pl = mesh.STEEL_PLASTIC.copy()
        pl[:, 0] *= 1.0 + 0.03 * i
        mats.append(Material(f"steel{i}", 7.8e-09, 210000. * (1.0 + 0.01 * i), 0.3 - 0.005 * i,
                             pl if i % 4 != 3 else np.zeros((0, 2)), mesh.STEEL_DUCTILE.copy() if i % 4 != 3 else np.zeros((0, 3))))
    return Model(m.coordmat, m.elementmat, 1 + np.arange(m.nElement, dtype=np.int64) % n, mats, bc=m.bc,
                 ic_dofs=m.ic_dofs, ic_values=m.ic_values, d_time=m.d_time, end_time=m.end_time,
                 mass_scaling=m.mass_scaling, name="many_materials")


def header_elements(H, m, st):
    nE, n = m.nElement, m.elementmat - 1
    x = (m.coordmat + st.disp.reshape(-1, 3))[n]
    pe = H.elements(x, m.coordmat[n], st.integ_stress.reshape(nE, 8, 6), st.integ_strain.reshape(nE, 8, 6),
                    st.integ_eq_plastic_strain.reshape(nE, 8), H.mats(list(m.materials)), m.element_material - 1)
    pe[np.asarray(st.element_flag) != 1] = 0.0
    return pe


# ---- 1, 2. per-element bits, set sums ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["small_bar", "many_materials", "inverted"])
def test_per_element_bits_and_set_sums(H, kind):
    pos = None
    if kind == "small_bar":
        m = small_bar()
    elif kind == "many_materials":
        m = many_materials()
    else:
        c = edge_cases.shape_case("inverted")
        m, pos = c["m"], c["pos"]
    nE = m.nElement
    st = crafted_state(m, 21, pos=pos)
    sets = [np.array([1]), np.arange(1, nE + 1, 2), np.zeros(0, np.int64), np.array([nE // 2 + 1])]
    with Solver(m) as sv:
        sv.upload(st)
        p = sv.elem_history_probe(sets, per_elem=True)
        again = sv.elem_history_probe(sets)
    pe = header_elements(H, m, st)
    assert bitwise_equal(p["per_elem"], pe), kind
    rs, flag = restate(m, st)
    assert bitwise_equal(rs, pe)
    assert np.all(p["per_elem"][nE // 2] == 0.0) and np.any(st.integ_stress[8 * (nE // 2)] != 0.0)
    check_record(p["values"], pe, flag, sets, nE)
    assert bitwise_equal(again["values"], p["values"])
    v = p["values"]
    assert v[0, 0] == nE - (1 if nE > 2 else 0) and v[0, 1] == (1 if nE > 2 else 0)
    assert np.all(v[3, :23] == 0.0) and v[3, 23] == np.inf                  # the empty set
    if nE > 2:
        assert v[4, 0] == 0 and v[4, 1] == 1 and v[4, 23] == np.inf          # only the inactive element
    assert v[0, 2] > 0 and v[0, 17] > 0 and v[0, 18] > 0 and v[0, 20] >= 1 and v[0, 22] >= 1


# ---- 3. reduction edges, both launch forms --------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 7), (1, 1, 9), (1, 1, 31), (1, 1, 33), (3, 5, 17), (1, 1, 257),
                                   (1, 3, 683)])
def test_reduction_edges_both_forms(shape):
    """1, 7, 9, 31, 33, 255, 257 and 2049 elements: both sides of a wave's 8 elements, a chunk's 32,
    a group of 8 chunks, which is also the one-block threshold (256 elements), and of 8 groups (nine
    groups: a tree with a childless right branch)."""
    m = small_bar(*shape)
    nE = m.nElement
    assert nE == shape[0] * shape[1] * shape[2]
    st = crafted_state(m, 100 + nE, disp_scale=0.02)
    sets = [np.array([1]), np.arange(1, nE + 1, 2), np.zeros(0, np.int64)]   # element 1 is in two sets
    pe, flag = restate(m, st)
    got, recs = [], []
    for form in (0, 1):
        with tuned(m, {"elem_history_one_block": form}) as sv:
            sv.upload(st)
            p = sv.elem_history_probe(sets, per_elem=True)
            assert bitwise_equal(p["per_elem"], pe)
            check_record(p["values"], pe, flag, sets, nE)
            got.append(p["values"])
            sv.elem_history_enable(sets, stride=1, capacity=4)
            sv.step(1, 3)
            h = sv.elem_history()
            assert list(h["steps"]) == [0, 1, 2]
            check_record(h["values"][0], pe, flag, sets, nE)                 # state 0 is the uploaded state
            recs.append(h["values"])
    assert bitwise_equal(got[0], got[1]) and bitwise_equal(recs[0], recs[1])
    assert bitwise_equal(recs[0][0], got[0])


# ---- 4. in-step records against a one-step-at-a-time run ---------------------------------------------------
def run_b(m, n_steps, tune=None, every=1):
    """Solver B: no history, `every` steps per call; the restatement of its state before each call."""
    out = {}
    with tuned(m, tune) as sv:
        for k in range(0, n_steps, every):
            out[k] = restate(m, sv.download())
            sv.step(k + 1, min(every, n_steps - k))
        final = sv.download()
        dels = sv.deleted()
    return out, final, dels


@pytest.mark.parametrize("exact", [0, 1])
def test_in_step_records_match_restatement(exact):
    m = small_bar()
    nE = m.nElement
    sets = [np.arange(1, 7), np.arange(nE - 5, nE + 1), np.array([17]), np.zeros(0, np.int64)]
    tune = {"elem_exact": exact}
    ref, fb, _ = run_b(m, 60, tune)
    for stride in (1, 7):
        with tuned(m, tune) as sv:
            sv.elem_history_enable(sets, stride=stride, capacity=128)
            sv.step(1, 60)
            h = sv.elem_history()
            assert sv.graph_steps() > 0
            fa = sv.download()
            last = sv.elem_history_probe(sets)
        assert list(h["steps"]) == list(range(0, 60, stride))
        for i, k in enumerate(h["steps"]):
            check_record(h["values"][i], *ref[int(k)], sets, nE)
        same_state(fa, fb)
        check_record(last["values"], *restate(m, fb), sets, nE)
        assert np.any(h["S"][-1, 0] != 0.0) and h["V"][-1, 0] > h["V0"][-1, 0] and h["SE"][-1, 0] > 0


# ---- 5. invariance ---------------------------------------------------------------------------------------
def test_records_and_trajectory_invariant():
    m = fast_deletion_bar(4, 4, 40)
    base = {"elem_pipe_min": 0, "elem_pipe_blocks": 3, "own_assembly": 1, "graph": 16, "fuse_bc": 1, "conn_templates": 1}
    sets = [np.arange(1, 17), np.arange(m.nElement - 15, m.nElement + 1)]
    nsets = [mesh.plane_nodes(4, 4, 0)]

    def run(on=True, **chg):
        with tuned(m, {**base, **chg}) as sv:
            sv.history_enable(nsets, stride=3, capacity=64)
            if on:
                sv.elem_history_enable(sets, stride=3, capacity=64)
            sv.step(1, 100)
            return (sv.elem_history() if on else None), sv.history(), sv.download(), sv.deleted(), sv.graph_steps()

    h0, n0, f0, d0, gs0 = run()
    assert gs0 > 0 and list(h0["steps"]) == list(range(0, 100, 3))
    for chg in ({"graph": 0}, {"own_assembly": 0}, {"conn_templates": 0}, {"fuse_bc": 0}, {"elem_history_one_block": 0},
                {"elem_history_one_block": 1}):
        h, n, f, d, gs = run(**chg)
        assert np.array_equal(h["steps"], h0["steps"]) and bitwise_equal(h["values"], h0["values"]), chg
        assert (gs == 0) == (chg.get("graph") == 0)
    _, n, f, d, _ = run(on=False)                                     # the feature off: the same trajectory
    same_state(f, f0)
    assert np.array_equal(d, d0)
    assert np.array_equal(n["steps"], n0["steps"]) and bitwise_equal(n["values"], n0["values"])


# ---- 6. deletions ---------------------------------------------------------------------------------------
def test_deletion_bar():
    m = fast_deletion_bar()
    nE = m.nElement
    sets = [np.arange(1, nE // 2 + 1), np.arange(nE // 2 + 1, nE + 1)]
    with Solver(m) as sv:
        sv.elem_history_enable(sets, stride=50, capacity=64)
        sv.step(1, 3000)
        h = sv.elem_history()
        dels = sv.deleted()
        last = sv.elem_history_probe(sets)
    ref, fb, db = run_b(m, 3000, every=50)
    assert np.array_equal(dels, db) and len(dels) == 4
    assert list(h["steps"]) == list(range(0, 3000, 50))
    size = np.array([nE, len(sets[0]), len(sets[1])])
    assert np.all(h["N_active"] + h["N_deleted"] == size[None, :]) and last["N_deleted"][0] == 4
    assert np.all(last["N_active"] + last["N_deleted"] == size)
    for i, k in enumerate(h["steps"]):                                  # a deletion of step t is in state t
        assert h["N_deleted"][i, 0] == np.sum(dels[:, 0] <= k)
        check_record(h["values"][i], *ref[int(k)], sets, nE)            # V, S, PD ... exclude the deleted
    check_record(last["values"], *restate(m, fb), sets, nE)
    assert h["N_deleted"][0, 0] == 0 and np.all(np.diff(h["N_deleted"][:, 0]) >= 0)


# ---- 7. ring, restart, refusals, poison --------------------------------------------------------------------
def test_ring_stride_restart_and_reenable():
    m = small_bar()
    sets = [np.arange(1, 7)]
    with Solver(m) as sv:
        sv.elem_history_enable(sets, stride=7, capacity=4)
        assert sv.elem_history_count() == (0, 0)
        sv.step(1, 60)
        assert sv.elem_history_count() == (9, 4)  # states 0, 7, .. 56
        h = sv.elem_history()
        assert list(h["steps"]) == [35, 42, 49, 56]
        one = sv.elem_history(first=6, n=2)
        assert list(one["steps"]) == [42, 49] and bitwise_equal(one["values"], h["values"][1:3])
        for first, n in ((4, 1), (0, 9), (8, 2), (-1, 1)):  # overwritten, or not yet written
            with pytest.raises(hakai.HakaiError) as ei:
                sv.elem_history(first=first, n=n)
            assert ei.value.code == _abi.HAKAI_ERR_ARG
        st = sv.download()                                  # an uploaded state restarts the count
        sv.upload(st)
        assert sv.elem_history_count() == (0, 0)
        sv.step(61, 10)  # states 60 .. 69: one multiple of 7
        h = sv.elem_history()
        assert list(h["steps"]) == [63] and sv.elem_history_count() == (1, 1)
        sv.reset()                                          # a reset does the same
        assert sv.elem_history_count() == (0, 0)
        sv.step(1, 8)
        first_run = sv.elem_history()
        assert list(first_run["steps"]) == [0, 7]
        sv.elem_history_disable()
        with pytest.raises(hakai.HakaiError) as ei:
            sv.elem_history_count()
        assert ei.value.code == _abi.HAKAI_ERR_STATE
        probe = sv.elem_history_probe(sets)                 # the probe works without the in-step history
        sv.step(9, 4)
        sv.reset()
        sv.elem_history_enable(sets, stride=7, capacity=4)
        sv.step(1, 8)
        again = sv.elem_history()
        assert np.array_equal(again["steps"], first_run["steps"]) and bitwise_equal(again["values"], first_run["values"])
        assert probe["values"].shape == (2, 24)


def test_refusals():
    m = small_bar()
    nE = m.nElement
    L = hakai.lib()
    ctx = ctypes.c_void_p()
    _abi.check(L.hakai_create(ctypes.byref(ctx), 0))
    off = np.zeros(1, np.int64)
    rc = L.hakai_elem_history_enable(ctx, 0, _abi.ptr(off, ctypes.c_int64), None, 1, 1)      # no model
    L.hakai_destroy(ctx)
    assert rc == _abi.HAKAI_ERR_STATE
    with Solver(m) as sv:
        sv.comm_init_local(0, 1, 424301)                    # a communicator is no obstacle, no interface needed
        sv.elem_history_enable([np.array([1, 2])], stride=2, capacity=8)
        bad = [dict(sets=[np.array([0])]), dict(sets=[np.array([nE + 1])]), dict(sets=[np.array([3, 3])]),
               dict(sets=[np.array([1])] * 16), dict(sets=[], stride=0), dict(sets=[], capacity=0)]
        for kw in bad:
            with pytest.raises(hakai.HakaiError) as ei:
                sv.elem_history_enable(**kw)
            assert ei.value.code == _abi.HAKAI_ERR_ARG, kw
        for kw in bad[:4]:
            with pytest.raises(hakai.HakaiError) as ei:
                sv.elem_history_probe(kw["sets"])
            assert ei.value.code == _abi.HAKAI_ERR_ARG, kw
        sv.step(1, 6)  # the refused calls changed nothing: two sets, stride 2
        h = sv.elem_history()
        assert list(h["steps"]) == [0, 2, 4] and h["values"].shape == (3, 2, 24)
        sv.elem_history_enable([np.array([1])] * 15)  # 15 sets are allowed
        with pytest.raises(hakai.HakaiError) as ei:
            sv.set_tuning("elem_history_one_block", 2)
        assert ei.value.code == _abi.HAKAI_ERR_ARG


def test_poisoned_step_leaves_no_record():
    """The contact_event_cap recipe of test_gpu_history.test_poisoned_step_leaves_no_record: the
    library handles the overflow and returns an error; the records stop at the last applied step and,
    after raising the cap and stepping on, equal an undisturbed run's bit for bit."""
    m = mesh.two_body_model(plate=(12, 12, 1), impactor=(8, 8, 1), v=-1e5, perturb=0.03, seed=4, n_steps=60)
    n1 = 12 * 12 * 1
    sets = [np.arange(1, n1 + 1), np.arange(n1 + 1, m.nElement + 1)]

    def solver(cap):
        sv = tuned(m, {"elem_pipe_min": 0, "elem_pipe_blocks": 3, "contact_event_cap": cap})
        sv.elem_history_enable(sets, stride=1, capacity=128)
        return sv

    with solver(1 << 12) as sv:
        sv.step(1, m.n_steps)
        full = sv.elem_history()
        final = sv.download()
    assert list(full["steps"]) == list(range(m.n_steps)) and np.any(full["SE"][-1] != 0.0)
    with solver(1) as sv:
        with pytest.raises(hakai.HakaiError) as ei:
            sv.step(1, m.n_steps)
        p = int(re.search(r"step (\d+) was not applied", str(ei.value)).group(1))
        assert 1 < p < m.n_steps
        part = sv.elem_history()
        assert list(part["steps"]) == list(range(p - 1))  # steps 1 .. p-1 ran: states 0 .. p-2
        assert bitwise_equal(part["values"], full["values"][:p - 1])
        sv.set_tuning("contact_event_cap", 1 << 12)
        sv.step(p, m.n_steps - p + 1)
        h = sv.elem_history()
        assert np.array_equal(h["steps"], full["steps"]) and bitwise_equal(h["values"], full["values"])
        same_state(sv.download(), final)


# ---- 8. ranks ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_context_case(which):
    if which == "small_bar":
        m, slab, n_steps, stride = small_bar(), (3, 2), 60, 7
    else:
        m, slab, n_steps, stride = fast_deletion_bar(), (2, 2), 3000, 500
    nE = m.nElement
    gsets = [np.arange(1, nE + 1, 2), np.array([nE]), np.zeros(0, np.int64)]
    with Solver(m) as sv:
        sv.elem_history_enable(gsets, stride=stride, capacity=64)
        sv.step(1, n_steps)
        one = sv.elem_history()
        one_last = sv.elem_history_probe(gsets)
    ref, fb, _ = run_b(m, n_steps, every=stride)
    return m, slab, n_steps, stride, gsets, one, one_last, ref, fb


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("which", ["small_bar", "deletion"])
def test_ranks_combined_record(world, which):
    """The rank states are bit-identical to one context's, so the combined counts, extremes and ids
    equal the one-context record exactly; the combined sums are within (d + R - 1) u sum|term| of the
    restatement; a rank's record is the same bits for both launch forms."""
    m, slab, n_steps, stride, gsets, one, one_last, ref, fb = one_context_case(which)
    nE = m.nElement
    per_form = []
    for form in (0, 1):
        ranks = build_group(m, world, 545000 + 100 * world + 10 * form + (which == "deletion"), slab=slab,
                            tune={"elem_history_one_block": form})
        lsets = []
        for rk in ranks:
            e0, n = rk.loc.global_element_offset, rk.loc.nElement
            lsets.append([s[(s > e0) & (s <= e0 + n)] - e0 for s in gsets])
            rk.sv.elem_history_enable(lsets[-1], stride=stride, capacity=64)
        group_step(ranks, 1, n_steps)
        hs = [rk.sv.elem_history() for rk in ranks]
        comb = elem_history_group([rk.sv for rk in ranks])
        lasts = [rk.sv.elem_history_probe(ls)["values"] for rk, ls in zip(ranks, lsets)]
        close_group(ranks)
        per_form.append((hs, lasts))
        assert np.array_equal(comb["steps"], one["steps"]) and len(comb["steps"]) > 0
        assert bitwise_equal(comb["values"][..., R.EXACT], one["values"][..., R.EXACT])
        for i, k in enumerate(comb["steps"]):
            check_record(comb["values"][i], *ref[int(k)], gsets, nE, extra=world - 1)
        last = elem_history_combine([dict(steps=np.zeros(1, np.int64), values=v[None]) for v in lasts])["values"][0]
        assert bitwise_equal(last[:, R.EXACT], one_last["values"][:, R.EXACT])
        check_record(last, *restate(m, fb), gsets, nE, extra=world - 1)
    (h0, l0), (h1, l1) = per_form
    for a, b in zip(h0, h1):
        assert np.array_equal(a["steps"], b["steps"]) and bitwise_equal(a["values"], b["values"])
    for a, b in zip(l0, l1):
        assert bitwise_equal(a, b)
    if which == "deletion":
        assert one_last["N_deleted"][0] == 4


# ---- 9. driver -----------------------------------------------------------------------------------------
def test_driver_writes_elem_history_csv(tmp_path, monkeypatch):
    from inp_writer import write_inp
    m0 = mesh.two_body_model(plate=(5, 5, 2), impactor=(3, 3, 2), v=-1e5, n_steps=300)
    deck = write_inp(str(tmp_path / "impact.inp"), m0)
    monkeypatch.delenv("HAKAI_ELEM_HISTORY", raising=False)
    monkeypatch.delenv("HAKAI_HISTORY", raising=False)
    hakai.hakai(deck, str(tmp_path / "plain"), verbose=False)
    assert not os.path.exists(tmp_path / "plain" / "elem_history.csv")
    monkeypatch.setenv("HAKAI_ELEM_HISTORY", "10")
    hakai.hakai(deck, str(tmp_path / "hist"), verbose=False)
    files = sorted(os.listdir(tmp_path / "plain"))
    assert len(files) == 101 and sorted(os.listdir(tmp_path / "hist")) == sorted(files + ["elem_history.csv"])
    for f in files:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "hist" / f, "rb").read(), f
    csv = read_elem_history_csv(str(tmp_path / "hist" / "elem_history.csv"))
    m = hakai.read_inp(deck)
    names, esets, dropped = m.elem_history_sets
    assert csv["sets"] == list(names) and names[:3] == ["all", "inst1", "inst2"] and not dropped
    inst = [np.flatnonzero(m.element_instance == i) + 1 for i in (1, 2)]
    assert np.array_equal(esets[0], inst[0]) and np.array_equal(esets[1], inst[1])
    with tuned(m, {"elem_exact": 1}) as sv:  # the driver's element arithmetic
        sv.elem_history_enable(esets, stride=10, capacity=100)
        sv.step(1, m.n_steps)
        h = sv.elem_history()
        last = sv.elem_history_probe(esets)
    assert np.array_equal(csv["steps"], list(h["steps"]) + [m.n_steps]) and len(h["steps"]) == 30
    assert bitwise_equal(csv["values"][:-1], h["values"]) and bitwise_equal(csv["values"][-1], last["values"])
    assert np.any(h["SE"][-1] != 0.0)
    with pytest.raises(Exception) as ei:                    # the N-GPU driver refuses, naming the variable
        from hakai import run as hrun
        hrun.hakai_multi(deck, str(tmp_path / "multi"), local_ranks=1, verbose=False)
    assert "HAKAI_ELEM_HISTORY" in str(ei.value)
