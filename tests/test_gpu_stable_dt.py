"""The stable-time-step diagnostic on the GPU (hakai_stable_dt, csrc/hakai_stable_dt.hip) against its
NumPy restatement (stable_dt_ref), BIT FOR BIT: both minima, both element ids, the three counts and
both per-element arrays. tests/test_stable_dt_cpu.py holds the restatement against the kernel's own
header compiled for the host and pins the formulas against dense eigensolves; here the kernel's
gather, its lane exchanges, the block and grid reductions, the material table, the element offset and
the drivers are under test, and that the call changes nothing a step reads."""
import os

import numpy as np
import pytest

import edge_cases
import hakai
import stable_dt_ref as R
from hakai import mesh
from hakai.model import Model, read_inp
from hakai.solver import Solver, State, read_stable_dt_csv, stable_dt_group
from history_ranks import build_group, close_group, step
from util import bitwise_equal, same_state, small_bar

pytestmark = pytest.mark.gpu


def same(got, ref):
    for k in R.KEYS:
        if k.startswith("dt_"):
            assert bitwise_equal(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k])
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])
    if "dt_est_elem" in got:
        assert bitwise_equal(got["dt_est_elem"], ref["dt_est_elem"])
        assert bitwise_equal(got["dt_safe_elem"], ref["dt_safe_elem"])


def set_state(sv, disp=None, flag=None):
    if disp is None and flag is None:
        return
    d = None if disp is None else np.ascontiguousarray(disp, np.float64)
    f = None if flag is None else np.ascontiguousarray(flag, np.int64)
    sv.upload(State(d, None, None, None, None, None, None, None, None, f, None))


def check(m, disp=None, flag=None, d_time=None, mass_scaling=None):
    """hakai_stable_dt at an uploaded (disp, flag) equals the restatement; returns the reference."""
    ref = R.model(m, disp, flag, d_time, mass_scaling)
    with Solver(m) as sv:
        set_state(sv, disp, flag)
        same(sv.stable_dt(d_time, mass_scaling, per_element=True), ref)
        plain = sv.stable_dt(d_time, mass_scaling)                 # without the per-element outputs
        same(plain, ref)
        assert "dt_est_elem" not in plain
    return ref


def with_material(m, mat):
    return Model(m.coordmat, m.elementmat, m.element_material, [mat], d_time=m.d_time, end_time=m.end_time)


# ---- sizes: every wave and block boundary, flags mixed, displacements uploaded ----------------------

@pytest.mark.parametrize("nE", sorted(edge_cases.SIZES))
def test_sizes(nE):
    c = edge_cases.size_case(nE)
    m = c["m"]
    disp = np.random.default_rng(nE).normal(0, 0.02, size=3 * m.nNode)
    d_time = float(np.median(R.model(m, disp, c["flag"])["dt_safe_elem"][c["flag"] == 1]))
    ref = check(m, disp, c["flag"], d_time=d_time)
    assert ref["n_active"] == int((c["flag"] == 1).sum()) and np.isinf(ref["dt_est_elem"][c["flag"] != 1]).all()
    if nE > 1:
        assert np.isfinite(ref["dt_safe"]) and ref["dt_safe"] > 0


def test_many_blocks():
    """2500 elements: 79 blocks, the last one partly filled, and the finish kernel's tree."""
    coord, elem = mesh.hex_bar(5, 5, 100, perturb=0.1, seed=4)
    m = Model(coord, elem, np.ones(2500, np.int64), [mesh.steel_ductile()])
    rng = np.random.default_rng(9)
    flag = (rng.random(2500) > 0.2).astype(np.int64)
    disp = rng.normal(0, 0.02, size=3 * m.nNode)
    d_time = float(np.quantile(R.model(m, disp, flag)["dt_est_elem"][flag == 1], 0.2))
    ref = check(m, disp, flag, d_time=d_time)
    assert 0 < ref["n_est_below"] < ref["n_active"] < 2500


@pytest.mark.parametrize("shape,where", [((1, 4, 16), 0), ((1, 4, 16), 63), ((1, 5, 14), 69), ((1, 5, 14), 31)])
def test_planted_minimum(shape, where):
    """One element of the mesh made small (its nodes drawn towards its centroid, so its mass shrinks
    with it): element 1, the last element (of a full block, and as the last lane group of a partly
    filled one) and the last lane group of the first block."""
    coord, elem = mesh.hex_bar(*shape)
    n = elem[where] - 1
    coord[n] -= 0.75 * (coord[n] - coord[n].mean(axis=0))
    m = Model(coord, elem, np.ones(len(elem), np.int64), [mesh.steel_elastic()])
    ref = check(m, np.random.default_rng(where).normal(0, 1e-3, size=coord.size))
    assert ref["element_est"] == where + 1 and ref["element_safe"] == where + 1


def test_equal_elements_report_the_lowest_id():
    """40 copies of one cube (own nodes, the same coordinates): every value is equal, so the reported
    element is the lowest active one; and an unperturbed cube mesh against the restatement."""
    c1, e1 = mesh.hex_bar(1, 1, 1)
    coord = np.tile(c1, (40, 1))
    elem = np.concatenate([e1 + 8 * i for i in range(40)])
    m = Model(coord, elem, np.ones(40, np.int64), [mesh.steel_elastic()])
    ref = check(m)
    assert ref["element_est"] == 1 and ref["element_safe"] == 1 and len(set(ref["dt_safe_elem"])) == 1
    flag = np.ones(40, np.int64)
    flag[:33] = 0
    ref = check(m, flag=flag)
    assert ref["element_est"] == 34 and ref["element_safe"] == 34 and ref["n_active"] == 7
    coord, elem = mesh.hex_bar(4, 4, 4)
    check(Model(coord, elem, np.ones(64, np.int64), [mesh.steel_elastic()]))


def test_every_element_deleted():
    m = small_bar(2, 2, 9)
    ref = check(m, flag=np.zeros(m.nElement, np.int64))
    assert ref["dt_est"] == np.inf and ref["dt_safe"] == np.inf and ref["element_est"] == 0
    assert ref["element_safe"] == 0 and ref["n_active"] == 0


def test_eleven_materials():
    """More materials than the element kernel stages in LDS: the table is read from global memory."""
    c = edge_cases.mixed_materials_case()
    m = c["m"]
    assert len(m.materials) == 11 and m.nElement == 33
    ref = check(m, np.random.default_rng(3).normal(0, 0.02, size=3 * m.nNode))
    per_mat = [ref["dt_est_elem"][m.element_material == i + 1].mean() for i in range(11)]
    assert len({round(float(v) * 1e12) for v in per_mat}) > 5          # the materials do differ


def test_mass_scaling():
    m = small_bar(2, 2, 9)
    m.mass_scaling = 100.0
    disp = np.random.default_rng(5).normal(0, 0.02, size=3 * m.nNode)
    ref = check(m, disp)                                                # the model's own factor, rho' = 100 rho
    one = R.model(m, disp, mass_scaling=1.0)
    assert abs(ref["dt_safe"] / one["dt_safe"] - 10.0) < 1e-12 and abs(ref["dt_est"] / one["dt_est"] - 10.0) < 1e-12
    check(m, disp, mass_scaling=1.0)


def graded_bar():
    coord, elem = mesh.hex_bar(2, 2, 16, perturb=0.05, seed=2)
    coord[:, 2] = coord[:, 2] * (0.1 + coord[:, 2] / 16.0)             # layers from 0.1 to 2 thick
    return Model(coord, elem, np.ones(len(elem), np.int64), [mesh.steel_elastic()])


def test_counts_against_d_time():
    m = graded_bar()
    free = R.model(m)
    d_time = float(np.sort(free["dt_est_elem"])[m.nElement // 8])       # one element's own value
    ref = check(m, d_time=d_time)
    assert 0 < ref["n_est_below"] < ref["n_active"] and 0 < ref["n_safe_below"] < ref["n_active"]
    assert ref["n_est_below"] == m.nElement // 8                        # strictly below: not the element itself
    zero = check(m, d_time=0.0)
    assert zero["n_est_below"] == 0 and zero["n_safe_below"] == 0 and zero["n_active"] == m.nElement


def test_degenerate_element_reports_zero():
    """Both node layers of one element moved into the plane z = 0: V = 0 exactly."""
    m = small_bar(2, 2, 9)
    e = 21
    disp = np.random.default_rng(6).normal(0, 0.01, size=(m.nNode, 3))
    n = m.elementmat[e] - 1
    disp[n, 2] = -m.coordmat[n, 2]
    ref = check(m, disp.ravel(), d_time=1e-9)
    assert ref["dt_est"] == 0.0 and ref["dt_safe"] == 0.0 and ref["element_est"] == e + 1
    assert ref["element_safe"] == e + 1 and ref["dt_est_elem"][e] == 0.0 and ref["n_safe_below"] >= 1


# ---- the call changes nothing a step reads ------------------------------------------------------------

@pytest.mark.parametrize("graph", [0, 16])
def test_steps_are_the_same_bits_with_and_without(graph):
    m = small_bar()

    def run(call):
        with Solver(m) as sv:
            sv.set_tuning("graph", graph)
            recs = []
            for i in range(4):
                sv.step(1 + 16 * i, 16)
                if call:
                    recs.append(sv.stable_dt(per_element=True))
            return sv.download(), sv.graph_steps(), recs

    a, ga, recs = run(True)
    b, gb, _ = run(False)
    same_state(a, b)
    assert bitwise_equal(a.velo, b.velo)
    assert ga == gb and (ga > 0) == (graph > 0)
    same(recs[-1], R.model(m, a.disp, a.element_flag))                  # and it saw the stepped state


# ---- ranks -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("world", [2, 3])
def test_group_equals_one_context(world):
    glob = small_bar(2, 2, 12)
    with Solver(glob) as sv:
        sv.step(1, 50)
        one = sv.stable_dt(per_element=True)
        st = sv.download(disp=True, element_flag=True)
    same(one, R.model(glob, st.disp, st.element_flag))
    ranks = build_group(glob, world, key=7100 + world)
    try:
        step(ranks, 1, 50)
        svs = [rk.sv for rk in ranks]
        same(stable_dt_group(svs), {k: one[k] for k in R.KEYS})
        e0 = 0
        for rk in ranks:                                                # every rank reports global ids
            p = rk.sv.stable_dt(per_element=True)
            assert e0 < p["element_safe"] <= e0 + rk.loc.nElement and e0 < p["element_est"] <= e0 + rk.loc.nElement
            assert bitwise_equal(p["dt_safe_elem"], one["dt_safe_elem"][e0:e0 + rk.loc.nElement])
            e0 += rk.loc.nElement
    finally:
        close_group(ranks)


# ---- driver ------------------------------------------------------------------------------------------

def test_driver_writes_stable_dt_csv(tmp_path, monkeypatch):
    from inp_writer import write_inp
    m0 = mesh.two_body_model(plate=(5, 5, 2), impactor=(3, 3, 2), v=-1e5, n_steps=300)
    deck = write_inp(str(tmp_path / "impact.inp"), m0)
    monkeypatch.delenv("HAKAI_DT_CHECK", raising=False)
    hakai.hakai(deck, str(tmp_path / "plain"), verbose=False)
    monkeypatch.setenv("HAKAI_DT_CHECK", "1")
    hakai.hakai(deck, str(tmp_path / "check"), verbose=False)
    monkeypatch.delenv("HAKAI_DT_CHECK")
    files = sorted(os.listdir(tmp_path / "plain"))
    assert len(files) == 101 and sorted(os.listdir(tmp_path / "check")) == files + ["stable_dt.csv"]
    for f in files:
        assert open(tmp_path / "plain" / f, "rb").read() == open(tmp_path / "check" / f, "rb").read(), f
    csv = read_stable_dt_csv(str(tmp_path / "check" / "stable_dt.csv"))
    m = read_inp(deck)
    assert len(csv["records"]) == 101 and list(csv["steps"]) == [3 * i for i in range(101)]
    assert bitwise_equal(csv["d_time"], np.full(101, m.dt))
    with Solver(m) as sv:
        fresh = sv.stable_dt()
    assert csv["records"][0] == fresh
    same(fresh, R.model(m))
    assert all(r["n_active"] == m.nElement for r in csv["records"])
    # the N-rank driver on 2 in-process ranks: the same file (its states are the one-GPU states) and VTKs
    from hakai.run import hakai_multi
    monkeypatch.setenv("HAKAI_DT_CHECK", "1")
    hakai_multi(deck, str(tmp_path / "multi"), local_ranks=2, verbose=False)
    monkeypatch.delenv("HAKAI_DT_CHECK")
    assert sorted(os.listdir(tmp_path / "multi")) == files + ["stable_dt.csv"]
    assert (open(tmp_path / "multi" / "stable_dt.csv", "rb").read() ==
            open(tmp_path / "check" / "stable_dt.csv", "rb").read())
    assert open(tmp_path / "multi" / files[-1], "rb").read() == open(tmp_path / "plain" / files[-1], "rb").read()
