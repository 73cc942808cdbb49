"""Selective mass scaling on the GPU (hakai_mass_scale, csrc/hakai_mass_scale.hip) against its NumPy
restatement (mass_scale_ref), BIT FOR BIT: the elements' added mass, the nodal mass the steps read,
the whole result record, and what hakai_stable_dt reports afterwards. tests/test_mass_scale_cpu.py
holds the restatement against the kernel's own header compiled for the host and pins the guarantee
against dense eigensolves; here the kernels' gather, the lane exchanges, the block and grid
reductions (the fixed tree of mass_added over several finish strides), the node gather, the call
sequence, and that a step really consumes the new mass (against the CPU oracle fed the scaled masses)
are under test."""
import os

import numpy as np
import pytest

import edge_cases
import loads_ref
import mass_scale_ref as MR
import oracle as O
import stable_dt_ref as R
from hakai import _abi, mesh
from hakai.model import Loads, Model
from hakai.solver import Solver, State
from history_ranks import build_group, close_group
from history_ref import HistoryRef, U, balance, prescribed_mask
from util import STATE, bitwise_equal, rel_err, same_state, shuffled, small_bar

pytestmark = pytest.mark.gpu

INF = float("inf")


def same(got, ref):
    for k in MR.KEYS:
        if isinstance(ref[k], float):
            assert bitwise_equal(np.float64(got[k]), np.float64(ref[k])), (k, got[k], ref[k])
        else:
            assert got[k] == ref[k], (k, got[k], ref[k])


def set_state(sv, disp=None, flag=None):
    if disp is None and flag is None:
        return
    d = None if disp is None else np.ascontiguousarray(disp, np.float64)
    f = None if flag is None else np.ascontiguousarray(flag, np.int64)
    sv.upload(State(d, None, None, None, None, None, None, None, None, f, None))


def graded(m, lo=0.15):
    """The model with its z layers graded from lo to 1 of their thickness: dt_safe spreads over the
    elements, so a target inside the spread scales some and leaves the rest."""
    z = m.coordmat[:, 2]
    L = max(float(z.max()), 1.0)
    m.coordmat[:, 2] = z * (lo + (1.0 - lo) * z / L)
    return m


def bar(nx, ny, nz, perturb=0.05, seed=2):
    coord, elem = mesh.hex_bar(nx, ny, nz, perturb=perturb, seed=seed)
    return graded(Model(coord, elem, np.ones(len(elem), np.int64), [mesh.steel_elastic()]))


def check(m, disp=None, flag=None, q=0.5, safety=0.9, max_factor=INF, mass_scaling=None):
    """hakai_mass_scale at an uploaded (disp, flag), with the target at quantile q of the active
    elements' unscaled dt_safe, equals the restatement: record, added mass, nodal mass, and
    hakai_stable_dt afterwards; the same call again changes no bit. Returns the reference."""
    with Solver(m) as sv:
        set_state(sv, disp, flag)
        free = sv.stable_dt(mass_scaling=mass_scaling, per_element=True)
        R_free = R.model(m, disp, flag, mass_scaling=mass_scaling)
        assert bitwise_equal(free["dt_safe_elem"], R_free["dt_safe_elem"])
        live = free["dt_safe_elem"][np.isfinite(free["dt_safe_elem"]) & (free["dt_safe_elem"] > 0)]
        dt = float(np.quantile(live, q)) if len(live) else 1e-7
        kw = dict(dt_target=dt, safety=safety, max_factor=max_factor, mass_scaling=mass_scaling)
        ref = MR.model(m, disp=disp, flag=flag, M0=sv.diag_M[0::3], **kw)
        got = sv.mass_scale(**kw)
        same(got, ref)
        st = sv.mass_scale_state()
        assert bitwise_equal(st["elem_added"], ref["elem_added"])
        assert bitwise_equal(st["diag_M"], ref["diag_M"])
        sd = sv.stable_dt(d_time=dt, mass_scaling=mass_scaling, per_element=True)
        assert bitwise_equal(sd["dt_safe_elem"], ref["dt_safe_elem"]) and bitwise_equal(sd["dt_est_elem"], ref["dt_est_elem"])
        assert bitwise_equal(np.float64(sd["dt_safe"]), np.float64(got["dt_safe"])) and sd["element_safe"] == got["element_safe"]
        keep = ref["elem_added"] == 0.0                                   # unscaled elements keep their earlier bits
        assert bitwise_equal(sd["dt_safe_elem"][keep], free["dt_safe_elem"][keep])
        assert bitwise_equal(sd["dt_est_elem"][keep], free["dt_est_elem"][keep])
        if max_factor == INF and got["n_unfixable"] == 0 and got["n_active"] > 0:
            assert sd["dt_safe"] >= dt and sd["n_safe_below"] == 0
        again = sv.mass_scale(**kw)
        assert again["n_changed"] == 0
        same(again, dict(ref, n_changed=0))
        st2 = sv.mass_scale_state()
        assert bitwise_equal(st2["elem_added"], st["elem_added"]) and bitwise_equal(st2["diag_M"], st["diag_M"])
    return ref


# ---- bit-exact masses ---------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 1, 5), (1, 1, 31), (2, 4, 4), (1, 3, 11)])
def test_element_counts_round_the_block(shape):
    """1, 5, 31, 32 and 33 elements: both sides of the 32-element block."""
    m = bar(*shape)
    ref = check(m, np.random.default_rng(m.nElement).normal(0, 0.01, size=3 * m.nNode))
    assert ref["n_active"] == m.nElement and (m.nElement == 1 or 0 < ref["n_scaled"] < m.nElement)
    assert ref["n_changed"] == ref["n_scaled"] and ref["mass_added"] > 0


def nodes_257():
    """257 is prime, so no box mesh has it: two bodies, 245 + 12 nodes."""
    c1, e1 = mesh.hex_bar(4, 6, 6, perturb=0.05, seed=5)
    c2, e2 = mesh.hex_bar(1, 1, 2, perturb=0.05, seed=6)
    coord = np.concatenate([c1, c2 * np.array([1.0, 1.0, 0.2]) + np.array([10.0, 0.0, 0.0])])
    elem = np.concatenate([e1, e2 + len(c1)])
    return graded(Model(coord, elem, np.ones(len(elem), np.int64), [mesh.steel_elastic()]))


@pytest.mark.parametrize("nN", [255, 256, 257])
def test_node_counts_round_the_block(nN):
    m = {255: lambda: bar(2, 4, 16), 256: lambda: bar(1, 1, 63), 257: nodes_257}[nN]()
    assert m.nNode == nN
    ref = check(m)
    assert 0 < ref["n_scaled"] < m.nElement
    M = ref["diag_M"][0::3]
    assert (M > m.lumped_mass()[0][0::3]).any() and M[-1] > 0


def test_several_finish_strides():
    """8320 elements: 260 blocks, more than the finish kernel's 256 threads, the last stride of the
    tree with a childless branch; every fifth element deleted."""
    m = bar(8, 8, 130)
    assert m.nElement == 8320
    rng = np.random.default_rng(12)
    flag = (rng.random(m.nElement) > 0.2).astype(np.int64)
    ref = check(m, rng.normal(0, 0.01, size=3 * m.nNode), flag, q=0.4)
    assert 0 < ref["n_scaled"] < ref["n_active"] < m.nElement


def test_sixteen_incidences_and_a_node_listed_twice():
    """Every element of a 2 x 2 x 2 block listed twice: the centre node has 16 incidences (the padded
    8-wide incidence table does not exist), and each listing adds its own share."""
    coord, elem = mesh.hex_bar(2, 2, 2, perturb=0.05, seed=8)
    coord[:, 2] *= 0.3
    m = Model(coord, np.concatenate([elem, elem]), np.ones(16, np.int64), [mesh.steel_elastic()])
    ref = check(m, q=1.0)
    assert ref["n_scaled"] >= 15
    assert bitwise_equal(ref["elem_added"][:8], ref["elem_added"][8:])


def test_shuffled_numbering():
    m = shuffled(graded(small_bar(3, 3, 9, material=mesh.steel_elastic())), 5)
    ref = check(m, np.random.default_rng(2).normal(0, 0.01, size=3 * m.nNode))
    assert 0 < ref["n_scaled"] < m.nElement


def test_deleted_elements_are_untouched_and_keep_their_mass():
    m = bar(2, 2, 12)
    flag = np.ones(m.nElement, np.int64)
    flag[::3] = 0
    ref = check(m, flag=flag, q=0.7)
    assert not ref["elem_added"][::3].any() and ref["n_active"] == int(flag.sum())
    with Solver(m) as sv:                                                # scaled first, deleted later: the mass stays
        first = sv.mass_scale(dt_target=2.0 * sv.stable_dt()["dt_safe"])
        a = sv.mass_scale_state()
        set_state(sv, flag=flag)
        ref2 = MR.model(m, dt_target=first["dt_safe"] * 4.0, flag=flag, prev=a["elem_added"], M0=sv.diag_M[0::3])
        got = sv.mass_scale(dt_target=first["dt_safe"] * 4.0)
        same(got, ref2)
        b = sv.mass_scale_state()
        assert bitwise_equal(b["elem_added"], ref2["elem_added"]) and bitwise_equal(b["diag_M"], ref2["diag_M"])
        assert bitwise_equal(b["elem_added"][::3], a["elem_added"][::3]) and a["elem_added"][::3].any()
        assert got["n_scaled"] >= int((a["elem_added"] > 0).sum())    # deleted elements with mass still count


def test_eleven_materials():
    c = edge_cases.mixed_materials_case()
    m = c["m"]
    assert len(m.materials) == 11
    ref = check(m, np.random.default_rng(3).normal(0, 0.02, size=3 * m.nNode))
    assert 0 < ref["n_scaled"] < m.nElement


@pytest.mark.parametrize("safety,max_factor,ms", [(1.0 - 2.0 ** -40, INF, None), (0.9, 1.25, None), (1.0, 1.0, None),
                                                   (0.9, INF, 100.0)])
def test_parameters_on_a_displaced_state(safety, max_factor, ms):
    m = bar(3, 3, 7)
    disp = np.random.default_rng(7).normal(0, 0.03, size=3 * m.nNode)
    ref = check(m, disp, q=0.6, safety=safety, max_factor=max_factor, mass_scaling=ms)
    if max_factor == 1.0:
        assert ref["n_capped"] > 0 and ref["n_scaled"] == 0 and ref["mass_added"] == 0.0 and ref["max_factor_reached"] == 1.0
    elif max_factor < INF:
        assert ref["n_capped"] > 0 and ref["max_factor_reached"] <= max_factor * (1 + 4 * U)
    else:
        assert ref["n_capped"] == 0 and ref["max_factor_reached"] > 1.0


def test_unfixable_elements():
    """One element flattened into a plane (V == 0): unfixable, reported, dt_safe 0 after the call."""
    m = bar(2, 2, 9)
    e = 13
    disp = np.random.default_rng(6).normal(0, 0.005, size=(m.nNode, 3))
    n = m.elementmat[e] - 1
    disp[n, 2] = -m.coordmat[n, 2]
    ref = check(m, disp.ravel(), q=0.5)
    assert ref["n_unfixable"] >= 1 and ref["status"][e] == MR.UNFIXABLE and ref["elem_added"][e] == 0.0
    assert ref["dt_safe"] == 0.0 and ref["element_safe"] == e + 1


# ---- no-op ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("graph", [0, 16])
def test_target_below_every_element_is_a_no_op(graph):
    m = small_bar()

    def run(call):
        with Solver(m) as sv:
            sv.set_tuning("graph", graph)
            sv.step(1, 32)
            if call:
                before = sv.mass_scale_state()["diag_M"]
                r = sv.mass_scale(dt_target=0.5 * sv.stable_dt()["dt_safe"])
                assert r["n_changed"] == 0 and r["n_scaled"] == 0 and r["mass_added"] == 0.0
                after = sv.mass_scale_state()
                assert bitwise_equal(after["diag_M"], before) and bitwise_equal(before, sv.diag_M)
                assert not after["elem_added"].any()
            sv.step(33, 200)
            return sv.download(), sv.graph_steps()

    a, ga = run(True)
    b, gb = run(False)
    same_state(a, b)
    assert bitwise_equal(a.velo, b.velo) and ga == gb and (ga > 0) == (graph > 0)


# ---- the step really consumes the new mass ------------------------------------------------------------------

def thin_layer_bar(cut=0.75):
    """A bar whose element layer 3 keeps 1 - cut of its thickness. At a quarter the deck's step is
    above the critical step (the unscaled run overflows within 20 steps); at 0.6 it is above every
    element's dt_safe but still below the critical step, for the runs that scale mid-way."""
    m = small_bar(2, 2, 8, material=mesh.steel_elastic(), v_end=1e4, n_steps=50)
    z = m.coordmat[:, 2]
    m.coordmat[:, 2] = np.where(z > 3.5, z - cut, z)
    return m


def assert_state(g, s):
    for k in STATE:
        assert bitwise_equal(getattr(g, k), s[k]), f"{k}: max rel diff {rel_err(getattr(g, k), s[k]):.3e}"


@pytest.mark.parametrize("mid", [0, 20])
def test_steps_read_the_scaled_mass_bit_for_bit(mid):
    """elem_exact on a bar with a thin layer, the target the deck's step: 50 steps from state 0, and
    with the call after 20 steps, equal the CPU oracle's run with the scaled masses written into its
    diag_M, bit for bit, in stream and in graph mode."""
    m = thin_layer_bar(0.75 if mid == 0 else 0.4)
    out = {}
    for graph in (0, 16):
        orc = O.Oracle(m)
        with Solver(m) as sv:
            sv.set_tuning("elem_exact", 1)
            sv.set_tuning("graph", graph)
            assert sv.stable_dt()["dt_safe"] < m.dt                      # the deck's step is above the bound
            if mid:
                sv.step(1, mid)
                orc.run(1, mid)
                assert_state(sv.download(), orc.s)
            r = sv.mass_scale()
            st = sv.mass_scale_state()
            ref = MR.model(m, disp=orc.s["disp"], M0=sv.diag_M[0::3])
            same(r, ref)
            assert bitwise_equal(st["diag_M"], ref["diag_M"]) and 0 < r["n_scaled"] and r["dt_safe"] >= m.dt
            assert (st["diag_M"] > orc.diag_M).any()
            orc.diag_M[:] = st["diag_M"]
            sv.step(mid + 1, 50 - mid)
            orc.run(mid + 1, 50 - mid)
            g = sv.download()
            assert_state(g, orc.s)
            assert np.all(np.isfinite(g.disp)) and np.all(np.isfinite(g.Q))
            out[graph] = (g, sv.graph_steps())
    same_state(out[0][0], out[16][0])
    assert out[0][1] == 0 and out[16][1] > 0
    plain = O.Oracle(m)
    plain.run(1, 50)
    assert not bitwise_equal(plain.s["disp"], out[0][0].disp)             # and the mass did matter


# ---- call sequence ----------------------------------------------------------------------------------------

def test_call_sequence_grow_clear_upload():
    m = bar(2, 3, 10)
    with Solver(m) as sv:
        M0 = sv.mass_scale_state()["diag_M"]
        assert bitwise_equal(M0, sv.diag_M)
        dt = 1.5 * sv.stable_dt()["dt_safe"]
        a = sv.mass_scale(dt_target=dt)
        sa = sv.mass_scale_state()
        assert a["n_changed"] > 0
        disp = np.random.default_rng(4).normal(0, 0.03, size=3 * m.nNode)   # a call after deformation only grows
        set_state(sv, disp)
        b = sv.mass_scale(dt_target=dt)
        sb = sv.mass_scale_state()
        ref = MR.model(m, dt_target=dt, disp=disp, prev=sa["elem_added"], M0=M0[0::3])
        same(b, ref)
        assert bitwise_equal(sb["elem_added"], ref["elem_added"]) and bitwise_equal(sb["diag_M"], ref["diag_M"])
        assert np.all(sb["elem_added"] >= sa["elem_added"]) and np.all(sb["diag_M"] >= sa["diag_M"]) and b["n_changed"] > 0
        sv.reset()                                                        # reset_state keeps the scaling
        assert bitwise_equal(sv.mass_scale_state()["diag_M"], sb["diag_M"])
        for bad in (dict(safety=0.0), dict(safety=1.5), dict(safety=float("nan")), dict(dt_target=0.0),
                    dict(dt_target=-1.0), dict(dt_target=INF), dict(max_factor=0.5), dict(max_factor=float("nan")),
                    dict(mass_scaling=0.0), dict(mass_scaling=INF)):
            with pytest.raises(_abi.HakaiError) as ei:
                sv.mass_scale(**bad)
            assert ei.value.code == _abi.HAKAI_ERR_ARG, bad
        sc = sv.mass_scale_state()                                        # refused: the scaling stays in force
        assert bitwise_equal(sc["elem_added"], sb["elem_added"]) and bitwise_equal(sc["diag_M"], sb["diag_M"])
        sv.clear_mass_scale()
        cleared = sv.mass_scale_state()
        assert bitwise_equal(cleared["diag_M"], M0) and not cleared["elem_added"].any()
        free = sv.stable_dt(per_element=True)
        assert bitwise_equal(free["dt_safe_elem"], R.model(m)["dt_safe_elem"])
        sv.mass_scale(dt_target=dt)                                       # upload_model clears
        mats, keep = m.c_materials()
        _abi.check(sv.L.hakai_upload_model(sv.ctx, m.nNode, _abi.ptr(m.coordmat), m.nElement,
                                           _abi.ptr(m.elementmat, _abi.c_int64), _abi.ptr(m.element_material, _abi.c_int64),
                                           len(m.materials), mats, _abi.ptr(sv.diag_M)))
        again = sv.mass_scale_state()
        assert bitwise_equal(again["diag_M"], M0) and not again["elem_added"].any()


# ---- interactions -------------------------------------------------------------------------------------------

def test_history_restarts_and_its_identity_holds():
    m = thin_layer_bar(0.4)
    sets = [mesh.plane_nodes(2, 2, 8)]
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", 1)
        sv.history_enable(sets)
        sv.step(1, 20)
        assert sv.history_count() == (20, 20)
        r = sv.mass_scale()
        assert r["n_changed"] > 0 and sv.history_count() == (0, 0)        # restarted
        diag = sv.mass_scale_state()["diag_M"]
        sv.step(21, 40)
        h = sv.history()
        assert sv.history_count() == (40, 40) and sv.mass_scale(dt_target=1e-12)["n_changed"] == 0
        assert sv.history_count() == (40, 40)                            # a call that changes nothing keeps the records
        final = sv.download()
    # the restatement on a second solver stepped one step at a time, with the scaled masses
    recs = []
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", 1)
        sv.step(1, 20)
        sv.mass_scale()
        ref = HistoryRef(diag, prescribed_mask(m), sets, m.dt)
        st = sv.download(disp=True, disp_pre=True, Q=True)
        seed = ref.seed(st.disp, st.disp_pre)
        for t in range(21, 61):
            sv.step(t, 1)
            nx = sv.download(disp=True, disp_pre=True, Q=True)
            recs.append(ref.step(nx.disp, st.disp, st.Q, None))
            st = nx
        same_state(final, sv.download())
    vals = np.array([v for v, _ in recs])
    mags = np.array([g for _, g in recs])
    assert np.all(np.abs(h["ke_seed"] - seed[0]) <= 48 * U * seed[1])
    plain = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 13, 14, 15]
    assert np.all(np.abs(h["values"][:, :, plain] - vals[:, :, plain]) <= 48 * U * mags[:, :, plain])
    # set 0's balance KE - KE_seed + W_int - W_ext - W_bc against the run's largest energy term: no
    # worse than 64 x the exactly rounded restatement's own residual (the existing history tests' factor)
    dev = [balance(v[0], h["ke_seed"][0]) for v in h["values"]]
    own = [balance(v[0], seed[0][0]) for v in vals]
    worst = max(abs(x) for x, _ in dev) / max(big for _, big in dev)
    floor = max(abs(x) for x, _ in own) / max(big for _, big in own)
    print(f"history after mass scaling: balance residual {worst:.3e} of the largest term, restatement {floor:.3e}")
    assert worst <= 64 * max(floor, U)


def test_gravity_weighs_the_added_mass():
    m = thin_layer_bar()
    g = [0.0, 0.0, -9.81e3]
    with Solver(m) as sv:
        sv.set_loads(Loads(grav_accel=[g]))
        f0 = sv.load_force(1)
        sv.mass_scale()
        diag = sv.mass_scale_state()["diag_M"]
        f1 = sv.load_force(1)
        st = sv.download(disp=True, element_flag=True)
    assert bitwise_equal(f1[2::3], diag[2::3] * g[2]) and (np.abs(f1) > np.abs(f0)).any()
    assert bitwise_equal(f1, loads_ref.load_force(m, Loads(grav_accel=[g]), diag, st.disp, st.element_flag, m.dt))


# ---- refusals -----------------------------------------------------------------------------------------------

def test_ranks_are_refused():
    glob = small_bar(2, 2, 12)
    ranks = build_group(glob, 2, key=7300)
    try:
        for rk in ranks:
            before = rk.sv.mass_scale_state()["diag_M"]
            with pytest.raises(_abi.HakaiError) as ei:
                rk.sv.mass_scale()
            assert ei.value.code == _abi.HAKAI_ERR_STATE
            assert bitwise_equal(rk.sv.mass_scale_state()["diag_M"], before)
    finally:
        close_group(ranks)


# ---- drivers ------------------------------------------------------------------------------------------------

def test_drivers_apply_the_keyword_and_write_mass_scale_csv(tmp_path):
    import hakai
    from hakai.solver import read_mass_scale_csv
    from loads_cases import write_loads_deck
    m0 = thin_layer_bar()
    m0.end_time = 300 * m0.d_time
    deck = write_loads_deck(str(tmp_path / "thin.inp"), m0,
                            step="*Variable Mass Scaling, safety=0.8, max factor=50, repeat=output\n")
    plain = write_loads_deck(str(tmp_path / "plain.inp"), m0)
    _abi.check(hakai.lib().hakai_run_inp(deck.encode(), str(tmp_path / "c").encode(), 0, 0))
    hakai.hakai(deck, str(tmp_path / "py"), verbose=False)
    hakai.hakai(plain, str(tmp_path / "plain"), verbose=False)
    files = sorted(f for f in os.listdir(tmp_path / "c") if f.endswith(".vtk"))
    assert len(files) == 101 and sorted(os.listdir(tmp_path / "py")) == files + ["mass_scale.csv"]
    assert sorted(os.listdir(tmp_path / "plain")) == files                 # no keyword: no csv, the run as before
    for f in files + ["mass_scale.csv"]:
        assert open(tmp_path / "c" / f, "rb").read() == open(tmp_path / "py" / f, "rb").read(), f
    assert open(tmp_path / "c" / files[-1], "rb").read() != open(tmp_path / "plain" / files[-1], "rb").read()
    rows = read_mass_scale_csv(str(tmp_path / "c" / "mass_scale.csv"))
    assert [r["step"] for r in rows] == [3 * i for i in range(100)]        # every output state but the last
    m = hakai.read_inp(deck)
    assert m.variable_mass_scaling == dict(dt=None, safety=0.8, max_factor=50.0, repeat=True)
    kw = dict(safety=0.8, max_factor=50.0)
    with Solver(m) as sv:                                                 # the API's doubles, at state 0 and after 3 steps
        sv.set_tuning("elem_exact", 1)
        for i in range(3):
            r = sv.mass_scale(**kw)
            assert {k: rows[i][k] for k in r} == r and rows[i]["dt_target"] == m.dt, i
            sv.step(1 + 3 * i, 3)
    assert rows[0]["n_changed"] > 0 and rows[0]["dt_safe"] >= m.dt and all(r["n_active"] == m.nElement for r in rows)
    from hakai import run
    with pytest.raises(ValueError, match="Variable Mass Scaling"):
        run.hakai_multi(deck, out_dir=str(tmp_path / "multi"), local_ranks=2, verbose=False)
