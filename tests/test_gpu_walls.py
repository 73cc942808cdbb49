"""Rigid walls (hakai_set_walls) on the GPU: the probe hakai_wall_force against tests/walls_ref.py bit for
bit (sizes around a wave and a block, one, three and 32 walls, node lists, special values, amplitude
breakpoints); one step from a known state equals tests/nodal_ref.py's update fed with the restated
total contact + loads + walls, bit for bit; graph against stream mode and the persistence rules; the
history records and the set-0 energy identity with a stationary and a moving wall; two in-process
ranks against one context; the argument errors; the driver."""
import ctypes

import numpy as np
import pytest

import hakai
import history_ranks as HR
import loads_ref as LR
import nodal_ref
import walls_ref as R
from edge_cases import SIZES
from hakai import _abi, mesh
from hakai.model import Loads, Model, Walls
from hakai.solver import Solver, read_history_csv
from history_ref import HistoryRef, balance, prescribed_mask
from loads_cases import nset, write_loads_deck
from test_gpu_loads import AMPS, BLOCKS, DT, PROBE_T, all_kinds, bar, contact_deck, only, tk
from util import bitwise_equal, same_state, small_bar
from walls_cases import corner_walls, many_walls, one_wall, random_state, rigid_wall

pytestmark = pytest.mark.gpu


def check_probe(sv, m, w, disp, pre, times=(1, 2, 7)):
    for t in times:
        got = sv.wall_force(t, DT)
        ref = R.wall_force(m, w, sv.diag_M, disp, pre, t, DT)
        assert bitwise_equal(got, ref), (t, float(np.max(np.abs(got - ref))))
    return ref


def plain(m, **kw):
    """The model without its loads and walls (or with the ones given)."""
    return Model(m.coordmat, m.elementmat, m.element_material, m.materials, m.bc, m.ic_dofs, m.ic_values, m.d_time,
                 m.end_time, m.mass_scaling, m.contact_flag, m.element_instance, contact_params=m.contact_params,
                 contact_pairs=m.contact_pairs, **kw)


# ---- 1. the probe ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", [SIZES[k] for k in sorted(SIZES)] + [BLOCKS[k] for k in sorted(BLOCKS)],
                         ids=[f"E{k}" for k in sorted(SIZES)] + [f"N{k}" for k in sorted(BLOCKS)])
def test_wall_force_sizes(shape):
    """One wall (all nodes, then a node list), three oblique walls in a corner, 32 walls with every
    mask bit and the all-nodes path, at a random state with about half the nodes through a wall."""
    m = bar(*shape)
    disp, pre = random_state(m, 200 + sum(shape), dt=DT)
    rng = np.random.default_rng(sum(shape))
    some = np.sort(rng.choice(m.nNode, max(1, m.nNode // 2), replace=False)) + 1
    with Solver(m) as sv:
        assert np.all(sv.wall_force(3, DT) == 0.0)               # no wall yet
        sv.upload(only(disp=disp, disp_pre=pre))
        w1 = one_wall(m)
        sv.set_walls(w1)
        f1 = check_probe(sv, m, w1, disp, pre)
        hit = np.any(f1.reshape(-1, 3) != 0.0, axis=1)
        assert hit.any() and (m.nNode < 16 or 0.25 < hit.mean() < 0.75)
        wl = one_wall(m, nodes=[some])
        sv.set_walls(wl)
        fl = check_probe(sv, m, wl, disp, pre).reshape(-1, 3)
        listed = np.zeros(m.nNode, bool)
        listed[some - 1] = True
        assert np.all(fl[~listed] == 0.0) and bitwise_equal(fl[listed], f1.reshape(-1, 3)[listed])
        w3 = corner_walls(m)
        sv.set_walls(w3)
        f3 = check_probe(sv, m, w3, disp, pre)
        if m.nNode >= 64:                                        # the order of the sum matters somewhere
            assert not bitwise_equal(f3, R.wall_force(m, w3, sv.diag_M, disp, pre, 7, DT, reverse=True))
        w32 = many_walls(m, 5 + sum(shape), amps=AMPS)
        sv.set_walls(w32)
        check_probe(sv, m, w32, disp, pre, times=(1, 2, 7, 12))
        mk = R.masks(m.nNode, w32)
        assert mk is not None and np.all(mk >> np.uint32(31)) and np.all(mk & np.uint32(1))
        if m.nNode >= 200:
            assert np.bitwise_or.reduce(mk) == 0xffffffff and len(set(mk.tolist())) > 32
        assert np.all(sv.load_force(3, DT) == 0.0)               # the loads' probe stays the loads'
    assert all((a + 1) * (b + 1) * (c + 1) == k for k, (a, b, c) in BLOCKS.items())


def test_special_values():
    """Nodes exactly on a plane get nothing; -0.0 displacements; disp == disp_pre (no slip: no NaN)."""
    m = bar(2, 2, 3, perturb=0.0)
    nN = m.nNode
    w = Walls(origin=[[0, 0, 1.0], [1.0, 0, 0]], normal=[[0, 0, 4.0], [0.5, 0, 0]], stiffness=[1024.0, 512.0],
              damping=[0.25, 0.0], friction=[0.5, 0.5])
    zero = np.zeros(3 * nN)
    with Solver(m) as sv:
        sv.set_walls(w)
        sv.upload(only(disp=zero, disp_pre=zero))
        f = check_probe(sv, m, w, zero, zero).reshape(-1, 3)
        on = (m.coordmat[:, 2] == 1.0) & (m.coordmat[:, 0] >= 1.0)
        assert on.sum() == 6 and np.all(f[on] == 0.0)           # on the plane (and beyond the other wall): nothing
        below = m.coordmat[:, 2] < 1.0
        assert np.all(f[below, 2] > 0.0) and not np.any(np.isnan(f))
        assert np.all(f[below & (m.coordmat[:, 0] >= 1.0), :2] == 0.0)   # no slip: purely normal
        neg = -zero
        sv.upload(only(disp=neg, disp_pre=zero))
        check_probe(sv, m, w, neg, zero)
        disp, _ = random_state(m, 4)
        sv.upload(only(disp=disp, disp_pre=disp))
        f = check_probe(sv, m, w, disp, disp)
        assert not np.any(np.isnan(f)) and np.any(f != 0.0)


def test_amplitude_breakpoints_and_moving_walls():
    """Every table (and the constant) moving a wall, at steps before, on and after the breakpoints;
    t = 1 included, where taum < 0 takes the first segment's extrapolation."""
    m = bar(1, 3, 3)
    tabs = list(range(-1, len(AMPS)))
    n = len(tabs)
    c = m.coordmat.mean(axis=0)
    rng = np.random.default_rng(6)
    w = Walls(origin=np.tile(c, (n, 1)), normal=rng.normal(0, 1, (n, 3)), motion=rng.normal(0, 0.2, (n, 3)), amp=tabs,
              stiffness=np.full(n, 1e4), damping=np.full(n, 0.2), friction=np.full(n, 0.3), amps=AMPS)
    disp, pre = random_state(m, 9, dt=DT)
    with Solver(m) as sv:
        sv.set_walls(w)
        sv.upload(only(disp=disp, disp_pre=pre))
        check_probe(sv, m, w, disp, pre, times=PROBE_T)
    o1, v1 = R.wall_frame(w, 1, 1, DT)                           # the ramp at t = 1: at rest position, moving
    assert np.all(o1 == c) and np.any(v1 != 0.0)
    f = [R.wall_force(m, w, np.ones(3 * m.nNode), disp, pre, t, DT) for t in (5, 6, 7, 8)]
    assert all(not bitwise_equal(f[i], f[i + 1]) for i in range(3))


# ---- 2. one step ------------------------------------------------------------------------------------------------

def skin_walls(m, **kw):
    """Two walls that shave the body: a slowly moving one 0.12 under its top (all nodes) and a side wall
    0.1 inside its low-x face on a node list that includes the first nodes (a clamped plane where
    the model has one). Shallow penetrations: the model can be stepped."""
    lo, hi = m.coordmat.min(axis=0), m.coordmat.max(axis=0)
    args = dict(origin=[[lo[0], lo[1], hi[2] - 0.12], [lo[0] + 0.1, lo[1], lo[2]]],
                normal=[[0.02, 0.01, -1.0], [1.0, 0.05, 0.02]], motion=[[0, 0.01, -0.02], [0, 0, 0]], amp=[1, -1],
                stiffness=[2e4, 0.0], scale=[0.125, 0.25], damping=[0.2, 0.1], friction=[0.3, 0.2],
                nodes=[[], list(range(1, m.nNode // 2 + 2))], amps=AMPS)
    args.update(kw)
    return Walls(**args)


def wall_bar():
    """A clamped plastic bar between two walls, no loads."""
    m = small_bar(2, 2, 4, material=mesh.steel_ductile(), perturb=0.05)
    return plain(m, walls=skin_walls(m))


def everything_deck():
    m = contact_deck()                                           # contact and loads (tests/test_gpu_loads.py)
    m.walls = skin_walls(m)
    return m


@pytest.mark.parametrize("fuse_bc", [1, 0])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("deck", ["wall", "everything"])
def test_one_step_equals_nodal_reference(deck, exact, fuse_bc):
    """disp after one hakai_step == nodal_ref's update of the downloaded disp, disp_pre and Q with
    f = contact (hakai_contact_force) + loads + walls, added in the stated order; then the BCs.
    Steps 1 (from the reset state) and 4, 5 (a natural Q, both parities)."""
    m = wall_bar() if deck == "wall" else everything_deck()
    full = deck == "everything"
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", exact)
        sv.set_tuning("fuse_bc", fuse_bc)
        any_contact = False
        for t in (1, 2, 3, 4, 5):
            st = sv.download(disp=True, disp_pre=True, Q=True, element_flag=True)
            fc = sv.contact_force(t) if full else None
            any_contact |= full and bool(np.any(fc != 0.0))
            f0 = LR.load_force(m, m.loads, sv.diag_M, st.disp, st.element_flag, float(t) * m.dt, fc) if full else None
            f = R.wall_force(m, m.walls, sv.diag_M, st.disp, st.disp_pre, t, m.dt, f=f0)
            fw = R.wall_force(m, m.walls, sv.diag_M, st.disp, st.disp_pre, t, m.dt)
            assert bitwise_equal(sv.wall_force(t), fw) and np.any(fw != 0.0)
            if full:                                             # the other probes keep their meaning
                assert bitwise_equal(sv.load_force(t), LR.load_force(m, m.loads, sv.diag_M, st.disp, st.element_flag,
                                                                     float(t) * m.dt))
                assert bitwise_equal(sv.contact_force(t), fc)
            else:
                assert np.all(sv.load_force(t) == 0.0)
            sv.step(t, 1)
            ref = nodal_ref.nodal_step(sv.diag_M, m.dt, st.disp, st.disp_pre, st.Q, f)
            nodal_ref.apply_bc(m, float(t) * m.dt, ref)
            got = sv.download(disp=True).disp
            assert bitwise_equal(got, ref), (t, float(np.max(np.abs(got - ref))))
            nowall = nodal_ref.nodal_step(sv.diag_M, m.dt, st.disp, st.disp_pre, st.Q, f0 if full else f * 0.0)
            assert not bitwise_equal(got, nodal_ref.apply_bc(m, float(t) * m.dt, nowall))   # the wall acts
        assert any_contact == full
        assert np.all(got[prescribed_mask(m)] == 0.0)


# ---- 3. launch forms and persistence ------------------------------------------------------------------------------

def test_graph_against_stream_mode():
    m = wall_bar()
    out = []
    for graph in (16, 0):
        with Solver(m) as sv:
            sv.set_tuning("graph", graph)
            sv.step(1, 40)
            out.append((sv.download(), sv.graph_steps()))
    same_state(out[0][0], out[1][0])
    assert out[0][1] > 0 and out[1][1] == 0
    with Solver(plain(m)) as sv:
        sv.step(1, 40)
        assert not bitwise_equal(sv.download(disp=True).disp, out[0][0].disp)


def test_set_walls_mid_run_drops_the_graphs():
    m = wall_bar()
    w2 = skin_walls(m, damping=[0.0, 0.3], friction=[0.1, 0.4], amp=[3, 0])
    out = []
    for graph in (16, 0):
        with Solver(m) as sv:
            sv.set_tuning("graph", graph)
            sv.step(1, 40)
            g0 = sv.graph_steps()
            sv.set_walls(w2)
            sv.step(41, 40)
            out.append((sv.download(), g0, sv.graph_steps()))
    same_state(out[0][0], out[1][0])
    assert out[0][1] > 0 and out[0][2] > out[0][1] and out[1][2] == 0


def test_clear_walls_equals_never_walled_and_persistence():
    m = wall_bar()
    with Solver(plain(m)) as sv:
        assert np.all(sv.wall_force(3) == 0.0)
        sv.step(1, 40)
        ref = sv.download()
    with Solver(m) as sv:
        assert np.any(sv.wall_force(3) != 0.0)
        sv.clear_walls()
        assert np.all(sv.wall_force(3) == 0.0)
        sv.step(1, 40)
        same_state(sv.download(), ref)
        assert sv.graph_steps() > 0
    with Solver(m) as sv:                                        # walls survive set_bc, reset and upload
        f3 = sv.wall_force(3)
        bc, keep = m.c_bc()
        _abi.check(sv.L.hakai_set_bc(sv.ctx, ctypes.byref(bc)))
        sv.reset()
        sv.upload(only(disp=np.zeros(3 * m.nNode), disp_pre=np.zeros(3 * m.nNode)))
        zero = R.wall_force(m, m.walls, sv.diag_M, np.zeros(3 * m.nNode), np.zeros(3 * m.nNode), 3, m.dt)
        assert bitwise_equal(sv.wall_force(3), zero) and np.any(zero != 0.0)
        sv.reset()
        assert bitwise_equal(sv.wall_force(3), f3)


def test_loads_and_walls_are_independent():
    m = wall_bar()
    ld = all_kinds(m, 31)
    both = plain(m, walls=m.walls, loads=ld)
    with Solver(both) as sv:
        fw, fl = sv.wall_force(3), sv.load_force(3)
        assert np.any(fw != 0.0) and np.any(fl != 0.0)
        sv.step(1, 24)
        ref = sv.download()
    with Solver(m) as sv:                                        # walls first, loads set later
        sv.set_loads(ld)
        assert bitwise_equal(sv.wall_force(3), fw) and bitwise_equal(sv.load_force(3), fl)
        sv.step(1, 24)
        same_state(sv.download(), ref)
    with Solver(both) as sv:
        sv.set_walls(m.walls)                                    # setting the walls leaves the loads
        assert bitwise_equal(sv.load_force(3), fl)
        sv.clear_loads()
        assert bitwise_equal(sv.wall_force(3), fw) and np.all(sv.load_force(3) == 0.0)
        sv.step(1, 24)
        only_walls = sv.download()
    with Solver(m) as sv:
        sv.step(1, 24)
        same_state(sv.download(), only_walls)
    with Solver(both) as sv:
        sv.clear_walls()
        assert bitwise_equal(sv.load_force(3), fl) and np.all(sv.wall_force(3) == 0.0)
        sv.step(1, 24)
        only_loads = sv.download()
    with Solver(plain(m, loads=ld)) as sv:
        sv.step(1, 24)
        same_state(sv.download(), only_loads)


# ---- 4. history ----------------------------------------------------------------------------------------------------

def impact_bar():
    """A free elastoplastic bar flying at 1e5 mm/s into a stationary floor just below it."""
    b = mesh.bar_model(2, 2, 6, mesh.steel_ductile(), -1e5, perturb=0.02, seed=3, n_steps=400)
    m = Model(b.coordmat, b.elementmat, b.element_material, b.materials, [], b.ic_dofs, b.ic_values, b.d_time, b.end_time)
    m.walls = Walls(origin=[[0, 0, -0.05]], normal=[[0, 0, 1]], scale=[0.5], damping=[0.1], friction=[0.3])
    return m


def crushed_bar(n):
    """A clamped elastoplastic bar at rest, crushed from its free end by a platen that ramps down."""
    m = small_bar(2, 2, 6, v_end=0.0, material=mesh.steel_ductile())
    m.walls = Walls(origin=[[0, 0, 6.0 + 0.03]], normal=[[0, 0, -1]], motion=[[0.05, 0, -1.0]], amp=[0],
                    scale=[0.5], damping=[0.1], friction=[0.3], amps=[(tk(0, n), [0.0, 0.6])])
    return m


@pytest.mark.parametrize("case", ["stationary", "moving"])
def test_history_identity_and_wall_force(case):
    """The records equal the restated force's sums within tests/test_gpu_history.py's record bounds, and
    the set-0 residual KE - KE_seed + W_int - W_ext - W_bc stays within the bound
    tests/test_gpu_loads.py uses for the same identity (64 x 1.3e-14 of the largest energy term)."""
    n = 120
    m = impact_bar() if case == "stationary" else crushed_bar(n)
    with Solver(m) as sv:
        sv.history_enable([], stride=1, capacity=256)
        sv.set_walls(m.walls)                                    # restarts the history
        assert sv.history_count() == (0, 0)
        sv.step(1, n)
        h = sv.history()
        final = sv.download()
        assert sv.graph_steps() > 0
    recs, mags = [], []
    with Solver(m) as sv:
        ref = HistoryRef(sv.diag_M, prescribed_mask(m), [], m.dt)
        st = sv.download(disp=True, disp_pre=True, Q=True)
        seed = ref.seed(st.disp, st.disp_pre)
        for t in range(1, n + 1):
            f = R.wall_force(m, m.walls, sv.diag_M, st.disp, st.disp_pre, t, m.dt)
            sv.step(t, 1)
            nx = sv.download(disp=True, disp_pre=True, Q=True)
            v, g = ref.step(nx.disp, st.disp, st.Q, f)
            recs.append(v)
            mags.append(g)
            st = nx
        same_state(sv.download(), final)
    from test_gpu_history import check_records
    check_records(h, np.array(recs), np.array(mags), seed)
    assert np.any(h["F_ext"][:, 0, 2] != 0.0)
    res = [balance(v[0], h["ke_seed"][0]) for v in h["values"]]
    worst = max(abs(r) for r, _ in res) / max(big for _, big in res)
    print(f"{case} wall: worst balance residual {worst:.3e} of the largest energy term")
    assert worst <= 64 * 1.3e-14
    assert np.any(final.integ_eq_plastic_strain > 0.0)          # the bar did yield
    if case == "moving":
        assert h["W_ext"][-1, 0] != 0.0                          # the platen does work


# ---- 5. two ranks -------------------------------------------------------------------------------------------------------

def test_two_ranks_side_wall_bitexact():
    """A bar cut in two z-slabs meets side walls (normals +x and -x) with friction and damping, so the
    interface nodes touch them: every rank's state is bit-identical to one context after 20 steps."""
    glob = small_bar(3, 2, 8, material=mesh.steel_ductile())
    mid = mesh.plane_nodes(3, 2, 4)                              # the cut of two z-slabs
    right = np.where(glob.coordmat[:, 0] > 2.5)[0] + 1
    args = dict(origin=[[0.06, 0, 0], [2.94, 0, 0]], normal=[[1, 0, 0], [-2, 0, 0]], motion=[[0.02, 0, 0], [0, 0, 0]],
                amp=[1, -1], scale=[0.25, 0.125], stiffness=[0.0, 5e3], damping=[0.2, 0.1], friction=[0.3, 0.2], amps=AMPS)
    gw = Walls(nodes=[[], right], **args)
    with Solver(glob) as sv:
        sv.set_walls(gw)
        f = sv.wall_force(1).reshape(-1, 3)
        assert np.any(f[mid - 1, 0] != 0.0) and np.any(f[mid - 1, 2] != 0.0)   # an interface node is on a wall and rubs
        sv.step(1, 20)
        one = sv.download()
    ranks = HR.build_group(glob, 2, 9292, slab=(3, 2))
    try:
        shared = 0
        for rk in ranks:
            loc = {int(gid): l + 1 for l, gid in enumerate(rk.l2g)}   # global 1-based -> local 1-based
            mine = [loc[int(g)] for g in right if int(g) in loc]
            shared += sum(1 for g in right if int(g) in loc and g in mid)
            rk.sv.set_walls(Walls(nodes=[[], mine], **args))
        assert shared == 2 * len(set(right) & set(mid)) > 0      # both ranks listed the interface nodes
        HR.step(ranks, 1, 20)
        for rk in ranks:
            st = rk.sv.download(disp=True, disp_pre=True)
            g = rk.l2g - 1
            assert bitwise_equal(st.disp.reshape(-1, 3), one.disp.reshape(-1, 3)[g])
            assert bitwise_equal(st.disp_pre.reshape(-1, 3), one.disp_pre.reshape(-1, 3)[g])
    finally:
        HR.close_group(ranks)
    with Solver(glob) as sv:
        sv.step(1, 20)
        assert not bitwise_equal(sv.download(disp=True).disp, one.disp)


# ---- 6. refusals ------------------------------------------------------------------------------------------------------------

def bad_walls():
    base = dict(origin=[[0, 0, 0]], normal=[[0, 0, 1]])
    B = {"too_many": dict(origin=np.zeros((33, 3)), normal=np.tile([0.0, 0, 1], (33, 1))),
         "node_zero": dict(base, nodes=[[0]]), "node_high": dict(base, nodes=[[10 ** 6]]),
         "normal_zero": dict(base, normal=[[0, 0, 0]]), "normal_nan": dict(base, normal=[[np.nan, 0, 1]]),
         "normal_inf": dict(base, normal=[[0, np.inf, 1]]),
         "amp": dict(base, amp=[len(AMPS)]), "amp_low": dict(base, amp=[-2]),
         "table": dict(base, amp=[0], amps=[([0.0], [1.0])])}
    for name in ("stiffness", "scale", "damping", "friction"):
        B[name + "_negative"] = dict(base, **{name: [-1.0]})
        B[name + "_nan"] = dict(base, **{name: [np.nan]})
        B[name + "_inf"] = dict(base, **{name: [np.inf]})
    return B


def test_argument_errors_leave_the_walls_in_force():
    m = wall_bar()
    with Solver(m) as sv:
        f3 = sv.wall_force(3)
        for name, kw in bad_walls().items():
            d = dict(amps=AMPS)
            d.update(kw)
            with pytest.raises(hakai.HakaiError) as ei:
                sv.set_walls(Walls(**d))
            assert ei.value.code == _abi.HAKAI_ERR_ARG, name
            assert bitwise_equal(sv.wall_force(3), f3), name
        s, keep = m.walls.c()
        s.n_wall = -1
        assert sv.L.hakai_set_walls(sv.ctx, ctypes.byref(s)) == _abi.HAKAI_ERR_ARG
        assert bitwise_equal(sv.wall_force(3), f3)
        sv.step(1, 10)
        a = sv.download()
    with Solver(m) as sv:
        sv.step(1, 10)
        same_state(sv.download(), a)
    ctx = ctypes.c_void_p()                                      # before upload_model: HAKAI_ERR_STATE
    L = hakai.lib()
    _abi.check(L.hakai_create(ctypes.byref(ctx), 0))
    try:
        s, keep = m.walls.c()
        assert L.hakai_set_walls(ctx, ctypes.byref(s)) == _abi.HAKAI_ERR_STATE
        assert L.hakai_clear_walls(ctx) == _abi.HAKAI_ERR_STATE
    finally:
        L.hakai_destroy(ctx)


# ---- 7. the driver --------------------------------------------------------------------------------------------------------------

def test_driver_applies_the_decks_walls(tmp_path, monkeypatch):
    """hakai(fname) on a deck with *Rigid Wall and *Dload gravity: its history.csv (every step, full
    doubles) and last VTK equal the Solver run of the same mesh with Walls and Loads given directly."""
    b = mesh.bar_model(2, 2, 4, mesh.steel_ductile(), -5e4, perturb=0.02, n_steps=200)
    base = Model(b.coordmat, b.elementmat, b.element_material, b.materials, [], b.ic_dofs, b.ic_values, b.d_time, b.end_time)
    top = mesh.plane_nodes(2, 2, 4)
    path = write_loads_deck(
        str(tmp_path / "deck.inp"), base, assembly=nset("TOP", top),
        amplitudes="*Amplitude, name=PUSH\n" + ", ".join(repr(x) for x in (0.0, 0.0, 200 * DT, 1.0)) + "\n",
        step="*Dload\n, GRAV, 9.81e6, 0., 0., -1.\n**\n"
             + rigid_wall("FLOOR", (0, 0, -0.02), (0, 0, 3), damping=0.1, friction=0.3)
             + rigid_wall("PLATEN", (0, 0, 4.1), (0, 0, -1), (0, 0.01, -0.4), nset="TOP", amplitude="PUSH",
                          stiffness=1e4, scale=0.25) + "**\n")
    m = hakai.read_inp(path)
    assert m.walls.n_wall == 2 and m.walls.nodes[1].tolist() == top.tolist() and len(m.loads.grav_accel) == 1
    direct = Walls(origin=[[0, 0, -0.02], [0, 0, 4.1]], normal=[[0, 0, 3], [0, 0, -1]], motion=[[0, 0, 0], [0, 0.01, -0.4]],
                   amp=[-1, 0], stiffness=[0.0, 1e4], scale=[0.5, 0.25], damping=[0.1, 0.0], friction=[0.3, 0.0],
                   nodes=[[], top], amps=[([0.0, 200 * DT], [0.0, 1.0])])
    monkeypatch.setenv("HAKAI_HISTORY", "1")
    out = tmp_path / "out"
    hakai.hakai(path, str(out), verbose=False)
    csv = read_history_csv(str(out / "history.csv"))
    mm = plain(m, loads=Loads(grav_accel=[[0.0, 0.0, -9.81e6]]), walls=direct)
    with Solver(mm) as sv:
        sv.set_tuning("elem_exact", 1)                           # the driver's element arithmetic
        sv.history_enable(m.history_sets[1], capacity=m.n_steps + 1)
        sv.step(1, m.n_steps)
        h = sv.history()
        disp = sv.download(disp=True).disp.reshape(-1, 3)
    assert bitwise_equal(csv["values"], h["values"]) and np.array_equal(csv["steps"], h["steps"])
    txt = open(out / "file100.vtk").read().split("\n")
    i = txt.index("VECTORS DISPLACEMENT float")
    got = np.array([[float(x) for x in l.split()] for l in txt[i + 1:i + 1 + m.nNode]])
    assert np.allclose(got, disp, rtol=2e-6, atol=1e-12) and np.abs(disp).max() > 0
    with Solver(plain(m, loads=mm.loads)) as sv:                 # without the walls the bar falls through
        sv.set_tuning("elem_exact", 1)
        sv.step(1, m.n_steps)
        assert not bitwise_equal(sv.download(disp=True).disp.reshape(-1, 3), disp)
