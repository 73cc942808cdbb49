"""External loads on the GPU (hakai_set_loads, csrc/hakai_loads.hip) against their NumPy restatement
(loads_ref, held against exact rationals and against the kernel's own header by
tests/test_loads_cpu.py). Through the probe hakai_load_force the comparison is bit for bit; one step
from a known state equals tests/nodal_ref.py's update fed with the restated force, bit for bit; whole
runs are compared between launch forms, contexts and ranks bit for bit.

Times: every table is given in units of the step, t_j = j * dt formed in Python as the library forms
t * d_time, so 'on a breakpoint' is exact."""
import ctypes
import math
from fractions import Fraction

import numpy as np
import pytest

import hakai
import history_ranks as HR
import loads_ref as R
import nodal_ref
from contact_cases import mixed_two_body
from edge_cases import SIZES
from hakai import _abi, mesh
from hakai.model import Loads, Model
from hakai.solver import Solver, State, read_history_csv
from history_ref import HistoryRef, balance, prescribed_mask
from loads_cases import amplitude, bar_end_elements, elset, write_loads_deck
from util import bitwise_equal, same_state, small_bar

pytestmark = pytest.mark.gpu

DT = 1e-7


def tk(*ks):
    return [float(k) * DT for k in ks]


AMPS = [(tk(0, 10), [0.0, 1.0]),                              # 0 ramp
        (tk(0, 4, 9, 20), [0.0, 1.0, 0.25, 2.0]),             # 1 multi-point
        (tk(0, 6, 6, 20), [0.0, 0.0, 1.0, 1.0]),              # 2 stepped
        (tk(0, 12, 5, 30), [1.0, -1.0, 3.0, 0.5]),            # 3 non-monotonic times
        (tk(3, 8, 16), [0.5, 1.5, -0.5])]                     # 4 starts late: extrapolated before it
PROBE_T = [1, 3, 4, 5, 6, 7, 8, 9, 10, 12, 16, 20, 25, 30, 31, 100]  # before, on and after the breakpoints


def bar(nx, ny, nz, material=None, perturb=0.05, bc=True, seed=3):
    m = small_bar(nx, ny, nz, material=material or mesh.steel_elastic(), perturb=perturb, seed=seed)
    if not bc:
        m = Model(m.coordmat, m.elementmat, m.element_material, m.materials, d_time=m.d_time, end_time=m.end_time)
    return m


def exterior_faces(m):
    seen = {}
    for e in range(m.nElement):
        for k in range(6):
            key = tuple(sorted(m.elementmat[e][list(R.FACE_NODES[k])]))
            seen.setdefault(key, []).append((e + 1, k + 1))
    return [v[0] for v in seen.values() if len(v) == 1]


def all_kinds(m, seed, amps=True, interior=True):
    """Concentrated entries (several on one dof), two gravity entries and pressure on every exterior
    face plus a few interior ones and one face twice, amplitudes mixed with the constant."""
    rng = np.random.default_rng(seed)
    pick = (lambda n: rng.integers(-1, len(AMPS), n)) if amps else (lambda n: np.full(n, -1))
    ext = exterior_faces(m)
    pe, pf = [e for e, _ in ext], [k for _, k in ext]
    if interior:
        extra = rng.integers(1, m.nElement + 1, 6)
        pe += list(extra) + [pe[0]]
        pf += list(rng.integers(1, 7, 6)) + [pf[0]]
    n_cl = min(3 * m.nNode, 20)
    dof = rng.integers(1, 3 * m.nNode + 1, n_cl)
    dof[:3] = dof[0]
    return Loads(amps=AMPS if amps else [], cload_dof=dof, cload_value=rng.normal(0, 50, n_cl), cload_amp=pick(n_cl),
                 grav_accel=[[0.0, 0.0, -9.81e3], [120.0, -40.0, 0.0]], grav_amp=pick(2),
                 press_elem=pe, press_face=pf, press_value=rng.normal(0, 200, len(pe)), press_amp=pick(len(pe)))


def only(**kw):
    """A State that uploads just the given arrays."""
    d = dict(disp=None, disp_pre=None, velo=None, Q=None, integ_stress=None, integ_strain=None,
             integ_yield_stress=None, integ_eq_plastic_strain=None, integ_triax_stress=None, element_flag=None, Qe=None)
    d.update(kw)
    return State(**d)


def check_probe(sv, m, ld, disp, flag, times=PROBE_T):
    for t in times:
        got = sv.load_force(t, DT)
        ref = R.load_force(m, ld, sv.diag_M, disp, flag, float(t) * DT)
        assert bitwise_equal(got, ref), (t, float(np.max(np.abs(got - ref))))


# ---- 1. the probe: sizes, geometry, deleted elements ---------------------------------------------------

BLOCKS = {255: (2, 4, 16), 256: (3, 3, 15), 258: (1, 2, 42)}   # nodes around one 256-thread block (257 is prime)


@pytest.mark.parametrize("shape", [SIZES[k] for k in sorted(SIZES)] + [BLOCKS[k] for k in sorted(BLOCKS)],
                         ids=[f"E{k}" for k in sorted(SIZES)] + [f"N{k}" for k in sorted(BLOCKS)])
def test_load_force_sizes(shape):
    m = bar(*shape)
    rng = np.random.default_rng(sum(shape))
    ld = all_kinds(m, 100 + sum(shape))
    disp = rng.normal(0, 0.03, 3 * m.nNode)                  # the load follows the current configuration
    flag = (rng.random(m.nElement) < 0.7).astype(np.int64)   # a deleted element's face contributes nothing
    if m.nElement == 1:
        flag[:] = 1
    with Solver(m) as sv:
        sv.set_loads(ld)
        check_probe(sv, m, ld, np.zeros(3 * m.nNode), np.ones(m.nElement, np.int64), times=[1, 7])
        sv.upload(only(disp=disp, element_flag=flag))
        check_probe(sv, m, ld, disp, flag)
        if not flag.all():
            on = R.load_force(m, ld, sv.diag_M, disp, np.ones(m.nElement, np.int64), 7 * DT)
            assert not bitwise_equal(on, sv.load_force(7, DT))   # the deleted faces did carry load
    assert all((a + 1) * (b + 1) * (c + 1) == k for k, (a, b, c) in BLOCKS.items())


def test_faces_per_node_and_special_values():
    """Nodes with 1, 2, 3 and 4 loaded faces; then every face of every element (the centre node of the
    2x2x2 bar gathers 24) with one face twice; -0.0 and zero pressures; a collapsed face."""
    m = bar(2, 2, 2, perturb=0.0)
    top = bar_end_elements(2, 2, 2)
    ld1 = Loads(press_elem=list(top) + [top[0]], press_face=[2] * 4 + [3], press_value=[10.0, -20.0, 30.0, 5.0, 7.0])
    counts = np.diff(R.plan(m, ld1)[4])
    assert {0, 1, 2, 3, 4} <= set(counts)
    pe = np.repeat(np.arange(1, 9), 6)
    pf = np.tile(np.arange(1, 7), 8)
    pv = np.random.default_rng(5).normal(0, 10, 48)
    pv[3], pv[4], pv[10] = -0.0, 0.0, -0.0
    ld2 = Loads(press_elem=list(pe) + [1], press_face=list(pf) + [1], press_value=list(pv) + [2.5])
    assert np.diff(R.plan(m, ld2)[4]).max() >= 9
    # node 1 moved onto node 2: faces with a collapsed edge; node 1, 2, 4, 5 onto one point: a zero-area S1
    disp = np.zeros((m.nNode, 3))
    for n in (1, 4, 5):
        disp[n - 1] = m.coordmat[1] - m.coordmat[n - 1]
    disp = disp.ravel()
    ones = np.ones(8, np.int64)
    with Solver(m) as sv:
        for ld in (ld1, ld2):
            sv.set_loads(ld)
            sv.upload(only(disp=np.zeros(3 * m.nNode)))
            check_probe(sv, m, ld, np.zeros(3 * m.nNode), ones, times=[1])
            sv.upload(only(disp=disp))
            check_probe(sv, m, ld, disp, ones, times=[1])
        z = Loads(press_elem=[1], press_face=[1], press_value=[-0.0], cload_dof=[1, 1], cload_value=[-0.0, -0.0])
        sv.set_loads(z)
        f = sv.load_force(1, DT)
        assert bitwise_equal(f, R.load_force(m, z, sv.diag_M, disp, ones, DT))
    x = (m.coordmat + disp.reshape(-1, 3))[m.elementmat[0][list(R.FACE_NODES[0])] - 1]
    assert np.all(x == x[0]) and np.all(R.face_corners(x, 3.0) == 0.0)


@pytest.mark.parametrize("kind", ["cload", "gravity", "pressure"])
def test_amplitudes_every_kind(kind):
    """Each load kind on each table (and the constant), at times before, on and after the breakpoints."""
    m = bar(1, 3, 3)
    tabs = list(range(-1, len(AMPS)))
    n = len(tabs)
    if kind == "cload":
        ld = Loads(amps=AMPS, cload_dof=np.arange(1, n + 1) * 4, cload_value=np.linspace(3.0, 9.0, n), cload_amp=tabs)
    elif kind == "gravity":
        ld = Loads(amps=AMPS, grav_accel=np.random.default_rng(1).normal(0, 1e3, (n, 3)), grav_amp=tabs)
    else:
        ext = exterior_faces(m)[:n]
        ld = Loads(amps=AMPS, press_elem=[e for e, _ in ext], press_face=[k for _, k in ext],
                   press_value=np.linspace(-50.0, 70.0, n), press_amp=tabs)
    disp = np.random.default_rng(2).normal(0, 0.02, 3 * m.nNode)
    with Solver(m) as sv:
        sv.set_loads(ld)
        sv.upload(only(disp=disp))
        check_probe(sv, m, ld, disp, np.ones(m.nElement, np.int64))
    for a, (t, v) in enumerate(AMPS):                          # the times do sit on the breakpoints
        assert all(any(float(p) * DT == x for p in PROBE_T) for x in t if x > 0), a


# ---- 2. one step ------------------------------------------------------------------------------------------

def bc_bar():
    """A clamped bar whose clamped plane also carries loads (the BC wins), plastic material."""
    m = small_bar(2, 2, 4, material=mesh.steel_ductile(), perturb=0.05)
    ld = all_kinds(m, 77)
    ld.cload_dof[5:8] = [1, 2, 6]                                # dofs of the clamped plane z = 0
    return Model(m.coordmat, m.elementmat, m.element_material, m.materials, m.bc, m.ic_dofs, m.ic_values, m.d_time,
                 m.end_time, loads=ld)


def contact_deck():
    m = mixed_two_body()
    rng = np.random.default_rng(8)
    ext = exterior_faces(m)[::3]
    # loads on the impactor's nodes that are in contact and on the plate, the clamped plane included
    m.loads = Loads(amps=AMPS, cload_dof=rng.integers(1, 3 * m.nNode + 1, 30), cload_value=rng.normal(0, 5, 30),
                    cload_amp=rng.integers(-1, len(AMPS), 30), grav_accel=[[0.0, 0.0, -9.81e3]], grav_amp=[1],
                    press_elem=[e for e, _ in ext], press_face=[k for _, k in ext],
                    press_value=rng.normal(0, 20, len(ext)), press_amp=rng.integers(-1, len(AMPS), len(ext)))
    m.loads.cload_dof[:2] = [1, 3]                               # node 1 is on the plate's clamped plane
    return m


@pytest.mark.parametrize("fuse_bc", [1, 0])
@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("deck", ["bar", "contact"])
def test_one_step_equals_nodal_reference(deck, exact, fuse_bc):
    """disp after one hakai_step == nodal_ref's update of the downloaded disp, disp_pre and Q with
    f = the restated total: hakai_contact_force (contact deck) plus the loads, added in the stated
    order; then the BCs. Steps 1 (from the reset state) and 4, 5 (a natural Q, both parities)."""
    m = bc_bar() if deck == "bar" else contact_deck()
    contact = deck == "contact"
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", exact)
        sv.set_tuning("fuse_bc", fuse_bc)
        any_contact = False
        for t in (1, 2, 3, 4, 5):
            st = sv.download(disp=True, disp_pre=True, Q=True, element_flag=True)
            fc = sv.contact_force(t) if contact else None
            any_contact |= contact and bool(np.any(fc != 0.0))
            f = R.load_force(m, m.loads, sv.diag_M, st.disp, st.element_flag, float(t) * m.dt, fc)
            assert bitwise_equal(sv.load_force(t), R.load_force(m, m.loads, sv.diag_M, st.disp, st.element_flag,
                                                                float(t) * m.dt))
            if contact:
                assert bitwise_equal(sv.contact_force(t), fc)      # contact only, as before
            sv.step(t, 1)
            ref = nodal_ref.nodal_step(sv.diag_M, m.dt, st.disp, st.disp_pre, st.Q, f)
            nodal_ref.apply_bc(m, float(t) * m.dt, ref)
            got = sv.download(disp=True).disp
            assert bitwise_equal(got, ref), (t, float(np.max(np.abs(got - ref))))
            free = nodal_ref.nodal_step(sv.diag_M, m.dt, st.disp, st.disp_pre, st.Q, f * 0.0)
            assert not bitwise_equal(got, nodal_ref.apply_bc(m, float(t) * m.dt, free))   # the loads act
        assert any_contact == contact
        pres = prescribed_mask(m)
        assert np.any(pres[m.loads.cload_dof - 1])                 # a prescribed dof carries a load
        assert np.all(got[pres] == 0.0)


# ---- 3. launch forms ------------------------------------------------------------------------------------------

def test_graph_against_stream_mode():
    m = bc_bar()
    out = []
    for graph in (16, 0):
        with Solver(m) as sv:
            sv.set_tuning("graph", graph)
            sv.step(1, 40)
            out.append((sv.download(), sv.graph_steps()))
    same_state(out[0][0], out[1][0])
    assert out[0][1] > 0 and out[1][1] == 0
    with Solver(Model(m.coordmat, m.elementmat, m.element_material, m.materials, m.bc, m.ic_dofs, m.ic_values,
                      m.d_time, m.end_time)) as sv:
        sv.step(1, 40)
        assert not bitwise_equal(sv.download(disp=True).disp, out[0][0].disp)


def test_set_loads_mid_run_drops_the_graphs():
    m = bc_bar()
    ld2 = all_kinds(m, 78)
    out = []
    for graph in (16, 0):
        with Solver(m) as sv:
            sv.set_tuning("graph", graph)
            sv.step(1, 40)
            g0 = sv.graph_steps()
            sv.set_loads(ld2)
            sv.step(41, 40)
            out.append((sv.download(), g0, sv.graph_steps()))
    same_state(out[0][0], out[1][0])
    assert out[0][1] > 0 and out[0][2] > out[0][1] and out[1][2] == 0


def test_clear_loads_equals_never_loaded():
    m = bc_bar()
    plain = Model(m.coordmat, m.elementmat, m.element_material, m.materials, m.bc, m.ic_dofs, m.ic_values, m.d_time,
                  m.end_time)
    with Solver(plain) as sv:
        assert np.all(sv.load_force(3) == 0.0)
        sv.step(1, 40)
        ref = sv.download()
    with Solver(m) as sv:
        assert np.any(sv.load_force(3) != 0.0)
        sv.clear_loads()
        assert np.all(sv.load_force(3) == 0.0)
        sv.step(1, 40)
        same_state(sv.download(), ref)
        assert sv.graph_steps() > 0
    with Solver(m) as sv:                                        # loads survive set_bc, reset and upload
        f3 = sv.load_force(3)
        bc, keep = m.c_bc()
        _abi.check(sv.L.hakai_set_bc(sv.ctx, ctypes.byref(bc)))
        sv.reset()
        sv.upload(only(disp=np.zeros(3 * m.nNode)))
        assert bitwise_equal(sv.load_force(3), f3)


# ---- 4. history ------------------------------------------------------------------------------------------------

def test_history_identity_and_external_force():
    """Gravity and pressure on a small elastoplastic bar: the set-0 residual KE - KE_seed + W_int -
    W_ext - W_bc stays within the bound tests/test_gpu_history.py uses for the same identity, and
    F_ext / W_ext are the restated force's sums within that file's record bounds (48 u sum|term|)."""
    m = small_bar(2, 2, 6, material=mesh.steel_ductile())
    top = bar_end_elements(2, 2, 6)
    n = 120
    ld = Loads(amps=[(tk(0, 60, n), [0.0, 1.0, 0.5]), (tk(0, 30, n), [1.0, -1.0, 1.0])],
               grav_accel=[[0.0, 3e8, -9.81e8]], grav_amp=[1], press_elem=top, press_face=[2] * 4,
               press_value=[-1500.0] * 4, press_amp=[0] * 4)
    with Solver(m) as sv:
        sv.history_enable([], stride=1, capacity=256)
        sv.set_loads(ld)                                         # restarts the history
        assert sv.history_count() == (0, 0)
        sv.step(1, n)
        h = sv.history()
        final = sv.download()
        assert sv.graph_steps() > 0
    recs, mags = [], []
    with Solver(m) as sv:
        sv.set_loads(ld)
        ref = HistoryRef(sv.diag_M, prescribed_mask(m), [], m.dt)
        st = sv.download(disp=True, disp_pre=True, Q=True, element_flag=True)
        seed = ref.seed(st.disp, st.disp_pre)
        for t in range(1, n + 1):
            f = R.load_force(m, ld, sv.diag_M, st.disp, st.element_flag, float(t) * m.dt)
            sv.step(t, 1)
            nx = sv.download(disp=True, disp_pre=True, Q=True, element_flag=True)
            v, g = ref.step(nx.disp, st.disp, st.Q, f)
            recs.append(v)
            mags.append(g)
            st = nx
        same_state(sv.download(), final)
    from test_gpu_history import check_records
    check_records(h, np.array(recs), np.array(mags), seed)
    assert np.all(h["F_ext"][5:, 0, 2] != 0.0) and h["W_ext"][-1, 0] != 0.0
    res = [balance(v[0], h["ke_seed"][0]) for v in h["values"]]
    worst = max(abs(r) for r, _ in res) / max(big for _, big in res)
    print(f"loaded bar: worst balance residual {worst:.3e} of the largest energy term")
    assert worst <= 64 * 1.3e-14
    assert np.any(final.integ_eq_plastic_strain > 0.0)          # the bar did yield


def test_free_fall():
    """An unconstrained bar at rest under constant gravity g, n steps.

    The computed trajectory satisfies, per dof and step, m (du_{k+1} - du_k) / dt^2 = f - Q_k +
    m d_k / dt^2, with d_k the nodal update's rounding error, |d_k| <= 8 u S_k (nodal_ref: 8 roundings,
    S_k = |f - Q| / A + 2 |u_k| + |u_{k-1}|). Summed over the nodes the internal forces cancel (to a
    rounding OF rounding-sized forces: second order), so with M = sum m and u_k = g dt^2 k (k + 1) / 2:
      P_n = sum m du_n / dt = M g n dt  +  [f = fl(m g): u M g n dt]  +  sum_k sum m d_k / dt,
      S_k <= g dt^2 (1 + 3 k (k + 1) / 2),   sum_{k<n} S_k <= g dt^2 (n + (n - 1) n (n + 1) / 2),
    so the nodal updates move P_n by at most 8 u M g dt (n + (n-1) n (n+1) / 2), relative to M g n dt:
    8 + 4 (n^2 - 1). The history sum itself is within 48 u (tests/test_gpu_history.py). Relative bound
    u (1 + 8 + 4 (n^2 - 1) + 48), doubled for the second-order terms.
    The mass-weighted mean displacement after n steps is g dt^2 n (n + 1) / 2: its error is the double
    sum of the same d_k, at most n * 8 u g dt^2 (n + (n-1) n (n+1) / 2), relative to the parabola
    8 (2 + n (n - 1)); plus f's rounding and the two roundings of forming the mean from an exact sum:
    u (8 (2 + n (n - 1)) + 3), doubled."""
    m = bar(2, 2, 3, bc=False)
    g = np.array([0.0, 0.0, -9.81e3])
    n = 40
    with Solver(m) as sv:
        sv.set_loads(Loads(grav_accel=[g]))
        sv.history_enable([])
        sv.step(1, n)
        h = sv.history()
        disp = sv.download(disp=True).disp.reshape(-1, 3)
        mass = sv.diag_M[0::3]
    M = sum(Fraction(float(x)) for x in mass)
    u = Fraction(1, 2 ** 53)
    dt = Fraction(float(m.dt))
    want_p = M * Fraction(float(g[2])) * n * dt
    bound_p = 2 * u * (57 + 4 * (n * n - 1)) * abs(want_p)
    assert h["steps"][-1] == n - 1
    err = abs(Fraction(float(h["P"][-1, 0, 2])) - want_p)
    print(f"free fall: momentum error {float(err / abs(want_p)):.3e} relative, bound {float(bound_p / abs(want_p)):.3e}")
    assert err <= bound_p
    mean = float(sum(Fraction(float(a)) * Fraction(float(b)) for a, b in zip(mass, disp[:, 2])) / M)
    want_u = Fraction(float(g[2])) * dt * dt * n * (n + 1) / 2
    bound_u = 2 * u * (8 * (2 + n * (n - 1)) + 3) * abs(want_u)
    print(f"free fall: mean displacement error {abs(float(Fraction(mean) - want_u) / float(want_u)):.3e} relative")
    assert abs(Fraction(mean) - want_u) <= bound_u
    assert math.isclose(h["F_ext"][-1, 0, 2], float(M) * g[2], rel_tol=1e-12)


# ---- 5. two ranks --------------------------------------------------------------------------------------------------

def test_two_ranks_cload_and_gravity_bitexact():
    """Concentrated loads on an interface node and gravity with a time-varying amplitude on two
    in-process ranks: bit-identical to one context after 20 steps. Pressure on a rank is refused."""
    glob = small_bar(3, 2, 8, material=mesh.steel_ductile())
    mid = mesh.plane_nodes(3, 2, 4)                              # the cut of two z-slabs
    cl_nodes = np.array([mid[0], mid[5], mid[5], 3, glob.nNode])
    cl_comp = np.array([0, 2, 2, 1, 2])
    cl_val, cl_amp = np.array([50.0, -80.0, 12.5, 30.0, -60.0]), np.array([-1, 1, 0, 2, 3])
    grav, gamp = [[0.0, 2e5, -9.81e5], [1e5, 0.0, 0.0]], [1, -1]
    gl = Loads(amps=AMPS, cload_dof=3 * (cl_nodes - 1) + cl_comp + 1, cload_value=cl_val, cload_amp=cl_amp,
               grav_accel=grav, grav_amp=gamp)
    with Solver(glob) as sv:
        sv.set_loads(gl)
        sv.step(1, 20)
        one = sv.download()
    ranks = HR.build_group(glob, 2, 9191, slab=(3, 2))
    try:
        shared = 0
        for rk in ranks:
            loc = {int(gid): l for l, gid in enumerate(rk.l2g)}  # global 1-based -> local 0-based
            keep = [i for i, nd in enumerate(cl_nodes) if int(nd) in loc]
            shared += sum(1 for i in keep if cl_nodes[i] in mid)
            dof = [3 * loc[int(cl_nodes[i])] + cl_comp[i] + 1 for i in keep]
            rk.sv.set_loads(Loads(amps=AMPS, cload_dof=dof, cload_value=cl_val[keep], cload_amp=cl_amp[keep],
                                  grav_accel=grav, grav_amp=gamp))
        assert shared == 6                                       # both ranks gave the interface entries
        with pytest.raises(hakai.HakaiError) as ei:
            ranks[0].sv.set_loads(Loads(press_elem=[1], press_face=[1], press_value=[1.0]))
        assert ei.value.code == _abi.HAKAI_ERR_STATE
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


# ---- 6. refusals ----------------------------------------------------------------------------------------------------

BAD = {"dof": dict(cload_dof=[0], cload_value=[1.0]),
       "dof_high": dict(cload_dof=[10 ** 6], cload_value=[1.0]),
       "elem": dict(press_elem=[10 ** 6], press_face=[1], press_value=[1.0]),
       "face": dict(press_elem=[1], press_face=[7], press_value=[1.0]),
       "amp": dict(grav_accel=[[0, 0, 1.0]], grav_amp=[len(AMPS)]),
       "table": dict(amps=[([0.0], [1.0])], grav_accel=[[0, 0, 1.0]], grav_amp=[0]),
       "nan": dict(cload_dof=[1], cload_value=[np.nan]),
       "inf": dict(press_elem=[1], press_face=[1], press_value=[np.inf])}


def test_argument_errors_leave_the_loads_in_force():
    m = bc_bar()
    with Solver(m) as sv:
        f3 = sv.load_force(3)
        for name, kw in BAD.items():
            d = dict(amps=AMPS)
            d.update(kw)
            with pytest.raises(hakai.HakaiError) as ei:
                sv.set_loads(Loads(**d))
            assert ei.value.code == _abi.HAKAI_ERR_ARG, name
            assert bitwise_equal(sv.load_force(3), f3), name
        sv.step(1, 10)
        a = sv.download()
    with Solver(m) as sv:
        sv.step(1, 10)
        same_state(sv.download(), a)


# ---- 7. the driver ----------------------------------------------------------------------------------------------------

def test_driver_applies_the_decks_loads(tmp_path, monkeypatch):
    """hakai(fname) on a deck with *Dload gravity and *Dsload pressure: its history.csv (every step, full
    doubles) and last VTK equal the Solver run of the same Model."""
    base = mesh.bar_model(2, 2, 4, mesh.steel_ductile(), 0.0, perturb=0.02, n_steps=200)
    top = bar_end_elements(2, 2, 4)
    path = write_loads_deck(
        str(tmp_path / "deck.inp"), base,
        assembly=elset("_TOP", top) + "*Surface, type=ELEMENT, name=TOP\n_TOP, S2\n",
        amplitudes=amplitude("RAMP", tk(0, 100, 200), [0.0, 1.0, 0.5]),
        step="*Dload\n, GRAV, 9.81e6, 0., 0.6, -0.8\n**\n*Dsload, amplitude=RAMP\nTOP, P, -300.\n**\n")
    m = hakai.read_inp(path)
    assert len(m.loads.grav_accel) == 1 and m.loads.press_face.tolist() == [2] * 4
    monkeypatch.setenv("HAKAI_HISTORY", "1")
    out = tmp_path / "out"
    hakai.hakai(path, str(out), verbose=False)
    csv = read_history_csv(str(out / "history.csv"))
    with Solver(m) as sv:
        sv.set_tuning("elem_exact", 1)                           # the driver's element arithmetic
        sv.history_enable(m.history_sets[1], capacity=m.n_steps + 1)
        sv.step(1, m.n_steps)
        h = sv.history()
        disp = sv.download(disp=True).disp.reshape(-1, 3)
    assert bitwise_equal(csv["values"], h["values"]) and np.array_equal(csv["steps"], h["steps"])
    assert np.any(h["F_ext"][:, 0, :] != 0.0)
    txt = open(out / "file100.vtk").read().split("\n")
    i = txt.index("VECTORS DISPLACEMENT float")
    got = np.array([[float(x) for x in l.split()] for l in txt[i + 1:i + 1 + m.nNode]])
    assert np.allclose(got, disp, rtol=2e-6, atol=1e-12) and np.abs(disp).max() > 0
