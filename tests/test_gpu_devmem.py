"""Device memory on the GPU: hakai_stat "device_buffers" counts the device arrays the library holds
(hkc::DevBuf, hakai-fem_amd/csrc/hakai_devmem.hpp). A watcher context on a 1x1x2 bar reads it; every
case ends with its own contexts closed and the watcher reading its first value again, exactly: every
owner -- model, BCs, contact, loads, walls, history, stable step, mass scaling, the in-process
exchange, the drop-ins' temporaries -- gave back what it took, also after a refused call."""
import ctypes

import numpy as np
import pytest

import hakai
from hakai import _abi, dist, mesh
from hakai.model import BCGroup, Loads, Model, Walls
from hakai.solver import I64, Solver, State, cal_stress_hexa, cal_triax_stress, step_group
from hakai._abi import check, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture
def watch():
    """(read, base): the process-wide count through a context that outlives the case's own."""
    m = mesh.bar_model(1, 1, 2, mesh.steel_elastic(), 0.0)
    with Solver(m) as sv:
        base = sv.stat("device_buffers")
        assert base > 0  # the watcher's own arrays
        yield (lambda: sv.stat("device_buffers")), base
        assert sv.stat("device_buffers") == base


def upload_model(sv, m, element_material=None):
    mats, keep = m.c_materials()
    em = m.element_material if element_material is None else np.ascontiguousarray(element_material, np.int64)
    check(sv.L.hakai_upload_model(sv.ctx, m.nNode, ptr(m.coordmat), m.nElement, ptr(m.elementmat, I64), ptr(em, I64),
                                  len(m.materials), mats, ptr(sv.diag_M)))
    del keep


def set_bc(sv, m):
    bc, keep = m.c_bc()
    check(sv.L.hakai_set_bc(sv.ctx, ctypes.byref(bc)))
    del keep


def some_loads(m):
    """One concentrated load, gravity and one face pressure."""
    return Loads(cload_dof=[3 * m.nNode], cload_value=[5.0], grav_accel=[[0.0, 0.0, -9.81e3]], press_elem=[1],
                 press_face=[1], press_value=[2.0])


def some_wall(m):
    """One wall below the plate, with a node list."""
    return Walls(origin=[[0.0, 0.0, -1.0]], normal=[[0.0, 0.0, 1.0]], stiffness=[1e5], nodes=[np.arange(1, 10)])


def loaded(m):
    sv = Solver(m)
    sv.set_loads(some_loads(m))
    sv.set_walls(some_wall(m))
    sv.history_enable([np.arange(1, 5)])
    return sv


def test_full_life_of_one_context(watch):
    read, base = watch
    m = mesh.two_body_model()
    assert m.contact_flag >= 1
    with loaded(m) as sv:  # model, BCs and contact, then loads, a wall and the history
        assert read() >= base + 20
        sd = sv.stable_dt(per_element=True)
        assert sd["dt_est_elem"].shape == (m.nElement,) and sd["n_active"] == m.nElement
        sv.mass_scale(dt_target=2.0 * sd["dt_safe"])
        sv.step(1, 34)
        assert sv.graph_steps() > 0
        nodes = sv.node_stress_strain()
        assert nodes["node_stress"].shape == (m.nNode, 6)
        st = sv.download()
        flag = st.element_flag.copy()
        flag[m.nElement - 1] = 0
        sv.upload(State(disp=st.disp, disp_pre=st.disp_pre, velo=None, Q=st.Q, integ_stress=st.integ_stress,
                        integ_strain=st.integ_strain, integ_yield_stress=None, integ_eq_plastic_strain=None,
                        integ_triax_stress=None, element_flag=flag, Qe=None))
        sv.clear_loads()  # the wall stays
        assert np.all(sv.load_force(35) == 0.0)
        sv.set_tuning("nodal_padded", 0)
        held = read()
        upload_model(sv, m)
        assert base + 20 <= read() < held  # the first mesh's arrays and every state sized for it went
    assert read() == base


def test_steady_state_allocates_nothing(watch):
    read, base = watch
    m = mesh.two_body_model()
    with loaded(m) as sv:
        sv.step(1, 34)
        held = read()
        sv.step(35, 34)
        assert read() == held
        assert sv.graph_steps() > 0
    assert read() == base


def test_in_process_group(watch):
    read, base = watch
    ranks = [dist.bar_slab(2, 2, 8, r, 2, mesh.steel_elastic(), lambda z, L: 1e4 * z / L) for r in range(2)]
    svs = [Solver(loc, diag_M=diag) for loc, diag, _ in ranks]
    try:
        for r, (sv, (_, _, iface)) in enumerate(zip(svs, ranks)):
            sv.comm_init_local(r, 2, 771001)
            sv.set_interface(*iface)
            sv.history_enable([np.arange(1, 4)])
        assert read() >= base + 40
        step_group(svs, 1, 4)
        assert all(sv.history_count()[0] == 4 for sv in svs)
    finally:
        for sv in svs:
            sv.close()
    assert read() == base


def test_stateless_drop_ins(watch):
    read, base = watch
    m = mesh.bar_model(1, 1, 1, mesh.steel_elastic(), 0.0)
    Qe, vol = np.zeros((1, 24)), np.zeros(1)
    sg, sn, ys, eq = np.zeros((8, 6)), np.zeros((8, 6)), np.zeros(8), np.zeros(8)
    d_disp = np.zeros(3 * m.nNode)
    d_disp[2::3] = 1e-4 * m.coordmat[:, 2]
    cal_stress_hexa(Qe, sg, sn, ys, eq, m.coordmat, d_disp, m.elementmat, np.ones(1, np.int64), 8, None, m.materials,
                    m.element_material, None, vol)
    assert np.any(sg != 0.0) and vol[0] > 0.0
    assert read() == base
    tx = np.zeros(8)
    cal_triax_stress(sg, tx)
    assert np.any(tx != 0.0)
    assert read() == base


def test_refused_calls_hold_nothing_more(watch):
    read, base = watch
    m = mesh.two_body_model()
    with loaded(m) as sv:
        def refused(code, call):
            before = read()
            with pytest.raises(hakai.HakaiError) as ei:
                call()
            assert ei.value.code == code
            assert read() <= before

        bad_loads = some_loads(m)
        bad_loads.press_elem = np.array([m.nElement + 1], np.int64)
        refused(_abi.HAKAI_ERR_ARG, lambda: sv.set_loads(bad_loads))
        one_point = Model(m.coordmat, m.elementmat, m.element_material, m.materials,
                          bc=[BCGroup([(np.array([1], np.int64), 1.0)], np.array([1e-7]), np.array([1.0]))])
        refused(_abi.HAKAI_ERR_MODEL, lambda: set_bc(sv, one_point))
        em = m.element_material.copy()
        em[3] = len(m.materials) + 1
        refused(_abi.HAKAI_ERR_ARG, lambda: upload_model(sv, m, em))  # (last: it leaves the context without a model)
    assert read() == base
