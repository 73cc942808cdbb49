"""The .inp reader's load keywords (*Cload, *Dload, *Dsload; hakai_inp_model_t::loads) on the CPU:
decks written by the test with each keyword, amplitudes named and absent, a surface with mixed face
ids, each error case, and a committed deck without loads (every count 0, Model.loads None)."""
import ctypes
import os

import numpy as np
import pytest

import hakai
from hakai import _abi, mesh
from loads_cases import amplitude, bar_end_elements, elset, nset, write_loads_deck

NX, NY, NZ = 2, 2, 3


def bar():
    return mesh.bar_model(NX, NY, NZ, mesh.steel_elastic(), 0.0, perturb=0.0, n_steps=50)


def read(tmp_path, **kw):
    return hakai.read_inp(write_loads_deck(str(tmp_path / "deck.inp"), bar(), **kw))


def test_cload_sets_nodes_and_amplitude(tmp_path):
    m = bar()
    top = mesh.plane_nodes(NX, NY, NZ)
    a = read(tmp_path, assembly=nset("TOP", top) + nset("ONE", [5]),
             amplitudes=amplitude("RAMP", [0.0, 1e-6, 4e-6], [0.0, 1.0, 0.5]),
             step="*Cload, amplitude=RAMP\nTOP, 3, -2.5\nONE, 1, 4.0\nONE, 6, 9.0\n**\n"
                  "*Cload\nP1-1.7, 2, 1.5\n12, 1, -0.25\nONE, 1, 1.0\n**\n")
    ld = a.loads
    assert ld is not None and len(ld.grav_accel) == 0 and len(ld.press_elem) == 0
    want_dof = list(top * 3) + [5 * 3 - 2] + [7 * 3 - 1, 12 * 3 - 2, 5 * 3 - 2]     # direction 6 is ignored
    assert ld.cload_dof.tolist() == want_dof
    assert ld.cload_value.tolist() == [-2.5] * len(top) + [4.0, 1.5, -0.25, 1.0]
    assert ld.cload_amp.tolist() == [0] * (len(top) + 1) + [-1, -1, -1]
    assert len(ld.amps) == 1 and ld.amps[0][0].tolist() == [0.0, 1e-6, 4e-6] and ld.amps[0][1].tolist() == [0.0, 1.0, 0.5]
    assert np.array_equal(a.coordmat, m.coordmat) and np.array_equal(a.elementmat, m.elementmat)


def test_dload_gravity_and_element_pressure(tmp_path):
    top_e = bar_end_elements(NX, NY, NZ)
    a = read(tmp_path, assembly=elset("TOPE", top_e),
             amplitudes=amplitude("G", [0.0, 1e-5], [1.0, 1.0]),
             step="*Dload, amplitude=G\n, GRAV, 9810., 0., 0.6, -0.8\n**\n*Dload\nTOPE, P2, 12.5\n, GRAV, 2., 1., 0., 0.\n**\n")
    ld = a.loads
    assert ld.grav_accel.tolist() == [[9810. * 0., 9810. * 0.6, 9810. * -0.8], [2.0, 0.0, 0.0]]
    assert ld.grav_amp.tolist() == [0, -1]
    assert ld.press_elem.tolist() == top_e.tolist() and ld.press_face.tolist() == [2] * len(top_e)
    assert ld.press_value.tolist() == [12.5] * len(top_e) and ld.press_amp.tolist() == [-1] * len(top_e)
    assert len(ld.cload_dof) == 0


def test_dsload_surface_with_mixed_faces(tmp_path):
    m = bar()
    top_e, bot_e = bar_end_elements(NX, NY, NZ), bar_end_elements(NX, NY, NZ, top=False)
    a = read(tmp_path, assembly=elset("_S_TOP", top_e) + elset("_S_BOT", bot_e[:2])
             + "*Surface, type=ELEMENT, name=SKIN\n_S_TOP, S2\n_S_BOT, S1\n",
             amplitudes=amplitude("PULSE", [0.0, 1e-6], [0.0, 2.0]),
             step="*Dsload, amplitude=PULSE\nSKIN, P, 3.0\n**\n*Dsload\nSKIN, P, -1.0\n**\n")
    ld = a.loads
    n = len(top_e) + 2
    assert ld.press_elem.tolist() == 2 * (top_e.tolist() + bot_e[:2].tolist())
    assert ld.press_face.tolist() == 2 * ([2] * len(top_e) + [1, 1])
    assert ld.press_value.tolist() == [3.0] * n + [-1.0] * n and ld.press_amp.tolist() == [0] * n + [-1] * n
    # S2 of the top layer and S1 of the bottom layer are the bar's end planes
    import loads_ref
    L = m.coordmat[:, 2].max()
    for e, f in zip(ld.press_elem[:n], ld.press_face[:n]):
        z = m.coordmat[m.elementmat[e - 1][list(loads_ref.FACE_NODES[f - 1])] - 1, 2]
        assert np.all(z == (L if f == 2 else 0.0))
    assert a.contact_pairs is None and a.contact_flag == 0          # a surface alone is no contact


def test_contact_pair_surfaces_unchanged(tmp_path):
    """What *Contact Pair sees of a *Surface does not change with the kept face ids."""
    from inp_writer import write_inp
    m = mesh.two_body_model(surfaces=True)
    a = hakai.read_inp(write_inp(str(tmp_path / "cp.inp"), m))
    for p, q in zip(a.contact_pairs, m.contact_pairs):
        for (ia, ea), (ib, eb) in zip(p, q):
            assert ia == ib and np.array_equal(ea, eb)
    assert a.loads is None


ERRORS = {
    "unknown_load_type": dict(assembly=elset("E1", [1]), step="*Dload\nE1, BX, 1.0\n**\n"),
    "unknown_dsload_type": dict(assembly=elset("E1", [1]) + "*Surface, type=ELEMENT, name=S\nE1, S1\n",
                                step="*Dsload\nS, HP, 1.0\n**\n"),
    "unknown_surface": dict(step="*Dsload\nNOPE, P, 1.0\n**\n"),
    "unknown_elset": dict(step="*Dload\nNOPE, P1, 1.0\n**\n"),
    "unknown_nset": dict(step="*Cload\nNOPE, 1, 1.0\n**\n"),
    "node_out_of_range": dict(step="*Cload\n999, 1, 1.0\n**\n"),
    "unknown_amplitude": dict(step="*Cload, amplitude=NOPE\n3, 1, 1.0\n**\n"),
    "grav_on_a_set": dict(assembly=elset("E1", [1]), step="*Dload\nE1, GRAV, 9.81, 0., 0., -1.\n**\n"),
    "surface_without_face": dict(assembly=elset("E1", [1]) + "*Surface, type=ELEMENT, name=S\nE1\n",
                                 step="*Dsload\nS, P, 1.0\n**\n"),
    "short_cload_line": dict(step="*Cload\n3, 1\n**\n"),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_reader_errors(tmp_path, name):
    with pytest.raises(hakai.HakaiError) as ei:
        read(tmp_path, **ERRORS[name])
    assert ei.value.code == _abi.HAKAI_ERR_IO


def test_deck_without_loads_has_zero_counts(ref_decks):
    path = os.path.join(ref_decks, "HAKAI-v0.0.0/input/Tensile5e.inp")
    out = ctypes.POINTER(_abi.InpModelT)()
    _abi.check(hakai.lib().hakai_inp_read(path.encode(), ctypes.byref(out)))
    try:
        ld = out.contents.loads
        assert (ld.n_amp, ld.n_cload, ld.n_grav, ld.n_press) == (0, 0, 0, 0)
    finally:
        hakai.lib().hakai_inp_free(out)
    a, b = hakai.read_inp(path), mesh.tensile5e_model()
    assert a.loads is None
    assert np.array_equal(a.coordmat, b.coordmat) and np.array_equal(a.elementmat, b.elementmat)
    assert len(a.bc) == len(b.bc)


def test_n_gpu_driver_refuses_loads(tmp_path):
    from hakai import run
    path = write_loads_deck(str(tmp_path / "deck.inp"), bar(), step="*Dload\n, GRAV, 9810., 0., 0., -1.\n**\n")
    with pytest.raises(ValueError, match="external loads"):
        run.hakai_multi(path, out_dir=str(tmp_path / "out"), local_ranks=2, verbose=False)
