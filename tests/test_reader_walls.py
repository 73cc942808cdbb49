"""The .inp reader's *Rigid Wall keyword (hakai_inp_model_t::walls) on the CPU: every parameter and the
defaults, a node set mapped to global ids through the instance offsets, an amplitude by name, each
error case, a committed deck without walls (n_wall 0, Model.walls None) and the N-GPU driver's refusal."""
import ctypes
import os

import numpy as np
import pytest

import hakai
from hakai import _abi, mesh
from inp_writer import write_inp
from loads_cases import amplitude, nset, write_loads_deck
from walls_cases import rigid_wall

NX, NY, NZ = 2, 2, 3


def bar():
    return mesh.bar_model(NX, NY, NZ, mesh.steel_elastic(), 0.0, perturb=0.0, n_steps=50)


def read(tmp_path, model=None, **kw):
    return hakai.read_inp(write_loads_deck(str(tmp_path / "deck.inp"), model or bar(), **kw))


def test_every_parameter_and_the_defaults(tmp_path):
    m = bar()
    top = mesh.plane_nodes(NX, NY, NZ)
    a = read(tmp_path, assembly=nset("TOP", top),
             amplitudes=amplitude("PUSH", [0.0, 1e-6, 4e-6], [0.0, 1.0, 0.5]) + amplitude("OTHER", [0.0, 1.0], [1.0, 2.0]),
             step=rigid_wall("FLOOR", (0.5, 0.25, -0.125), (0, 0, 2))
             + rigid_wall("PLATEN", (0, 0, 3.5), (0, 0.6, -0.8), (0, 0, -1.5), nset="TOP", amplitude="PUSH",
                          stiffness=2.5e5, scale=0.25, damping=0.125, friction=0.375)
             + rigid_wall("SIDE", (1, 2, 3), (-1, 0, 0), friction=0.5, amplitude="OTHER") + "**\n")
    w = a.walls
    assert w is not None and w.n_wall == 3 and not w.empty
    assert w.origin.tolist() == [[0.5, 0.25, -0.125], [0, 0, 3.5], [1, 2, 3]]
    assert w.normal.tolist() == [[0, 0, 2], [0, 0.6, -0.8], [-1, 0, 0]]          # as written: the library normalises
    assert w.motion.tolist() == [[0, 0, 0], [0, 0, -1.5], [0, 0, 0]]
    assert w.stiffness.tolist() == [0.0, 2.5e5, 0.0] and w.scale.tolist() == [0.5, 0.25, 0.5]
    assert w.damping.tolist() == [0.0, 0.125, 0.0] and w.friction.tolist() == [0.0, 0.375, 0.5]
    assert w.amp.tolist() == [-1, 0, 1]
    assert [len(x) for x in w.nodes] == [0, len(top), 0] and w.nodes[1].tolist() == top.tolist()
    assert w.amps[0][0].tolist() == [0.0, 1e-6, 4e-6] and w.amps[0][1].tolist() == [0.0, 1.0, 0.5]
    assert w.amps[1][1].tolist() == [1.0, 2.0]
    assert a.loads is None
    assert np.array_equal(a.coordmat, m.coordmat) and np.array_equal(a.elementmat, m.elementmat)
    s, keep = w.c()                                         # round trip into the C struct
    assert s.n_wall == 3 and s.n_amp == 2 and [s.node_off[k] for k in range(4)] == [0, 0, len(top), len(top)]
    del keep


def test_nset_maps_through_the_instance_offset(tmp_path):
    m = mesh.two_body_model(plate=(2, 2, 1), impactor=(1, 1, 2), contact_flag=0)
    n1 = 3 * 3 * 2
    a = read(tmp_path, model=m, assembly=nset("IMP", [1, 2, 5], instance="P2-1") + nset("PL", [4], instance="P1-1"),
             step=rigid_wall("A", (0, 0, 0), (0, 0, 1), nset="IMP") + rigid_wall("B", (0, 0, 0), (0, 0, 1), nset="PL"))
    assert a.walls.nodes[0].tolist() == [n1 + 1, n1 + 2, n1 + 5] and a.walls.nodes[1].tolist() == [4]


def walls33():
    return "".join(rigid_wall(f"W{k}", (0, 0, -k), (0, 0, 1)) for k in range(33))


ERRORS = {
    "unknown_parameter": dict(step="*Rigid Wall, name=F, stifness=1.0\n0,0,0,0,0,1\n"),
    "bare_parameter": dict(step="*Rigid Wall, name=F, friction\n0,0,0,0,0,1\n"),
    "unknown_nset": dict(step=rigid_wall("F", (0, 0, 0), (0, 0, 1), nset="NOPE")),
    "unknown_amplitude": dict(step=rigid_wall("F", (0, 0, 0), (0, 0, 1), amplitude="NOPE")),
    "short_data_line": dict(step="*Rigid Wall, name=F\n0, 0, 0, 0, 1\n"),
    "seven_values": dict(step="*Rigid Wall, name=F\n0, 0, 0, 0, 0, 1, 2\n"),
    "ten_values": dict(step="*Rigid Wall, name=F\n0, 0, 0, 0, 0, 1, 0, 0, 1, 4\n"),
    "not_a_number": dict(step="*Rigid Wall, name=F\n0, 0, zero, 0, 0, 1\n"),
    "bad_parameter_value": dict(step="*Rigid Wall, name=F, friction=lots\n0, 0, 0, 0, 0, 1\n"),
    "no_data_line": dict(step="*Rigid Wall, name=F\n**\n"),
    "two_data_lines": dict(step="*Rigid Wall, name=F\n0, 0, 0, 0, 0, 1\n0, 0, 1, 0, 0, 1\n"),
    "no_name": dict(step="*Rigid Wall, friction=0.5\n0, 0, 0, 0, 0, 1\n"),
    "thirty_three_walls": dict(step=walls33()),
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_reader_errors(tmp_path, name):
    with pytest.raises(hakai.HakaiError) as ei:
        read(tmp_path, **ERRORS[name])
    assert ei.value.code == _abi.HAKAI_ERR_IO


def test_thirty_two_walls_parse(tmp_path):
    a = read(tmp_path, step=walls33()[:-len(rigid_wall("W32", (0, 0, -32), (0, 0, 1)))])
    assert a.walls.n_wall == 32 and a.walls.origin[31].tolist() == [0, 0, -31]


def test_deck_without_walls_has_zero_counts(ref_decks):
    path = os.path.join(ref_decks, "HAKAI-v0.0.0/input/Tensile5e.inp")
    out = ctypes.POINTER(_abi.InpModelT)()
    _abi.check(hakai.lib().hakai_inp_read(path.encode(), ctypes.byref(out)))
    try:
        w = out.contents.walls
        assert (w.n_amp, w.n_wall) == (0, 0)
    finally:
        hakai.lib().hakai_inp_free(out)
    a, b = hakai.read_inp(path), mesh.tensile5e_model()
    assert a.walls is None and a.loads is None
    assert np.array_equal(a.coordmat, b.coordmat) and np.array_equal(a.elementmat, b.elementmat)


def test_struct_layout():
    """hakai_walls_t: two int32 counts, each followed by pointers (x86-64 SysV: padded to 8)."""
    assert ctypes.sizeof(_abi.WallsT) == 8 + 4 * 8 + 8 + 10 * 8
    assert _abi.InpModelT.walls.offset == _abi.InpModelT.loads.offset + ctypes.sizeof(_abi.LoadsT)
    assert {"hakai_set_walls", "hakai_clear_walls", "hakai_wall_force"} <= set(_abi.exported_symbols())


def test_n_gpu_driver_refuses_walls(tmp_path):
    from hakai import run
    path = write_loads_deck(str(tmp_path / "deck.inp"), bar(), step=rigid_wall("FLOOR", (0, 0, -0.5), (0, 0, 1)))
    with pytest.raises(ValueError, match="rigid walls"):
        run.hakai_multi(path, out_dir=str(tmp_path / "out"), local_ranks=2, verbose=False)
