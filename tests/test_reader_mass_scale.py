"""The .inp reader's *Variable Mass Scaling keyword (hakai_inp_model_t::vms_*) on the CPU: the defaults,
every parameter, each parse error, that *Fixed Mass Scaling still parses next to it, a committed deck
without the keyword (vms_set 0, Model.variable_mass_scaling None, the same model as before), the
ctypes mirror of the struct against the C compiler's layout, and the N-GPU driver's refusal."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hakai
from hakai import _abi, mesh
from loads_cases import write_loads_deck

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INF = float("inf")


def bar():
    return mesh.bar_model(2, 2, 3, mesh.steel_elastic(), 0.0, perturb=0.0, n_steps=50)


def read(tmp_path, model=None, **kw):
    return hakai.read_inp(write_loads_deck(str(tmp_path / "deck.inp"), model or bar(), **kw))


def test_defaults(tmp_path):
    m = bar()
    a = read(tmp_path, step="*Variable Mass Scaling\n**\n")
    assert a.variable_mass_scaling == dict(dt=None, safety=0.9, max_factor=INF, repeat=False)
    assert a.mass_scaling == m.mass_scaling and a.dt == m.dt
    assert np.array_equal(a.coordmat, m.coordmat) and np.array_equal(a.elementmat, m.elementmat)
    assert a.loads is None and a.walls is None


def test_every_parameter(tmp_path):
    a = read(tmp_path, step="*Variable Mass Scaling, dt=2.5e-7, safety=0.75, max factor=12.5, repeat=output\n")
    assert a.variable_mass_scaling == dict(dt=2.5e-7, safety=0.75, max_factor=12.5, repeat=True)
    b = read(tmp_path, step="*Variable Mass Scaling, repeat=output, max factor=1, safety=1\n")
    assert b.variable_mass_scaling == dict(dt=None, safety=1.0, max_factor=1.0, repeat=True)
    c = read(tmp_path, step="*Variable Mass Scaling, dt = 1e-8\n")          # blanks round '=' as the reader strips them
    assert c.variable_mass_scaling == dict(dt=1e-8, safety=0.9, max_factor=INF, repeat=False)


def test_fixed_mass_scaling_still_parses_next_to_it(tmp_path):
    m = bar()
    m.mass_scaling = 100.0
    a = read(tmp_path, model=m, step="*Variable Mass Scaling, safety=0.5\n")
    plain = read(tmp_path, model=m)
    assert a.mass_scaling == plain.mass_scaling == 100.0 and a.dt == plain.dt == m.dt
    assert a.variable_mass_scaling["safety"] == 0.5 and plain.variable_mass_scaling is None


ERRORS = {
    "unknown_parameter": "*Variable Mass Scaling, saftey=0.9\n",
    "bare_parameter": "*Variable Mass Scaling, safety\n",
    "bad_dt": "*Variable Mass Scaling, dt=fast\n",
    "empty_dt": "*Variable Mass Scaling, dt=\n",
    "zero_dt": "*Variable Mass Scaling, dt=0\n",
    "negative_dt": "*Variable Mass Scaling, dt=-1e-7\n",
    "safety_zero": "*Variable Mass Scaling, safety=0\n",
    "safety_above_one": "*Variable Mass Scaling, safety=1.5\n",
    "bad_safety": "*Variable Mass Scaling, safety=0.9x\n",
    "max_factor_below_one": "*Variable Mass Scaling, max factor=0.5\n",
    "bad_max_factor": "*Variable Mass Scaling, max factor=big\n",
    "repeat_other": "*Variable Mass Scaling, repeat=step\n",
    "longer_keyword": "*Variable Mass Scaling Extra, dt=1e-7\n",
    "twice": "*Variable Mass Scaling\n*Variable Mass Scaling, safety=0.5\n",
}


@pytest.mark.parametrize("name", sorted(ERRORS))
def test_reader_errors(tmp_path, name):
    with pytest.raises(hakai.HakaiError) as ei:
        read(tmp_path, step=ERRORS[name])
    assert ei.value.code == _abi.HAKAI_ERR_IO


def test_deck_without_the_keyword_is_the_model_it_was(ref_decks):
    path = os.path.join(ref_decks, "HAKAI-v0.0.0/input/Tensile5e.inp")
    out = ctypes.POINTER(_abi.InpModelT)()
    _abi.check(hakai.lib().hakai_inp_read(path.encode(), ctypes.byref(out)))
    try:
        p = out.contents
        assert (p.vms_set, p.vms_repeat, p.vms_dt, p.vms_safety, p.vms_max_factor) == (0, 0, 0.0, 0.9, INF)
    finally:
        hakai.lib().hakai_inp_free(out)
    a, b = hakai.read_inp(path), mesh.tensile5e_model()
    assert a.variable_mass_scaling is None and a.walls is None and a.loads is None
    assert np.array_equal(a.coordmat, b.coordmat) and np.array_equal(a.elementmat, b.elementmat)
    assert a.mass_scaling == b.mass_scaling and a.d_time == b.d_time and a.end_time == b.end_time


LAYOUT = r"""
#include <stddef.h>
#include <stdio.h>
#include "hakai_hip.h"
int main(void) {
    printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", sizeof(hakai_inp_model_t), offsetof(hakai_inp_model_t, walls),
           offsetof(hakai_inp_model_t, vms_set), offsetof(hakai_inp_model_t, vms_repeat),
           offsetof(hakai_inp_model_t, vms_dt), offsetof(hakai_inp_model_t, vms_safety),
           offsetof(hakai_inp_model_t, vms_max_factor), sizeof(hakai_mass_scale_t));
    return 0;
}
"""


def test_struct_layout_matches_the_c_compiler(tmp_path):
    """The new fields are appended after walls, and the ctypes mirrors have the header's layout."""
    c, exe = tmp_path / "layout.c", tmp_path / "layout"
    c.write_text(LAYOUT)
    subprocess.run(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    T = _abi.InpModelT
    assert got == [ctypes.sizeof(T), T.walls.offset, T.vms_set.offset, T.vms_repeat.offset, T.vms_dt.offset,
                   T.vms_safety.offset, T.vms_max_factor.offset, ctypes.sizeof(_abi.MassScaleT)]
    assert T.vms_set.offset == T.walls.offset + ctypes.sizeof(_abi.WallsT)
    assert ctypes.sizeof(_abi.MassScaleT) == 10 * 8
    assert {"hakai_mass_scale", "hakai_mass_scale_get", "hakai_clear_mass_scale"} <= set(_abi.exported_symbols())
    L = hakai.lib()
    assert all(hasattr(L, s) for s in ("hakai_mass_scale", "hakai_mass_scale_get", "hakai_clear_mass_scale"))


def test_n_gpu_driver_refuses_the_deck(tmp_path):
    from hakai import run
    path = write_loads_deck(str(tmp_path / "deck.inp"), bar(), step="*Variable Mass Scaling\n")
    with pytest.raises(ValueError, match="Variable Mass Scaling"):
        run.hakai_multi(path, out_dir=str(tmp_path / "out"), local_ranks=2, verbose=False)
