"""Template form of the owner-assembly entry lists on the GPU (tuning key "own_templates").

The kernel reads a 16-byte header per super-batch and the shared relative entries instead of the
plain list, adds the header's bases to the targets and derives the LDS slot as node mod P
(csrc/hakai_own_plan.hpp, hakai_own_pass.hpp own_load_tpl / own_entry). The additions and their order
are the plain form's, so every run here must be BIT-identical, in every downloaded field and in the
deletion log, to the same run with own_templates 0 and to the fe path (own_assembly 0). Grids are
forced small so that most sums straddle blocks and the head and tail passes of block runs dominate.
The plans themselves are replayed on the CPU in tests/test_own_templates.py.
"""
import dataclasses

import numpy as np
import pytest

from hakai import mesh
from hakai.model import BCGroup
from hakai.solver import Solver
from util import STATE, shuffled

pytestmark = pytest.mark.gpu

STEPS = 60
DT = 2e-8


def pulled_bar(nx, ny, nz, pull=2.0, steps=STEPS, seed=5):
    """Bar clamped at z = 0 whose free end is pulled `pull` element lengths within `steps` steps: the
    top layers yield at once and are deleted before the call ends."""
    m = mesh.bar_model(nx, ny, nz, mesh.steel_ductile(), 0.0, perturb=0.02, seed=seed, d_time=DT, n_steps=steps,
                       name="pulled_bar")
    top = mesh.plane_nodes(nx, ny, nz)
    m.bc.append(BCGroup([(top * 3, pull)], np.array([0.0, steps * DT]), np.array([0.0, 1.0])))
    return m


def run(m, tune, own, templates, calls=((1, STEPS),), graph=None, exact=0):
    with Solver(m) as sv:
        for k, v in tune.items():
            sv.set_tuning(k, v)
        sv.set_tuning("elem_exact", exact)
        sv.set_tuning("own_assembly", own)
        sv.set_tuning("own_templates", templates)
        if graph is not None:
            sv.set_tuning("graph", graph)
        for t0, n in calls:
            sv.step(t0, n)
        g = sv.download()
        dels = [tuple(x) for x in sv.deleted()]
        st = {k: sv.stat(k) for k in ("own_steps", "own_entries", "own_entries_stored", "own_templates", "own_slots",
                                      "graph_steps")}
    return g, dels, st


def same(a, b):
    ga, da, _ = a
    gb, db, _ = b
    for k in STATE + ("integ_triax_stress",):
        assert np.array_equal(getattr(ga, k), getattr(gb, k)), k
    assert da == db


def three_ways(m, tune, own=1, fits=True, **kw):
    """own_templates 1 against own_templates 0 and against the fe path; returns the three runs.
    fits: the mesh is known to take owner assembly (a shuffled one may need too many open sums)."""
    t1 = run(m, tune, own, 1, **kw)
    t0 = run(m, tune, own, 0, **kw)
    fe = run(m, tune, 0, 1, **kw)
    n = sum(c[1] for c in kw.get("calls", ((1, STEPS),)))
    assert t1[2]["own_steps"] == t0[2]["own_steps"] and fe[2]["own_steps"] == 0, (t1[2], t0[2], fe[2])
    assert t1[2]["own_steps"] == n or not fits, t1[2]
    assert t0[2]["own_templates"] == 0 and t0[2]["own_entries_stored"] == t0[2]["own_entries"], t0[2]
    assert t1[2]["own_entries"] == t0[2]["own_entries"], (t1[2], t0[2])  # entries executed per step
    same(t1, t0)
    same(t1, fe)
    return t1, t0, fe


def grid(blocks):
    return {"elem_pipe_min": 0, "elem_pipe_blocks": blocks}


@pytest.fixture(scope="module")
def bar20():
    return pulled_bar(20, 20, 40)


@pytest.mark.parametrize("graph", [0, 16])
@pytest.mark.parametrize("blocks", [3, 16])
def test_templates_deleting_bar_fused(bar20, blocks, graph):
    """20x20x40 deleting bar, 500 batches on 3 and on 16 blocks, stream mode and graphs."""
    t1, _, _ = three_ways(bar20, grid(blocks), graph=graph)
    s = t1[2]
    assert s["own_templates"] > 0 and s["own_entries_stored"] < s["own_entries"], s
    assert (s["graph_steps"] > 0) == (graph > 0), s
    assert len(t1[1]) > 0  # elements were deleted
    assert np.any(t1[0].integ_eq_plastic_strain > 0)


@pytest.mark.parametrize("blocks", [3, 16])
def test_templates_deleting_bar_reference_order(bar20, blocks):
    """Reference-order kernel with own_assembly 2: fewer LDS slots, so P is no power of two."""
    t1, _, _ = three_ways(bar20, grid(blocks), own=2, exact=1)
    s = t1[2]
    assert s["own_templates"] > 0 and s["own_slots"] & (s["own_slots"] - 1), s
    assert len(t1[1]) > 0


def test_templates_no_period_divides_the_batch():
    """7x5x33: 35-element layers against 64-element super-batches on 4 blocks -- every pass is its
    own template, head and tail passes included."""
    t1, _, _ = three_ways(pulled_bar(7, 5, 33), grid(4))
    assert t1[2]["own_templates"] > 0, t1[2]
    assert len(t1[1]) > 0


def test_templates_two_materials():
    """Two materials, alternating by element layer: the element kernel's material load has stride 4
    (one material: stride 0)."""
    m = pulled_bar(6, 5, 60)
    soft = dataclasses.replace(mesh.steel_ductile(), name="soft", young=150000.0, plastic=mesh.STEEL_PLASTIC * [0.8, 1.0])
    em = np.ones(m.nElement, np.int64)
    em[(np.arange(m.nElement) // 30) % 2 == 1] = 2
    m = dataclasses.replace(m, element_material=em, materials=[mesh.steel_ductile(), soft])
    t1, _, _ = three_ways(m, grid(5))
    assert t1[2]["own_templates"] > 0, t1[2]
    one = run(pulled_bar(6, 5, 60), grid(5), 1, 1)
    assert not np.array_equal(one[0].integ_stress, t1[0].integ_stress)  # the second material is in use


def test_templates_toggled_between_calls_with_upload(bar20):
    """own_templates switched between calls, a state upload in between: each switch re-plans."""
    def go(own, toggle):
        with Solver(bar20) as sv:
            for k, v in grid(16).items():
                sv.set_tuning(k, v)
            sv.set_tuning("own_assembly", own)
            seen = []
            for t0, n, tpl in ((1, 21, 1), (22, 20, 0), (42, 19, 1)):
                sv.set_tuning("own_templates", tpl if toggle else 0)
                if t0 > 1:
                    sv.upload(sv.download())
                sv.step(t0, n)
                seen.append(sv.stat("own_templates"))
            return (sv.download(), [tuple(x) for x in sv.deleted()], None), seen
    a, seen = go(1, True)
    b, seen0 = go(1, False)
    c, _ = go(0, False)
    assert seen[0] > 0 and seen[1] == 0 and seen[2] == seen[0], seen
    assert seen0 == [0, 0, 0]
    same(a, b)
    same(a, c)


def test_templates_shuffled_numbering_keeps_plain_form():
    """Shuffled 3x3x200 bar: no node mod P separates the open sums, so the plain lists stay."""
    m = shuffled(pulled_bar(3, 3, 200), seed=11)
    t1, _, _ = three_ways(m, grid(8), fits=False)
    assert t1[2]["own_templates"] == 0 and t1[2]["own_entries_stored"] == t1[2]["own_entries"], t1[2]
