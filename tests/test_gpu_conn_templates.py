"""Connectivity templates on the GPU (tuning key "conn_templates").

The owner-assembly template variants of the fused element kernel read one packed 4-byte record per
element (base node and pattern id) and a small table of node offsets instead of the 32-byte
connectivity row (csrc/hakai_conn_plan.hpp, hakai_elem_io.hpp conn_rec / conn_off / conn_node). The
node ids are the same numbers, so every run here must be BIT-identical, in every downloaded field and
in the deletion log, to the same run with conn_templates 0. The stat conn_patterns says which form
ran: the number of patterns, or 0 for the plain array -- key off, a mesh above the pattern cap, or the
reference-order kernel, which keeps the plain array. Grids are forced small so that the
persistent kernel runs on these meshes, down to blocks with fewer batches than its pipeline is deep.
The planner itself is checked on the CPU in tests/test_conn_templates.py.
"""
import dataclasses

import numpy as np
import pytest

from hakai import mesh
from hakai.model import BCGroup
from hakai.solver import Solver
from util import STATE, bitwise_equal, shuffled

pytestmark = pytest.mark.gpu

STEPS = 30
DT = 2e-8


def pulled_bar(nx, ny, nz, pull=2.0, steps=STEPS, seed=5):
    """Bar clamped at z = 0 whose free end is pulled `pull` element lengths within `steps` steps: the
    top layers yield at once and are deleted before the call ends."""
    m = mesh.bar_model(nx, ny, nz, mesh.steel_ductile(), 0.0, perturb=0.02, seed=seed, d_time=DT, n_steps=steps,
                       name="pulled_bar")
    top = mesh.plane_nodes(nx, ny, nz)
    m.bc.append(BCGroup([(top * 3, pull)], np.array([0.0, steps * DT]), np.array([0.0, 1.0])))
    return m


def grid(blocks):
    return {"elem_pipe_min": 0, "elem_pipe_blocks": blocks}


def run(m, tune, conn, calls=((1, STEPS),), graph=None, exact=0, switch=None):
    """switch: conn_templates per call (else `conn` throughout); returns state, deletions, stats and the
    conn_patterns seen after each call."""
    with Solver(m) as sv:
        for k, v in tune.items():
            sv.set_tuning(k, v)
        sv.set_tuning("elem_exact", exact)
        sv.set_tuning("own_assembly", 2 if exact else 1)
        if graph is not None:
            sv.set_tuning("graph", graph)
        seen = []
        for i, (t0, n) in enumerate(calls):
            sv.set_tuning("conn_templates", switch[i] if switch else conn)
            sv.step(t0, n)
            seen.append(sv.stat("conn_patterns"))
        g = sv.download()
        dels = [tuple(x) for x in sv.deleted()]
        st = {k: sv.stat(k) for k in ("conn_patterns", "conn_bytes", "own_steps", "own_templates", "graph_steps")}
    return g, dels, st, seen


def same(a, b):
    for k in STATE + ("integ_triax_stress",):
        assert bitwise_equal(getattr(a[0], k), getattr(b[0], k)), k
    assert a[1] == b[1]


def both(m, tune, compressed=True, **kw):
    """conn_templates 1 against 0: identical results; the stats say which form each run used."""
    c1 = run(m, tune, 1, **kw)
    c0 = run(m, tune, 0, **kw)
    nEp = -(-m.nElement // 32) * 32
    assert c0[2]["conn_patterns"] == 0 and c0[2]["conn_bytes"] == 32 * nEp, c0[2]
    if compressed:
        p = c1[2]["conn_patterns"]
        assert p > 0 and c1[2]["conn_bytes"] == 4 * nEp + 32 * p, c1[2]
        assert c1[2]["own_templates"] > 0 and c1[2]["own_steps"] == sum(n for _, n in kw.get("calls", ((1, STEPS),))), c1[2]
    else:
        assert c1[2]["conn_patterns"] == 0 and c1[2]["conn_bytes"] == 32 * nEp, c1[2]
    same(c1, c0)
    return c1, c0


@pytest.fixture(scope="module")
def bar140():
    return pulled_bar(5, 4, 7)


@pytest.mark.parametrize("graph", [0, 16])
@pytest.mark.parametrize("exact", [0, 1])
def test_bar_140_elements(bar140, exact, graph):
    """5x4x7: 140 elements, 4.4 batches on two blocks; fused and reference order (plain array: the key
    must change nothing there), stream and graphs."""
    c1, _ = both(bar140, grid(2), compressed=not exact, exact=exact, graph=graph)
    assert c1[2]["conn_patterns"] == (0 if exact else 2)  # the lattice's pattern and the padding's
    assert c1[2]["own_templates"] > 0 and c1[2]["own_steps"] == STEPS, c1[2]
    assert (c1[2]["graph_steps"] > 0) == (graph > 0), c1[2]
    assert np.any(c1[0].integ_eq_plastic_strain > 0)


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("dims,blocks", [((1, 1, 33), 1), ((1, 1, 33), 2), ((3, 2, 4), 1)])
def test_blocks_shorter_than_the_pipeline(dims, blocks, exact):
    """nE = 33 (two batches, on one block and on two) and nE = 24 (one batch): iterations past a
    block's end re-load its last batch, records and offsets included."""
    m = pulled_bar(*dims)
    assert m.nElement in (33, 24)
    both(m, grid(blocks), compressed=not exact, exact=exact)


def test_two_materials():
    """Alternating materials by element layer: the material load next to the record has stride 4."""
    m = pulled_bar(6, 5, 20)
    soft = dataclasses.replace(mesh.steel_ductile(), name="soft", young=150000.0, plastic=mesh.STEEL_PLASTIC * [0.8, 1.0])
    em = np.ones(m.nElement, np.int64)
    em[(np.arange(m.nElement) // 30) % 2 == 1] = 2
    m2 = dataclasses.replace(m, element_material=em, materials=[mesh.steel_ductile(), soft])
    c1, _ = both(m2, grid(5))
    one = run(m, grid(5), 1)
    assert not np.array_equal(one[0].integ_stress, c1[0].integ_stress)  # the second material is in use


def test_deletion_within_the_run():
    """4x4x30 pulled to deletion: the flags change from step to step, the records never do."""
    c1, _ = both(pulled_bar(4, 4, 30, steps=60), grid(4), calls=((1, 60),))
    assert len(c1[1]) > 0  # elements were deleted


def test_above_the_pattern_cap_keeps_the_plain_array():
    """Shuffled 3x3x200: every element has its own pattern, 1800 against a cap of 256."""
    both(shuffled(pulled_bar(3, 3, 200), seed=11), grid(8), compressed=False)


def test_switched_between_calls(bar140):
    """conn_templates 1, 0, 1 over three calls on one solver (graphs of 16 steps in each call): the
    captured graphs are dropped at each switch, and the state equals an unswitched run's."""
    calls = ((1, 20), (21, 20), (41, 20))
    a = run(bar140, grid(2), 1, calls=calls, switch=(1, 0, 1))
    b = run(bar140, grid(2), 1, calls=calls)
    c = run(bar140, grid(2), 0, calls=calls)
    assert a[3][0] > 0 and a[3][1] == 0 and a[3][2] == a[3][0], a[3]
    assert all(p > 0 for p in b[3]) and c[3] == [0, 0, 0], (b[3], c[3])
    assert a[2]["graph_steps"] > 0, a[2]
    same(a, b)
    same(a, c)
