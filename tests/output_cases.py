"""Crafted inputs for the output node averages (tests/test_output_ref_cpu.py on the CPU,
tests/test_gpu_output.py on the device). Plain module, shared by both so that the CPU test pins
exactly the meshes and Gauss-point values the device test uploads.

A case is a mesh (as a Model, so that the device test can upload it) and the five arrays
cal_node_stress_strain reads plus the element flags:

  n8, n255, n256, n257, n513   one element; bars 2x4x16, 3x7x7, the 3x7x7 bar plus one node no
                   element uses (its last), 2x8x18. k_node_average launches blocks of 256 nodes:
                   the sizes sit on both sides of one and two full blocks, n257's second block holds
                   the unused node alone. nE = 1, 128, 147, 147, 288: the Gauss-point arrays' leading
                   dimension 8 * roundup(nE, 32) is padded for all but 128 and 288.
  dup16            every element of the 2x4x16 bar twice: up to 16 incidences per node
  shuffled         the 3x7x7 bar with elements and nodes renumbered at random; magnitudes from
                   1e-12 to 1e8, so every node's sum depends on the order of its elements
  shuffled_dup257  all three at once: the shuffled bar, every element twice, one unused last node
  deleted          a third of the elements with flag 0, zero stress and strain, but eqps and triax
                   kept: they still count in the divisor
  cancel           within an element the Gauss points cancel in pairs (+a, -a) or to one ulp
  zeros            +0.0 and -0.0 only, in every sign pattern over the Gauss points of an element
  subnormal        a few units of 2^-1074 of either sign (the divisions by 8 and by the count round)
  huge             +-1.7e308: the element sums overflow to +-Inf, some then meet the other sign
  nan_gp           one Gauss point of one element NaN in stress[0], another element's in eqps
  inf_pair         +Inf and -Inf in one element (same component: NaN; two components: Inf - -Inf)
  mises            eight disjoint elements, every Gauss point of element e the dyadic tensor
                   MISES_KNOWN[e][0]: each operation of the average and of :3477 is exact
"""
from __future__ import annotations

import functools
from collections import namedtuple

import numpy as np

from hakai import mesh
from hakai.model import Model
from util import shuffled, small_bar

Case = namedtuple("Case", "name model stress strain eqps triax flag")

# (stress six-vector, Mises): (2,0,0,0,0,0) -> 2, (1,0,0,1,0,0) -> 2, hydrostatic -> 0, negatives
MISES_KNOWN = (((2., 0., 0., 0., 0., 0.), 2.0), ((1., 0., 0., 1., 0., 0.), 2.0), ((3., 3., 3., 0., 0., 0.), 0.0),
               ((0.5, 0.5, 0.5, 0., 0., 0.), 0.0), ((-2., 0., 0., 0., 0., 0.), 2.0),
               ((-1., 0., 0., -1., 0., 0.), 2.0), ((-3., -3., -3., 0., 0., 0.), 0.0),
               ((0., 0., 0., 0., 0., 0.), 0.0))


def _bar(nx, ny, nz):
    m = small_bar(nx, ny, nz, n_steps=1)
    m.bc = []
    return m


def _with(m: Model, coordmat=None, elementmat=None, name=None) -> Model:
    em = m.elementmat if elementmat is None else elementmat
    return Model(m.coordmat if coordmat is None else coordmat, em, np.ones(em.shape[0], np.int64), m.materials,
                 d_time=m.d_time, end_time=m.end_time, name=name or m.name)


def _unused_last_node(m: Model) -> Model:
    return _with(m, coordmat=np.vstack([m.coordmat, m.coordmat.max(axis=0) + 1.0]), name=m.name + "_unused")


def _duplicated(m: Model) -> Model:
    return _with(m, elementmat=np.repeat(m.elementmat, 2, axis=0), name=m.name + "_dup")


def _disjoint(n: int) -> Model:
    """n unit cubes that share no node."""
    c1, e1 = mesh.hex_bar(1, 1, 1)
    coord = np.concatenate([c1 + np.array([2.0 * i, 0.0, 0.0]) for i in range(n)])
    elem = np.concatenate([e1 + 8 * i for i in range(n)])
    return Model(coord, elem, np.ones(n, np.int64), [mesh.steel_ductile()], name="disjoint")


def _wide(rng, shape):
    """Magnitudes 1e-12 .. 1e8 of either sign, a few +-0."""
    v = rng.standard_normal(shape) * 10.0 ** rng.uniform(-12, 8, shape)
    z = rng.random(shape)
    v[z < 0.02] = 0.0
    v[(z >= 0.02) & (z < 0.04)] = -0.0
    return v


def _random(name, m, seed, flag=None):
    rng = np.random.default_rng(seed)
    nE = m.nElement
    return Case(name, m, _wide(rng, (8 * nE, 6)), _wide(rng, (8 * nE, 6)), np.abs(_wide(rng, 8 * nE)),
                _wide(rng, 8 * nE), np.ones(nE, np.int64) if flag is None else flag)


def _fill(name, m, gen):
    """gen(shape) -> (nE, 8, ...) values; the four arrays get independent draws."""
    nE = m.nElement
    return Case(name, m, gen((nE, 8, 6)).reshape(8 * nE, 6), gen((nE, 8, 6)).reshape(8 * nE, 6),
                gen((nE, 8)).reshape(8 * nE), gen((nE, 8)).reshape(8 * nE), np.ones(nE, np.int64))


@functools.lru_cache(maxsize=None)
def cases() -> tuple:
    out = []
    b8, b255, b256, b513 = _bar(1, 1, 1), _bar(2, 4, 16), _bar(3, 7, 7), _bar(2, 8, 18)
    b257 = _unused_last_node(b256)
    for name, m in (("n8", b8), ("n255", b255), ("n256", b256), ("n257", b257), ("n513", b513)):
        out.append(_random(name, m, len(out) + 1))
    assert [c.model.nNode for c in out] == [8, 255, 256, 257, 513]
    assert [c.model.nElement for c in out] == [1, 128, 147, 147, 288]

    out.append(_random("dup16", _duplicated(b255), 11))
    sh = shuffled(b256, 7)
    out.append(_random("shuffled", _with(sh), 12))
    out.append(_random("shuffled_dup257", _unused_last_node(_duplicated(sh)), 13))

    # deleted elements: zero stress and strain (v2/HAKAI_j.jl:742-746), eqps and triax kept
    c = _random("deleted", b255, 14)
    flag = np.ones(b255.nElement, np.int64)
    flag[::3] = 0
    gp = np.repeat(flag == 0, 8)
    c.stress[gp] = 0.0
    c.strain[gp] = 0.0
    assert np.any(c.eqps[gp] != 0) and np.any(c.triax[gp] != 0)
    out.append(c._replace(flag=flag))

    rng = np.random.default_rng(15)

    def cancel(shape):
        a = rng.standard_normal((shape[0], 4) + shape[2:]) * 10.0 ** rng.uniform(-3, 6, (shape[0], 4) + shape[2:])
        v = np.empty(shape)
        v[:, 0::2] = a
        v[:, 1::2] = -a
        odd = np.arange(shape[0]) % 3 == 1          # one ulp off: the pair leaves a rounding-sized rest
        v[odd, 1] = np.nextafter(v[odd, 1], np.inf)
        swap = np.arange(shape[0]) % 3 == 2         # + + + + - - - -: cancels only at the end
        v[swap] = np.concatenate([v[swap, 0::2], v[swap, 1::2]], axis=1)
        return v
    out.append(_fill("cancel", b256, cancel))

    def zeros(shape):
        e = np.arange(shape[0]).reshape((-1, 1) + (1,) * (len(shape) - 2))
        k = np.arange(8).reshape((1, 8) + (1,) * (len(shape) - 2))
        return np.broadcast_to(np.where((e >> k) & 1, -0.0, 0.0), shape).copy()
    out.append(_fill("zeros", b256, zeros))

    out.append(_fill("subnormal", b256,
                     lambda s: rng.choice([-1.0, 1.0], s) * rng.integers(0, 40, s) * 2.0 ** -1074))

    def huge(shape):
        v = rng.choice([-1.0, 1.0], shape) * 1.7e308
        v[np.arange(shape[0]) % 4 == 0] = 1.7e308   # one sign: +Inf, no NaN
        v[np.arange(shape[0]) % 4 == 1] *= 1e-300   # ordinary neighbours
        return v
    out.append(_fill("huge", b255, huge))

    c = _random("nan_gp", b256, 16)
    c.stress[8 * NAN_ELEMENTS[0] + 3, 0] = np.nan
    c.eqps[8 * NAN_ELEMENTS[1] + 7] = np.nan
    out.append(c)

    c = _random("inf_pair", b256, 17)
    c.strain[8 * INF_ELEMENTS[0] + 0, 1] = np.inf
    c.strain[8 * INF_ELEMENTS[0] + 5, 1] = -np.inf
    c.stress[8 * INF_ELEMENTS[1] + 2, 0] = np.inf
    c.stress[8 * INF_ELEMENTS[1] + 6, 2] = -np.inf
    out.append(c)

    m = _disjoint(len(MISES_KNOWN))
    st = np.repeat(np.array([t for t, _ in MISES_KNOWN]), 8, axis=0)
    out.append(Case("mises", m, st, st[:, ::-1].copy(), np.repeat(np.arange(8.0), 8), np.repeat(-np.arange(8.0), 8),
                    np.ones(m.nElement, np.int64)))
    for c in out:
        for a in (c.stress, c.strain, c.eqps, c.triax):
            a.setflags(write=False)
    return tuple(out)


def contact_deck() -> Model:
    """Plate and impactor with deletions in the contact zone; with 400 steps the outputs come every
    4 steps, and some of them (tests assert it from the oracle's log) land on deletion steps."""
    return mesh.two_body_model(plate=(6, 6, 1), impactor=(2, 2, 3), v=-3e5, d_time=2e-8, n_steps=400)


def mass_scaled_bar() -> Model:
    """A 2 x 3 x 4 ductile bar with an initial velocity ramp and mass_scaling = 4: the stepped d_time
    is twice the deck's increment. end_time holds 200.5 stepped increments, so end_time / d_time
    floors to 200 whatever the division rounds to."""
    m = small_bar(2, 3, 4, v_end=2e5, n_steps=1, d_time=1e-7)
    m.mass_scaling = 4.0
    m.end_time = 200.5 * 2e-7
    m.name = "mass_scaled_bar"
    return m


# 0-based elements of the 3x7x7 bar that hold the non-finite Gauss points (interior and first)
NAN_ELEMENTS = (73, 0)
INF_ELEMENTS = (100, 146)


def case(name: str) -> Case:
    return next(c for c in cases() if c.name == name)


def names() -> tuple:
    return tuple(c.name for c in cases())


def args(c: Case):
    """The arguments of output_ref.node_average / node_average_exact."""
    return c.model.nNode, c.model.elementmat, c.stress, c.strain, c.eqps, c.triax
