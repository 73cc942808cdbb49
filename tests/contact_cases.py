"""Crafted contact states for the contact-force probes (tests/test_contact_edges_cpu.py on the CPU,
tests/test_gpu_contact_edges.py on the device). Plain module, shared by both so that the CPU test
pins exactly the decks and states the device test probes.

mixed_two_body: a plate of unit cubes under an impactor of cubes of edge h (a power of two below
one), already pen deep in the plate's top face. The fine impactor puts many i-nodes into one cell of
a plate triangle (more than the four events a search thread keeps in registers), and the contact
constants differ from the reference's defaults, so the damping term and the stiffness factors are
live. Every number is a dyadic rational: coord + disp, the shifts and every difference the contact
expressions form are exact in double.

The sweeps (SWEEPS) place one impactor node on a decision boundary of the contact test and a few
ulps to either side; the reference decides each point.
"""
from __future__ import annotations

import math

import numpy as np

from hakai import mesh
from hakai.model import Model

PARAMS = (0.25, 1.5, 0.75, 0.125, 0.25)


def mixed_two_body(plate=(3, 3, 1), imp=(8, 8, 2), h=0.25, pen=1 / 32, off=(1 / 16, 1 / 32), params=PARAMS,
                   flag=1, one_instance=False, shift=(0, 0, 0)) -> Model:
    px, py, pz = plate
    ix, iy, iz = imp
    c1, e1 = mesh.hex_bar(px, py, pz)
    c2, e2 = mesh.hex_bar(ix, iy, iz, h=h)
    c2[:, 0] += (px - ix * h) / 2.0 + off[0]
    c2[:, 1] += (py - iy * h) / 2.0 + off[1]
    c2[:, 2] += pz - pen
    n1 = c1.shape[0]
    coord = np.concatenate([c1, c2]) + np.asarray(shift, np.float64)
    elem = np.concatenate([e1, e2 + n1])
    inst = np.concatenate([np.ones(e1.shape[0], np.int64),
                           np.full(e2.shape[0], 1 if one_instance else 2, np.int64)])
    imp_nodes = np.arange(n1 + 1, coord.shape[0] + 1, dtype=np.int64)
    return Model(coord, elem, np.ones(elem.shape[0], np.int64), [mesh.steel_ductile()],
                 bc=[mesh.encastre(mesh.plane_nodes(px, py, 0))], ic_dofs=imp_nodes * 3,
                 ic_values=np.full(imp_nodes.shape[0], -1e4), contact_flag=flag, element_instance=inst,
                 name="mixed_two_body", contact_params=tuple(float(x) for x in params) if params else None)


def n_plate_nodes(plate=(3, 3, 1)) -> int:
    return (plate[0] + 1) * (plate[1] + 1) * (plate[2] + 1)


def imp_node(plate, imp, ix, iy, iz) -> int:
    """0-based id of impactor node (ix, iy, iz) of mixed_two_body(plate, imp)."""
    return n_plate_nodes(plate) + mesh.node_id(ix, iy, iz, imp[0], imp[1]) - 1


def noisy_velocity(model, seed=0):
    """The model's initial velocity plus dyadic noise on every dof: relative velocity, friction
    direction and damping are nonzero and differ from event to event."""
    v = np.zeros(3 * model.nNode)
    v[model.ic_dofs - 1] = model.ic_values
    rng = np.random.default_rng(seed)
    return v + rng.integers(-8, 8, size=v.shape) * 128.0


def set_state(o, position=None, velo=None):
    """Write a crafted position (nN, 3) / velocity into an oracle's state, consistently: disp is
    position - coord (exact for the dyadic decks) and disp_pre the step before at that velocity."""
    s = o.s
    if velo is not None:
        s["velo"][:] = velo
    if position is not None:
        s["position"][:] = position
        s["disp"][:] = (position - o.m.coordmat).ravel()
    s["disp_pre"][:] = s["disp"] - s["velo"] * o.m.dt


def ulps(x, k):
    """x moved k units in the last place (k of either sign)."""
    x = float(x)
    for _ in range(abs(k)):
        x = float(np.nextafter(x, math.inf if k > 0 else -math.inf))
    return x


def realised(model, position):
    """The position the device forms from an uploaded state, coord + (position - coord): equal to
    `position` wherever the node stays within a factor two of its coordinate (or is dyadic), and the
    nearest realisable point elsewhere. Every reference is evaluated at this position."""
    return model.coordmat + (position - model.coordmat)


# ---- decision-boundary sweeps on the default 137-hex deck ---------------------------------------
# Geometry (plate 3x3x1 of unit cubes, top face z = 1; impactor 8x8x2 of edge 1/4, bottom face at
# z = 1 - pen): min_size = 1/4, d_lim = 0.3 * min_size, max_size = 1, ddiv = 1.1. Pair 0 is
# (i: plate nodes, j: impactor triangles), pair 1 (i: impactor nodes, j: plate triangles). A plate
# top quad [a, a+1] x [b, b+1] is cut along its (a, b)-(a+1, b+1) diagonal, and a triangle's first
# node q0 is one end of that diagonal. One impactor bottom node, the probe, is moved; each sweep
# returns (model, probe node (0-based), [(label, position (nN, 3))]). tests/test_contact_edges_cpu.py
# requires that the probe's set of events (pair, triangle) is not the same at every point of a
# sweep: the boundary is crossed.
PLATE, IMP = (3, 3, 1), (8, 8, 2)
PROBE = (3, 4, 0)  # impactor bottom node at (1.3125, 1.53125): inside the quad [1,2]^2, upper triangle


def _plate_top(ix, iy):
    return mesh.node_id(ix, iy, 1, 3, 3) - 1


def _sweep(m, pos, k, axis, x0, us, name):
    out = []
    for u in us:
        p = pos.copy()
        p[k, axis] = ulps(x0, u)
        out.append((f"{name}{u:+d}", realised(m, p)))
    return out


def sweep_d_lim():
    """Depth d through d_lim = 0.3 * min_size, +-4 ulps. The deck is shifted by -1 in z, so the
    plate's top face is z = 0 and the probe at z = -d_lim has d == d_lim exactly (accepted); one
    ulp deeper it is rejected."""
    m = mixed_two_body(shift=(0, 0, -1))
    k = imp_node(PLATE, IMP, *PROBE)
    return m, k, _sweep(m, m.coordmat, k, 2, -(0.25 * 0.3), range(-4, 5), "d_lim")


def sweep_d_zero():
    """Depth through 0 (d > 0): the node on the plate's top face and +-4 ulps."""
    m = mixed_two_body()
    k = imp_node(PLATE, IMP, *PROBE)
    return m, k, _sweep(m, m.coordmat, k, 2, 1.0, range(-4, 5), "d_zero")


def sweep_edges():
    """off = (0, 0): the impactor's x/y grid (multiples of 1/4) lies on plate triangle edges
    (x1 == 0, x2 == 0), vertices and the quads' diagonals (x1 + x2 == 1) exactly. The probe starts on
    the plate vertex (1, 1) and is moved 1 ulp across the plate edge, then onto a diagonal and an
    edge and 1 ulp across each."""
    m = mixed_two_body(off=(0.0, 0.0))
    k = imp_node(PLATE, IMP, 2, 2, 0)
    pos = m.coordmat
    assert pos[k, 0] == 1.0 and pos[k, 1] == 1.0
    out = [("grid", pos.copy())]
    out += _sweep(m, pos, k, 0, 1.0, (-1, 1), "vertex_x")
    p = pos.copy()
    p[k, 0] = 1.25
    out += _sweep(m, p, k, 1, 1.25, (-1, 0, 1), "diagonal_y")
    p = pos.copy()
    p[k, 0] = 1.5
    out += _sweep(m, p, k, 1, 1.0, (-1, 0, 1), "edge_y")
    return m, k, out


def sweep_range_box():
    """The probe's x on the range-box bound rmx_x of its pair exactly, and +-1, 2 ulps. The bound must
    come from the OTHER body for the node test to decide anything, and the point must otherwise be
    an event: one far impactor top node is moved to x = 4, so the overlap box ends at the plate's own
    x = 3, and the plate's top nodes at x = 3 are raised by 1/4, so the last column's triangles lean
    (normal towards -x) and a point just past x = 3, below that surface, still projects into the
    triangle along the normal."""
    m = mixed_two_body()
    k = imp_node(PLATE, IMP, *PROBE)
    pos = m.coordmat.copy()
    pos[imp_node(PLATE, IMP, 8, 8, 2), 0] = 4.0
    for iy in range(4):
        pos[_plate_top(3, iy), 2] = 1.25
    pos[k, 1] = 1.53125
    pos[k, 2] = 1.25 - 1 / 32
    return m, k, _sweep(m, pos, k, 0, 3.0, (-2, -1, 0, 1, 2), "rmx_x")


def sweep_cell():
    """The probe across a cell boundary where that decides: (p - amn) / ddiv an exact integer, and
    +-1..3 units of 2^-52 in p (the spacing of coord + disp there). A node lies in cell m when
    ceil((p - amn) / ddiv) == m. The plate top node (1, 1), first node of the triangle
    (1,1)-(2,1)-(2,2), is moved in the plane to x = -1 = amn_x (cell 0), which stretches the
    triangle over three cells; the probe at x = fl(1.1) - 1 (exact) has p - amn == ddiv, so
    (p - amn) / ddiv == 1 exactly: cell 1, a neighbour of cell 0, while one step above it is in
    cell 2 and no candidate of that triangle any more."""
    m = mixed_two_body()
    k = imp_node(PLATE, IMP, *PROBE)
    ddiv = 1.0 * 1.1
    pos = m.coordmat.copy()
    pos[_plate_top(1, 1), 0] = -1.0
    pos[k, 1] = 1.25
    x0 = ddiv - 1.0
    out = []
    for u in range(-3, 4):
        p = pos.copy()
        p[k, 0] = x0 + u * 2.0 ** -52
        out.append((f"cell_x{u:+d}", realised(m, p)))
        assert out[-1][1][k, 0] == p[k, 0]
    return m, k, out


def sweep_sphere():
    """The probe on the bounding sphere, dpc == Rmax exactly, of the triangle (1,1)-(2,1)-(2,2) and
    +-3 ulps of its x: inside the triangle next to its far vertex (1, 1), where the depth alone
    lifts |p - c| over Rmax. The point is searched with the reference's own expressions: x is
    bisected on the line y = 1 + 2^-12, z = 1 - pen until my3norm(p - c) < Rmax changes, then the
    neighbouring doubles in x and y are tried until the rounded norm equals Rmax (a step of x moves
    the radicand by more than one of its ulps, a step of y by about one)."""
    m = mixed_two_body()
    k = imp_node(PLATE, IMP, *PROBE)
    q = [[1.0, 1.0, 1.0], [2.0, 1.0, 1.0], [2.0, 2.0, 1.0]]
    c = [(q[0][d] + q[1][d] + q[2][d]) / 3.0 for d in range(3)]
    norm = lambda a, b, cc: math.sqrt(a * a + b * b + cc * cc)  # noqa: E731
    Rmax = max(norm(*(v[d] - c[d] for d in range(3))) for v in q)
    pos = m.coordmat.copy()
    y0, z = 1.0 + 2.0 ** -12, pos[k, 2]
    dpc = lambda x, y: norm(x - c[0], y - c[1], z - c[2])  # noqa: E731
    lo, hi = y0, 1.25  # inside the triangle (x >= y); dpc(lo) >= Rmax > dpc(hi)
    assert dpc(lo, y0) >= Rmax > dpc(hi, y0)
    while ulps(lo, 1) < hi:
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if dpc(mid, y0) >= Rmax else (lo, mid)
    hit = next(((ulps(hi, i), ulps(y0, j)) for j in range(64) for i in range(-8, 9)
                if dpc(ulps(hi, i), ulps(y0, j)) == Rmax), None)
    assert hit is not None, "no double on the sphere near the crossing"
    pos[k, 1] = hit[1]
    return m, k, _sweep(m, pos, k, 0, hit[0], range(-3, 4), "sphere")


SWEEPS = {"d_lim": sweep_d_lim, "d_zero": sweep_d_zero, "edges": sweep_edges, "range_box": sweep_range_box,
          "cell": sweep_cell, "sphere": sweep_sphere}


def degenerate_plate():
    """Zero-area triangles: plate top node (1, 1) moved onto its +x neighbour (2, 1) through disp, so
    each top triangle that holds both has two equal vertices: mag_n == 0, a NaN normal, no event.
    Returns (model, position, the two nodes (0-based))."""
    m = mixed_two_body()
    pos = m.coordmat.copy()
    a, b = _plate_top(1, 1), _plate_top(2, 1)
    pos[a] = pos[b]
    return m, realised(m, pos), (a, b)


# ---- the decks of the GPU probes: name -> builder arguments --------------------------------------
SMALL_DECKS = {
    "h4": dict(),                                           # 137 hex, 85 events, 6 per search thread
    "h4_flag2": dict(flag=2),
    "h8": dict(imp=(16, 16, 2), h=0.125, pen=1 / 64),       # 521 hex, 293 events, 28 per thread
    "small": dict(plate=(2, 2, 1), imp=(4, 4, 1)),          # 20 hex, 26 events
    "self": dict(one_instance=True),                        # one self pair, 60 events, 5 per thread
}
LARGE = dict(plate=(64, 64, 1), imp=(16, 16, 2), h=0.125, pen=1 / 64)   # 4608 hex: the large-deck search
SHIFTS = [(2.0 ** 20, -2.0 ** 20, 2.0 ** 10), (-2.0 ** 30, 2.0 ** 30, 2.0 ** 30)]
