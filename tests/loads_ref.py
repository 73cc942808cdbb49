"""Restatement of the external loads (hakai_set_loads) in NumPy -- TEST INFRASTRUCTURE ONLY.

Written from the formulas of include/hakai_hip.h ("external loads"), with the operation order of
csrc/hakai_loads_face.hpp, one IEEE double operation per operation:

  amp_value          the amplitude rule (first matching segment, the first one extrapolated)
  face_corners       the four consistent nodal forces F_a of a bilinear pressure face
  face_exact         the same in exact rationals (fractions.Fraction), no rounding at all
  load_force         the node sums in their fixed order: contact force (or +0.0), concentrated entries
                     in list order, gravity entries in list order, pressure contributions in ascending
                     order of the entry index
  plan               the per-node lists the host planner builds (what k_loads gathers)

Rounding bound of face_corners against face_exact (FACE_COUNT)
-------------------------------------------------------------
Let D be the largest |x_i[c] - x_j[c]| over the face's corners and components, u = 2^-53, pa = p * amp
taken as given (its one rounding belongs to the caller). First order in u:
  g1, g2, h   ((a - b) + (c - d)) * 0.25: two differences and one sum, each relative u, the scaling
              exact: |dg| <= 2u (|a - b| + |c - d|) / 4 <= u D, and |g| <= D / 2.
  a cross component  a1 b2 - a2 b1: each product carries the operands' errors, 2 (u D)(D / 2) = u D^2,
              and its own rounding u D^2 / 4; the difference rounds once more, u D^2 / 2:
              |dn| <= 2 (1.25 u D^2) + 0.5 u D^2 = 3 u D^2, and |n| <= D^2 / 2.
  s * n       s = +-fl(1/3) (relative u): 3 u D^2 / 3 + 2 u (D^2 / 6) = 1.34 u D^2, |s n| <= D^2 / 6.
  the two sums       magnitudes <= 2 D^2 / 3 and 5 D^2 / 6: roundings 0.67 u D^2 and 0.84 u D^2.
  pa * (...)  one more rounding of a value <= 5 D^2 / 6 |pa|.
Total (3 + 2 * 1.34 + 0.67 + 0.84 + 0.84) u |pa| D^2 = 8.03 u |pa| D^2. FACE_COUNT = 9 covers it and
the second-order terms (below 100 u^2); it counts operations, it is not fitted. Underflow is outside
the bound: the tests use coordinates of ordinary size.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

# S1..S6 as 0-based elementmat columns, corners (xi, eta) = (-,-), (+,-), (+,+), (-,+)
FACE_NODES = ((0, 1, 2, 3), (4, 7, 6, 5), (0, 4, 5, 1), (1, 5, 6, 2), (2, 6, 7, 3), (3, 7, 4, 0))
XI = (-1, 1, 1, -1)
ETA = (-1, -1, 1, 1)
FACE_COUNT = 9
U = Fraction(1, 2 ** 53)


def amp_value(a_t, a_v, ct):
    a_t = [float(x) for x in a_t]
    a_v = [float(x) for x in a_v]
    ct = float(ct)
    ti = 0
    for j in range(len(a_t) - 1):
        if a_t[j] <= ct <= a_t[j + 1]:
            ti = j
            break
    return a_v[ti] + (a_v[ti + 1] - a_v[ti]) * (ct - a_t[ti]) / (a_t[ti + 1] - a_t[ti])


def amp_of(loads, table, ct):
    if table < 0:
        return 1.0
    t, v = loads.amps[table]
    return amp_value(t, v, ct)


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _face(x, pa, third, quarter):
    x0, x1, x2, x3 = x
    g1 = [((x1[c] - x0[c]) + (x2[c] - x3[c])) * quarter for c in range(3)]
    g2 = [((x3[c] - x0[c]) + (x2[c] - x1[c])) * quarter for c in range(3)]
    h = [((x0[c] - x1[c]) + (x2[c] - x3[c])) * quarter for c in range(3)]
    n0, n1, n2 = _cross(g1, g2), _cross(g1, h), _cross(h, g2)
    out = []
    for a in range(4):
        sx, sy = XI[a] * third, ETA[a] * third
        out.append([pa * ((n0[c] + sx * n1[c]) + sy * n2[c]) for c in range(3)])
    return out


def face_corners(x, pa):
    """F_a, a = 0..3, of the face with corners x (4, 3) under pa = p * amp: (4, 3) doubles."""
    with np.errstate(all="ignore"):
        xs = [[np.float64(v) for v in row] for row in np.asarray(x, np.float64)]
        return np.array(_face(xs, np.float64(pa), np.float64(1.0) / np.float64(3.0), np.float64(0.25)), np.float64)


def face_exact(x, pa):
    """The same in exact rationals: 4 x 3 Fractions."""
    xs = [[Fraction(float(v)) for v in row] for row in np.asarray(x, np.float64)]
    return _face(xs, Fraction(float(pa)), Fraction(1, 3), Fraction(1, 4))


def face_bound(x, pa):
    """|face_corners - face_exact| <= this, per component (module docstring)."""
    x = np.asarray(x, np.float64)
    D = max(Fraction(float(abs(x[i, c] - x[j, c]))) for i in range(4) for j in range(4) for c in range(3))
    D = D * (1 + U)  # (the difference above was itself rounded)
    return FACE_COUNT * U * abs(Fraction(float(pa))) * D * D


def load_force(model, loads, diag_M, disp, element_flag, ct, fc=None):
    """The total external force (3nN) of a step at time ct: fc (the contact force, or +0.0) plus the
    loads, every addition rounded once, in the order the header fixes."""
    nN = model.nNode
    f = np.zeros(3 * nN) if fc is None else np.array(fc, np.float64)
    mass = np.asarray(diag_M, np.float64)[0::3]
    with np.errstate(all="ignore"):
        for d, v, a in zip(loads.cload_dof, loads.cload_value, loads.cload_amp):
            f[d - 1] = f[d - 1] + np.float64(v) * np.float64(amp_of(loads, int(a), ct))
        for acc, a in zip(loads.grav_accel, loads.grav_amp):
            amp = np.float64(amp_of(loads, int(a), ct))
            for c in range(3):
                f[c::3] = f[c::3] + mass * (np.float64(acc[c]) * amp)
        x = np.asarray(model.coordmat, np.float64) + np.asarray(disp, np.float64).reshape(nN, 3)
        for e, face, p, a in zip(loads.press_elem, loads.press_face, loads.press_value, loads.press_amp):
            if element_flag[e - 1] != 1:
                continue
            nodes = model.elementmat[e - 1][list(FACE_NODES[face - 1])] - 1
            F = face_corners(x[nodes], np.float64(p) * np.float64(amp_of(loads, int(a), ct)))
            for q in range(4):
                for c in range(3):
                    f[3 * nodes[q] + c] = f[3 * nodes[q] + c] + F[q, c]
    return f


def plan(model, loads):
    """The planner's per-node lists: (cl_ptr, cl_comp, cl_amp, cl_val, pr_ptr, pr_ent), 0-based;
    concentrated entries grouped by node in list order, pressure pairs 4 * entry + corner per node in
    ascending order. Empty arrays where a kind has no entry."""
    nN = model.nNode
    e = np.zeros(0, np.int32)
    cl = (e, e, e, np.zeros(0))
    if len(loads.cload_dof):
        node = (loads.cload_dof - 1) // 3
        order = np.argsort(node, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=nN))]).astype(np.int32)
        cl = (ptr, ((loads.cload_dof - 1) % 3)[order].astype(np.int32), loads.cload_amp[order].astype(np.int32),
              loads.cload_value[order])
    pr = (e, e)
    if len(loads.press_elem):
        node, ent = [], []
        for k, (el, face) in enumerate(zip(loads.press_elem, loads.press_face)):
            for a in range(4):
                node.append(model.elementmat[el - 1][FACE_NODES[face - 1][a]] - 1)
                ent.append(4 * k + a)
        node, ent = np.array(node), np.array(ent, np.int32)
        order = np.argsort(node, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(node, minlength=nN))]).astype(np.int32)
        pr = (ptr, ent[order])
    return cl + pr
