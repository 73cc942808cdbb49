"""Restatement of the rigid walls (hakai_set_walls) in NumPy -- TEST INFRASTRUCTURE ONLY.

Written from the formulas of include/hakai_hip.h ("rigid walls"), with the operation order of
csrc/hakai_walls_node.hpp, one IEEE double operation per operation:

  normalise    n = normal / sqrt((nx*nx + ny*ny) + nz*nz), each component divided
  frame        o = origin + motion * s0, vw = motion * ((s0 - sm) / dt)
  gap          g = ((x0 - o0) * n0 + (x1 - o1) * n1) + (x2 - o2) * n2, x = coord + u
  node_force   the force of one wall on penetrating nodes (d = -g > 0), vectorised over the nodes
  wall_force   the node sums: a start value (or +0.0) plus the walls in ascending index, a wall adding
               only where its mask bit is set and d > 0 (strictly)
  masks        the planner's per-node membership masks
  valid        the planner's validation: what hakai_set_walls accepts
  *_hp         the same pieces in 60-digit decimal arithmetic (as tests/hp_ref.py)

Rounding bounds against the 60-digit evaluation (u = 2^-53, first order in u, every input double
taken as given; the constants count the operations of the definition, they are not fitted; underflow is
outside the bounds: the tests use values of ordinary size).

frame: o[c] has one product and one sum: |do| <= u |motion s0| + u (|origin| + |motion s0|)
  <= 2 u (|origin[c]| + |motion[c] s0|). rate = (s0 - sm) / dt has two roundings and vw one more:
  |dvw| <= 3 u |vw|.
gap (GAP_COUNT = 9): with X = max_c (|coord[c]| + |u[c]| + |o[c]|): x = coord + u errs by u X, x - o by
  another u X on top, the product with n[c] adds u X |n[c]|: 3 u X |n[c]| per term, and sum_c |n[c]| <=
  sqrt(3) for a unit normal, 5.2 u X; the two additions round values <= sqrt(3) X, 3.5 u X. 8.7 u X.
force (node_force_bound): with V = max_c (|(u - um) / dt| + |vw[c]|), k, cd, d as computed,
  Nmax = k d + 2 cd V (>= |k d - cd vn| since |vn| <= sqrt(3) V) and mdt = m / dt:
  v[c]   a difference, a quotient and a difference: |dv| <= 3 u V
  k      dt*dt, m / ., scale * ., + : no cancellation (all terms >= 0), relative 4 u
  vn     three products (3 u V + u V each, times |n[c]|, summed: 4 sqrt(3) u V = 6.93 u V) and two
         sums of values <= sqrt(3) V (3.47 u V): |dvn| <= 10.4 u V <= 11 u V
  cd     2 zeta exact, m * k relative 5 u, the root halves it and rounds, the product rounds:
         relative 4.5 u
  k d    relative 5 u;  cd vn: 4.5 u cd sqrt(3) V + 11 u cd V + u cd sqrt(3) V = 20.6 u cd V
  Nr     the difference rounds a value <= k d + sqrt(3) cd V: |dN| <= u EN, EN = 6 k d + 23 cd V
         (max(., 0) is 1-Lipschitz)
  vt[c]  vn * n[c] errs 11 u V + 1.74 u V, the difference rounds a value <= 2.74 V, plus dv:
         |dvt| <= 18.5 u V <= 19 u V
  s      the norm is 1-Lipschitz in vt (sqrt(3) 19 u V = 33 u V); its own roundings (squares, two sums:
         relative 3 u, halved by the root, plus the root's) 2.5 u s <= 4.4 u V: |ds| <= 38 u V
  T / s * vt[c]   T = min(mu N, m s / dt) is 1-Lipschitz in both arguments:
         |dT| <= max(mu u EN + u mu N, mdt 38 u V + 2 u T). The direction vt[c] / s errs by
         (19 + 38) u V / s, and T / s <= mdt in BOTH branches (that is what the min is for), so the
         direction contributes 57 u mdt V however small s is; the quotient and the product round a
         value <= T <= mu Nmax twice. Sum: u (mu EN + 5 mu Nmax + 95 mdt V)
  N n[c] u EN + u Nmax;  the final difference rounds a value <= (1 + mu) Nmax.
  Per component: |dF| <= u ((1 + mu) EN + (2 + 6 mu) Nmax + 95 mdt V).
"""
from __future__ import annotations

from decimal import Decimal, localcontext

import numpy as np

from loads_ref import amp_value

PREC = 60
GAP_COUNT = 9
U = 2.0 ** -53
MAX_WALLS = 32


def normalise(normal):
    """(n, length) of one normal (3,), the planner's operation order."""
    with np.errstate(all="ignore"):
        a = [np.float64(v) for v in normal]
        ln = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
        return np.array([a[0] / ln, a[1] / ln, a[2] / ln], np.float64), ln


def amp_of(walls, table, ct):
    if table < 0:
        return np.float64(1.0)
    t, v = walls.amps[table]
    with np.errstate(all="ignore"):
        return np.float64(amp_value(t, v, ct))


def frame(origin, motion, s0, sm, dt):
    """(o, vw) of one wall from the two amplitude values."""
    with np.errstate(all="ignore"):
        origin, motion = np.asarray(origin, np.float64), np.asarray(motion, np.float64)
        s0, sm, dt = np.float64(s0), np.float64(sm), np.float64(dt)
        rate = (s0 - sm) / dt
        return origin + motion * s0, motion * rate


def wall_frame(walls, w, t, d_time):
    """Wall w's frame at step t: tau0 = (t - 1.0) * d_time, taum = (t - 2.0) * d_time."""
    t, dt = np.float64(t), np.float64(d_time)
    tau0, taum = (t - np.float64(1.0)) * dt, (t - np.float64(2.0)) * dt
    a = int(walls.amp[w])
    return frame(walls.origin[w], walls.motion[w], amp_of(walls, a, tau0), amp_of(walls, a, taum), dt)


def gap(coord, u, o, n):
    """g of every node: coord, u (nN, 3); o, n (3,)."""
    with np.errstate(all="ignore"):
        a = [((coord[:, c] + u[:, c]) - o[c]) * n[c] for c in range(3)]
        return (a[0] + a[1]) + a[2]


def node_force(d, u, um, m, dt, vw, n, stiffness, scale, zeta, mu):
    """F (nN, 3) of one wall for penetrations d (nN,) -- meaningful where d > 0."""
    with np.errstate(all="ignore"):
        dt = np.float64(dt)
        v = [(u[:, c] - um[:, c]) / dt - vw[c] for c in range(3)]
        k = np.float64(stiffness) + np.float64(scale) * (m / (dt * dt))
        vn = (v[0] * n[0] + v[1] * n[1]) + v[2] * n[2]
        cd = (np.float64(2.0) * np.float64(zeta)) * np.sqrt(m * k)
        Nr = k * d - cd * vn
        N = np.where(Nr > 0.0, Nr, 0.0)
        vt = [v[c] - vn * n[c] for c in range(3)]
        s = np.sqrt((vt[0] * vt[0] + vt[1] * vt[1]) + vt[2] * vt[2])
        Ta, Tb = np.float64(mu) * N, (m * s) / dt
        T = np.where(Ta < Tb, Ta, Tb)
        r = T / s
        return np.stack([np.where(s > 0.0, N * n[c] - r * vt[c], N * n[c]) for c in range(3)], axis=1)


def masks(n_node, walls):
    """The planner's masks (uint32 per node), or None when every wall takes every node."""
    if all(len(x) == 0 for x in walls.nodes):
        return None
    mask = np.zeros(n_node, np.uint32)
    for w, nodes in enumerate(walls.nodes):
        if len(nodes) == 0:
            mask |= np.uint32(1 << w)
        else:
            mask[np.asarray(nodes) - 1] |= np.uint32(1 << w)
    return mask


def valid(n_node, walls, n_wall=None):
    """What the planner accepts (the header's list of refusals, restated)."""
    n_wall = walls.n_wall if n_wall is None else n_wall
    if n_wall < 0 or n_wall > MAX_WALLS:
        return False
    for t, v in walls.amps:
        if len(t) < 2 or not (np.all(np.isfinite(t)) and np.all(np.isfinite(v))):
            return False
    for w in range(n_wall):
        if not -1 <= int(walls.amp[w]) < len(walls.amps):
            return False
        if not (np.all(np.isfinite(walls.origin[w])) and np.all(np.isfinite(walls.motion[w]))
                and np.all(np.isfinite(walls.normal[w]))):
            return False
        ln = normalise(walls.normal[w])[1]
        if not (ln > 0.0 and np.isfinite(ln)):
            return False
        for p in (walls.stiffness[w], walls.scale[w], walls.damping[w], walls.friction[w]):
            if not (np.isfinite(p) and p >= 0.0):
                return False
        if len(walls.nodes[w]) and (np.min(walls.nodes[w]) < 1 or np.max(walls.nodes[w]) > n_node):
            return False
    return True


def wall_force(model, walls, diag_M, disp, disp_pre, t, d_time, f=None, reverse=False):
    """The wall force (3nN) of step t at the state (disp, disp_pre): f (the sum so far: contact, loads;
    or +0.0) plus the walls in ascending index (reverse: descending, to show the order matters),
    every addition rounded once."""
    nN = model.nNode
    out = (np.zeros(3 * nN) if f is None else np.array(f, np.float64)).reshape(nN, 3)
    coord = np.asarray(model.coordmat, np.float64)
    u = np.asarray(disp, np.float64).reshape(nN, 3)
    um = np.asarray(disp_pre, np.float64).reshape(nN, 3)
    m = np.ascontiguousarray(np.asarray(diag_M, np.float64)[0::3])
    mk = masks(nN, walls)
    order = range(walls.n_wall - 1, -1, -1) if reverse else range(walls.n_wall)
    with np.errstate(all="ignore"):
        for w in order:
            n, _ = normalise(walls.normal[w])
            o, vw = wall_frame(walls, w, t, d_time)
            d = -gap(coord, u, o, n)
            act = d > 0.0
            if mk is not None:
                act &= ((mk >> np.uint32(w)) & np.uint32(1)).astype(bool)
            F = node_force(d, u, um, m, d_time, vw, n, walls.stiffness[w], walls.scale[w], walls.damping[w],
                           walls.friction[w])
            out[act] = out[act] + F[act]
    return out.reshape(-1)


# ---- 60-digit decimal arithmetic -------------------------------------------------------------------------

def _D(x):
    return Decimal(float(x))


def frame_hp(origin, motion, s0, sm, dt):
    with localcontext() as ctx:
        ctx.prec = PREC
        rate = (_D(s0) - _D(sm)) / _D(dt)
        return [_D(origin[c]) + _D(motion[c]) * _D(s0) for c in range(3)], [_D(motion[c]) * rate for c in range(3)]


def gap_hp(coord, u, o, n):
    with localcontext() as ctx:
        ctx.prec = PREC
        return sum(((_D(coord[c]) + _D(u[c])) - _D(o[c])) * _D(n[c]) for c in range(3))


def node_force_hp(d, u, um, m, dt, vw, n, stiffness, scale, zeta, mu):
    """One node, every input a double taken exactly."""
    with localcontext() as ctx:
        ctx.prec = PREC
        d, m, dt = _D(d), _D(m), _D(dt)
        n = [_D(x) for x in n]
        v = [(_D(u[c]) - _D(um[c])) / dt - _D(vw[c]) for c in range(3)]
        k = _D(stiffness) + _D(scale) * (m / (dt * dt))
        vn = sum(v[c] * n[c] for c in range(3))
        cd = 2 * _D(zeta) * (m * k).sqrt()
        N = max(k * d - cd * vn, Decimal(0))
        vt = [v[c] - vn * n[c] for c in range(3)]
        s = sum(x * x for x in vt).sqrt()
        T = min(_D(mu) * N, m * s / dt)
        if s > 0:
            return [N * n[c] - T / s * vt[c] for c in range(3)]
        return [N * n[c] for c in range(3)]


def node_force_bound(d, u, um, m, dt, vw, stiffness, scale, zeta, mu):
    """|node_force - node_force_hp| <= this per component (module docstring), as a float (the bound
    itself is evaluated in doubles and padded by 1e-9 of itself for that)."""
    V = max(abs((u[c] - um[c]) / dt) + abs(vw[c]) for c in range(3))
    k = stiffness + scale * (m / (dt * dt))
    cd = 2.0 * zeta * np.sqrt(m * k)
    EN = 6.0 * k * d + 23.0 * cd * V
    Nmax = k * d + 2.0 * cd * V
    return U * ((1.0 + mu) * EN + (2.0 + 6.0 * mu) * Nmax + 95.0 * (m / dt) * V) * (1.0 + 1e-9)
