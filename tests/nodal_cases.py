"""Crafted inputs for the nodal update, the boundary conditions and the amplitudes
(tests/test_nodal_bc_cpu.py on the CPU, tests/test_gpu_nodal_bc.py on the device). Plain module,
shared by both so that the CPU test pins exactly the decks and operands the device test runs.

bc_deck: a small_bar whose *Boundary groups exercise every rule of v2/HAKAI_j.jl:585-617. Breakpoints
are T(k) = float64(k) * d_time, the very product the time loop forms (t * d_time), so step k lies on
breakpoint k bit for bit. Groups, in order:

  0 ENCASTRE   bottom plane, x, y and z as three entries
  (ROLLERS     bc_deck_wide only: x on the x faces, y on the y faces, no amplitude)
  1 TOP        z of the top plane; T(5) T(20) T(20) T(40) -> 0 1 .5 .25: starts late, a vertical
               step, ends before the run does
  2 MID        x of the middle plane = 0, y of three of its nodes = 1e-4, no amplitude
  3 ZIGZAG     z of the first four top nodes, then again of the first two with another value, in the
               same group; T(2) T(30) T(12) T(60) T(70) -> 0 1 -1 2 0: non-monotonic (segments 0 and
               2 both hold T(12)..T(30), the first wins), overlaps TOP
  4 PIN        z of top nodes 2-3 = 0, no amplitude: overwrites part of ZIGZAG
  5 COLUMN     y of the side column (0, 1, iz), every layer; T(3) T(10) T(25) -> 1 0 3. Overwrites
               ENCASTRE's y at the bottom and MID's y in the middle plane
  6 ZERO       value 0.0 on otherwise free dofs; T(4) T(16) T(50) -> 1 -1 -2: 0.0 * amp is -0.0
               once the amplitude is negative

Every table starts after step 1 and ends before step 80, so each sees a time before its first
point and one after its last (both extrapolate the FIRST segment). check_deck() proves that no
case is vacuous; tests/test_nodal_bc_cpu.py asserts it.

probe_states / probe_bars: one-step operand sets for the uploaded-Q path of k_nodal on 1 x 1 x nz
bars whose block counts straddle xcd_remap_rev's switch at 16 blocks and its remainder branch.
"""
from __future__ import annotations

import numpy as np

import nodal_ref as R
from hakai import mesh
from hakai.model import BCGroup, Model
from util import small_bar

D_TIME = 1e-7
N_STEPS = 80
CHECK_STEPS = (4, 20, 40, 41, 80)
GROUPS = ("ENCASTRE", "TOP", "MID", "ZIGZAG", "PIN", "COLUMN", "ZERO")


def T(k) -> float:
    """Breakpoint k: the product t * d_time the time loop forms at step k."""
    return float(np.float64(k) * np.float64(D_TIME))


def _x(n):
    return np.asarray(n, np.int64) * 3 - 2


def _y(n):
    return np.asarray(n, np.int64) * 3 - 1


def _z(n):
    return np.asarray(n, np.int64) * 3


def _tab(ks, vs):
    return np.array([T(k) for k in ks]), np.array(vs, np.float64)


def bc_deck(nx=3, ny=2, nz=6, rollers=False) -> Model:
    m = small_bar(nx, ny, nz, v_end=2e4, n_steps=N_STEPS, d_time=D_TIME)
    nid = lambda ix, iy, iz: mesh.node_id(ix, iy, iz, nx, ny)  # noqa: E731
    bottom, top = mesh.plane_nodes(nx, ny, 0), mesh.plane_nodes(nx, ny, nz)
    km = nz // 2
    mid = mesh.plane_nodes(nx, ny, km)
    col = np.array([nid(0, 1, k) for k in range(nz + 1)], np.int64)
    bc = [BCGroup([(_x(bottom), 0.0), (_y(bottom), 0.0), (_z(bottom), 0.0)])]
    if rollers:
        n1 = np.arange(1, m.nNode + 1, dtype=np.int64)
        ix = (n1 - 1) % (nx + 1)
        iy = ((n1 - 1) // (nx + 1)) % (ny + 1)
        bc.append(BCGroup([(_x(n1[(ix == 0) | (ix == nx)]), 0.0), (_y(n1[(iy == 0) | (iy == ny)]), 0.0)]))
    bc.append(BCGroup([(_z(top), 0.02)], *_tab((5, 20, 20, 40), (0, 1, .5, .25))))
    bc.append(BCGroup([(_x(mid), 0.0), (_y([mid[0], mid[1], nid(0, 1, km)]), 1e-4)]))
    bc.append(BCGroup([(_z(top[:4]), 0.01), (_z(top[:2]), -0.015)],
                      *_tab((2, 30, 12, 60, 70), (0, 1, -1, 2, 0))))
    bc.append(BCGroup([(_z(top[2:4]), 0.0)]))
    bc.append(BCGroup([(_y(col), 2e-4)], *_tab((3, 10, 25), (1, 0, 3))))
    bc.append(BCGroup([(_z([mid[-1], nid(1, 1, 2)]), 0.0), (_x([nid(nx, ny, 1)]), 0.0)],
                      *_tab((4, 16, 50), (1, -1, -2))))
    m.bc = bc
    m.name = "bc_deck_wide" if rollers else "bc_deck"
    return m


def bc_deck_wide() -> Model:
    """The same groups on a 6 x 6 x 8 bar with its lateral faces on rollers: more than 256 resolved
    dofs, and not a multiple of 256, so k_bc runs a full and a partial block."""
    return bc_deck(6, 6, 8, rollers=True)


def top_nodes(m: Model, nx=3, ny=2) -> np.ndarray:
    return mesh.plane_nodes(nx, ny, m.nNode // ((nx + 1) * (ny + 1)) - 1)


def writers(m: Model) -> dict:
    """dof (0-based) -> [(group, value)] in the order :585-617 writes it."""
    w = {}
    for g, grp in enumerate(m.bc):
        for dofs, v in grp.entries:
            for d in np.asarray(dofs, np.int64):
                w.setdefault(int(d) - 1, []).append((g, float(v)))
    return w


def resolved(m: Model) -> dict:
    """dof (0-based) -> (group, value) of its last writer: what hakai_set_bc must keep."""
    return {d: ws[-1] for d, ws in writers(m).items()}


def group_amp(m: Model, g: int, t: int) -> float:
    grp = m.bc[g]
    return 1.0 if grp.amp_time is None else R.amplitude(grp.amp_time, grp.amp_value, float(t) * m.dt)


def bc_values(m: Model, t: int) -> dict:
    """dof (0-based) -> prescribed value of step t, through nodal_ref.apply_bc."""
    x = np.full(3 * m.nNode, np.nan)
    R.apply_bc(m, float(t) * m.dt, x)
    return {d: x[d] for d in writers(m)}


def check_deck(m: Model, steps=range(1, N_STEPS + 1), subsets=True, writers_differ=True):
    """The self-check of bc_deck (computed with nodal_ref): every listed branch is hit. The rollers of
    bc_deck_wide write the same zero as ENCASTRE and MID on shared dofs and cover the lateral nodes:
    there the two checks on the writers and the dof subsets are switched off."""
    steps = list(steps)
    for g, grp in enumerate(m.bc):
        if grp.amp_time is None:
            continue
        a_t = [float(x) for x in grp.amp_time]
        cts = [float(t) * m.dt for t in steps]
        assert any(ct < min(a_t) and not R.segment(a_t, ct)[1] for ct in cts), f"group {g}: no step before the table"
        assert any(ct in a_t[1:-1] for ct in cts), f"group {g}: no step on an interior breakpoint"
        assert any(R.segment(a_t, ct)[0] > 0 for ct in cts), f"group {g}: only the first segment"
        assert any(ct > max(a_t) and not R.segment(a_t, ct)[1] for ct in cts), f"group {g}: no step after the table"
    multi = {d: ws for d, ws in writers(m).items() if len(ws) > 1}
    assert multi
    for d, ws in multi.items() if writers_differ else ():
        (g0, v0), (g1, v1) = ws[0], ws[-1]
        assert any(v0 * group_amp(m, g0, t) != v1 * group_amp(m, g1, t) for t in steps), \
            f"dof {d}: first and last writer agree at every step"
    assert any(len({g for g, _ in ws}) < len(ws) for ws in multi.values()), "no dof written twice by one group"
    assert any(len({g for g, _ in ws}) > 1 for ws in multi.values()), "no dof written by two groups"
    neg0 = [t for t in steps for v in bc_values(m, t).values() if v == 0.0 and np.signbit(v)]
    assert neg0, "no -0.0 among the prescribed values"
    if subsets:
        res = resolved(m)
        per_node = {}
        for d in res:
            per_node.setdefault(d // 3, set()).add(d % 3)
        assert {frozenset(s) for s in per_node.values()} == \
            {frozenset(s) for s in ((0,), (1,), (2,), (0, 1), (0, 2), (1, 2), (0, 1, 2))}, "dof subsets"
        assert 0 in per_node and m.nNode - 1 in per_node, "first / last node"
        nodes = sorted(per_node)
        assert any(b == a + 1 and per_node[a] != per_node[b] for a, b in zip(nodes, nodes[1:])), "neighbours"
        assert any(b > a + 1 for a, b in zip(nodes, nodes[1:])), "no free node between constrained ones"


# ---- one-step probes of k_nodal's uploaded-Q path ------------------------------------------------
PROBE_BLOCKS = (1, 15, 16, 17, 23, 24, 25, 33)   # k_nodal blocks of 256 nodes: nwg < 16 | nwg & 7 = 0, 1, 7
PROBE_SETS = ("random", "cancel", "subnormal_q", "huge_tiny", "zeros")


def probe_bars() -> list:
    """[(blocks, model)]: elastic 1 x 1 x nz bars without BCs, nN = 4 (nz + 1) = 256 (blocks - 1) + 100."""
    out = []
    for b in PROBE_BLOCKS:
        nz = 64 * (b - 1) + 24
        m = small_bar(1, 1, nz, material=mesh.steel_elastic(), n_steps=1, d_time=D_TIME)
        m.bc = []
        assert m.nNode % 256 == 100 and (m.nNode + 255) // 256 == b
        out.append((b, m))
    return out


def probe_bc(m: Model) -> list:
    """BC groups for a probe bar: all seven dof subsets over residues of the node id, the first and
    the last node, one group with an amplitude that step 1 interpolates."""
    n = np.arange(1, m.nNode + 1, dtype=np.int64)
    ends = np.array([1, m.nNode], np.int64)
    return [BCGroup([(_x(n[n % 7 == 0]), 1e-3), (_z(ends), -2e-3)]),
            BCGroup([(_y(n[n % 5 == 0]), 2.0), (_z(n[n % 11 == 0]), -3.0), (_x(ends), 0.0), (_y(ends), 0.5)],
                    np.array([0.0, T(4)]), np.array([0.5, 1.5]))]


def probe_states(nN: int, seed: int) -> list:
    """One-step operand sets [(name, diag_M, u, u_pre, Q)], 3 nN values each, for the uploaded-Q
    path (f = 0). One diag_M per (nN, seed), shared by the sets so that one device context serves
    them all: per-node masses of 1e-9..1e-8, every third node's NEGATIVE (an inverted mesh gives
    that). No zero mass, nothing whose exact result overflows, no Inf or NaN.

      random       normal u, u_pre, Q: every dof its own expected value
      cancel       u_pre = 2u exactly (2u - u_pre == 0) and one ulp to either side of it; Q = 0 on
                   some of them, so the whole bracket is a signed zero
      subnormal_q  Q a few units of 2^-1074 of either sign; u = u_pre = 0 on half the dofs, where
                   inv * (-Q) rounds into the subnormal range or to a signed zero
      huge_tiny    terms of 1e150 next to 1e-150 in every slot
      zeros        +-0.0 in each slot: all three at once in the 8 sign combinations, and one slot
                   at a time next to random values
    """
    rng = np.random.default_rng([seed, nN])
    fn = 3 * nN
    i = np.arange(fn)
    mass = rng.uniform(1e-9, 1e-8, size=nN)
    mass[np.arange(nN) % 3 == 1] *= -1.0
    diag = np.repeat(mass, 3)
    nrm = lambda s: rng.normal(0.0, s, size=fn)  # noqa: E731
    sgn = lambda: rng.choice([-1.0, 1.0], size=fn)  # noqa: E731
    out = [("random", diag, nrm(1e-2), nrm(1e-2), nrm(1e3))]

    u = nrm(1e-2)
    up = 2.0 * u
    up[i % 4 == 1] = np.nextafter(up[i % 4 == 1], np.inf)
    up[i % 4 == 3] = np.nextafter(up[i % 4 == 3], -np.inf)
    q = nrm(1e3)
    q[i % 8 == 0] = 0.0
    q[i % 8 == 4] = -0.0
    out.append(("cancel", diag, u, up, q))

    q = sgn() * rng.integers(1, 1000, size=fn) * 2.0 ** -1074
    u, up = nrm(1e-2), nrm(1e-2)
    u[i % 2 == 0] = 0.0
    up[i % 2 == 0] = 0.0
    out.append(("subnormal_q", diag, u, up, q))

    big, tiny = sgn() * rng.uniform(1.0, 9.0, size=fn) * 1e150, sgn() * rng.uniform(1.0, 9.0, size=fn) * 1e-150
    k = i % 6
    u = np.where(k < 3, big, tiny)
    up = np.where((k == 1) | (k == 3) | (k == 4), rng.permutation(big), rng.permutation(tiny))
    q = np.where((k == 2) | (k == 3) | (k == 5), rng.permutation(big), rng.permutation(tiny))
    out.append(("huge_tiny", diag, u, up, q))

    u, up, q = nrm(1e-2), nrm(1e-2), nrm(1e3)
    k = i % 16
    z = lambda bit: np.where((k >> bit) & 1, -0.0, 0.0)  # noqa: E731
    all3 = k < 8
    u = np.where(all3 | (k == 8) | (k == 9), np.where(k == 9, -0.0, z(0)), u)
    up = np.where(all3 | (k == 10) | (k == 11), np.where(k == 11, -0.0, np.where(k == 10, 0.0, z(1))), up)
    q = np.where(all3 | (k == 12) | (k == 13), np.where(k == 13, -0.0, np.where(k == 12, 0.0, z(2))), q)
    out.append(("zeros", diag, u, up, q))
    assert tuple(s[0] for s in out) == PROBE_SETS
    return [(name, d, np.ascontiguousarray(a), np.ascontiguousarray(b), np.ascontiguousarray(c))
            for name, d, a, b, c in out]
