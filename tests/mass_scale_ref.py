"""NumPy float64 restatement of hakai-fem_amd/csrc/hakai_mass_scale_elem.hpp and of the nodal gather and
the reductions of hakai_mass_scale -- TEST INFRASTRUCTURE. No GPU, no library.

Every sum, product and division below is the header's, one rounding each, so the header compiled for
the host (tests/test_mass_scale_cpu.py) and the kernels (tests/test_gpu_mass_scale.py) must give the
same bits. V, gg, ss, V0 and A_max are stable_dt_ref's (the restatement of hakai_stable_dt_elem.hpp).

The guarantee, by counting roundings (u = 2^-53, no overflow or underflow; every (1 + d) has |d| <= u).
Let h = dt_target / (2 safety) exactly. For an active element that is neither capped nor unfixable:
  half  = fl((0.5 dt_target) / safety) = h (1 + d1)            (0.5 dt_target is exact)
  hh    = fl(half half)               = h^2 (1 + d1)^2 (1 + d2)
  p     = fl(kappa hh)                = kappa h^2 (1 + d1)^2 (1 + d2)(1 + d3)
  a     = fl(p - m0)                  = (p - m0)(1 + d4)
If a <= added_prev (a < 0 included) the element keeps added_prev >= a, and every operation below is
monotone in the added mass, so it is enough to take added_new = a >= 0, where 0 <= p - m0 <= p:
  me    = fl(m0 + a) = (p + (p - m0) d4)(1 + d5) >= p (1 - u)^2
  q     = fl(me / kappa) >= h^2 (1 - u)^6
  dt_safe = 2 fl(sqrt(q)) >= 2 h (1 - u)^3 (1 - u) = (dt_target / safety)(1 - u)^4
so dt_safe >= dt_target whenever safety <= (1 - u)^4, and 1 - 2^-40 is far below that. (The bound on
the true critical step is DESIGN section 2's: v'Kv <= sum_e kappa_e |v_e|^2 <= max_e (kappa_e / me_e)
v'Mv with M = sum_e me_e I_e, for any per-element masses.)

mass_added: the terms 8 added_e are non-negative and the tree has ceil(log2 nE) levels, each level
rounding every partial sum once, so |tree - exact| <= ((1 + u)^L - 1) exact ~ L u exact."""
import numpy as np

import numpy_ref
import stable_dt_ref as R

OK, CAPPED, UNFIXABLE = 0, 1, 2
KEYS = ("n_active", "n_scaled", "n_changed", "n_capped", "n_unfixable", "max_factor_reached", "element_factor",
        "mass_added", "dt_safe", "element_safe")


def sums(x, X):
    """(V, gg, ss, V0, Amax), each (n,), of n elements at current / initial positions (n, 8, 3): the
    quantities stable_element hands to stable_finish."""
    x, X = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(X, np.float64)
    P = numpy_ref.pusai()
    t, d0 = zip(*[R._gp(P[k], x, X) for k in range(8)])
    S = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))
    V0 = np.zeros(x.shape[0])
    for k in range(8):
        V0 = V0 + d0[k]
    Amax = R._face(x, *R.FACES[0])
    for f in R.FACES[1:]:
        a = R._face(x, *f)
        Amax = np.where(a > Amax, a, Amax)
    Amax = 0.5 * np.sqrt(Amax)
    V = S[0]
    with np.errstate(divide="ignore", invalid="ignore"):
        p = []
        for i in range(8):
            g0, g1, g2 = S[1 + i] / V, S[9 + i] / V, S[17 + i] / V
            p.append((g0 * g0 + g1 * g1) + g2 * g2)
        gg = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]))
    return V, gg, S[25], V0, Amax


def half_of(dt_target, safety):
    return (np.float64(0.5) * np.float64(dt_target)) / np.float64(safety)


def need(V, gg, ss, V0, Kb, two_mu, rho8, half, max_factor, prev):
    """mass_need: (added_new, status)."""
    prev = np.asarray(prev, np.float64)
    with np.errstate(all="ignore"):
        kappa = (Kb * V) * gg + two_mu * ss
        unfix = (V0 <= 0.0) | (V == 0.0) | ~((kappa - kappa) == 0.0)
        m0 = rho8 * V0
        a = kappa * (half * half) - m0
        cap = (np.float64(max_factor) - 1.0) * m0
        capped = ~unfix & (a > cap)
        a = np.where(capped, cap, a)
        new = np.where(a > prev, a, prev)
    status = np.where(unfix, UNFIXABLE, np.where(capped, CAPPED, OK))
    return np.where(unfix, prev, new), status


def factor(V0, rho8, added):
    with np.errstate(all="ignore"):
        m0 = rho8 * V0
        return (m0 + added) / m0


def finish_added(V, gg, ss, V0, Amax, c, Kb, two_mu, rho8, added):
    """stable_finish_added: (dt_est, dt_safe)."""
    with np.errstate(all="ignore"):
        L = V / Amax
        kappa = (Kb * V) * gg + two_mu * ss
        m0 = rho8 * V0
        me = m0 + added
        est = (L / c) * np.sqrt(me / m0)
        safe = 2.0 * np.sqrt(me / kappa)
    zero = (V0 <= 0.0) | (V == 0.0) | (Amax == 0.0)
    return np.where(zero, 0.0, est), np.where(zero, 0.0, safe)


def tree_sum(v):
    """One fixed binary tree in order: neighbours first, a subtree without a sibling moves up unchanged."""
    v = np.array(v, np.float64)
    if v.size == 0:
        return 0.0
    while v.size > 1:
        n2 = v.size // 2
        w = v[0:2 * n2:2] + v[1:2 * n2:2]
        v = np.concatenate([w, v[2 * n2:]])
    return float(v[0])


def nodal_mass(M0, elementmat, added):
    """M_n = M0_n + sum of added_e over the node's incidences in ascending (8e + i) order, one rounding
    per addition, zeros included. M0 (nN,), elementmat (nE, 8) 1-based."""
    M = np.array(M0, np.float64)
    node = (np.asarray(elementmat) - 1).ravel()
    order = np.argsort(node, kind="stable")              # by node, ascending (8e + i) within a node
    ns = node[order]
    first = np.searchsorted(ns, ns, side="left")
    rank = np.arange(ns.size) - first
    val = np.repeat(np.asarray(added, np.float64), 8)[order]
    for r in range(int(rank.max()) + 1 if rank.size else 0):
        sel = rank == r                                   # at most one incidence of a node per pass
        M[ns[sel]] = M[ns[sel]] + val[sel]
    return M


def model(m, dt_target=None, safety=0.9, max_factor=np.inf, mass_scaling=None, disp=None, flag=None, prev=None,
          M0=None, element_offset=0):
    """hakai_mass_scale on a hakai Model at displacement disp (3 nN), flags and previous added mass:
    the record (KEYS) plus elem_added (nE), diag_M (3 nN) and the per-element dt_est_elem /
    dt_safe_elem that hakai_stable_dt reports afterwards (+inf where the element is deleted)."""
    ms = m.mass_scaling if mass_scaling is None else mass_scaling
    dt = m.dt if dt_target is None else dt_target
    nE = m.nElement
    X = m.coordmat
    xc = X if disp is None else X + np.asarray(disp).reshape(-1, 3)
    flag = np.ones(nE, np.int64) if flag is None else np.asarray(flag)
    prev = np.zeros(nE) if prev is None else np.asarray(prev, np.float64)
    if M0 is None:
        M0 = m.lumped_mass()[0][0::3]
    act = flag == 1
    mats = np.array([R.stable_mat(mt.young, mt.poisson, mt.density, ms) for mt in m.materials])
    k = mats[m.element_material - 1]
    n = m.elementmat - 1
    V, gg, ss, V0, Amax = sums(xc[n], X[n])
    new, status = need(V, gg, ss, V0, k[:, 1], k[:, 2], k[:, 3], half_of(dt, safety), max_factor, prev)
    added = np.where(act, new, prev)
    est, safe = finish_added(V, gg, ss, V0, Amax, k[:, 0], k[:, 1], k[:, 2], k[:, 3], added)
    est, safe = np.where(act, est, np.inf), np.where(act, safe, np.inf)
    out = dict(n_active=int(act.sum()), n_scaled=int((added > 0).sum()), n_changed=int((act & (added > prev)).sum()),
               n_capped=int((act & (status == CAPPED)).sum()), n_unfixable=int((act & (status == UNFIXABLE)).sum()),
               max_factor_reached=1.0, element_factor=0, mass_added=tree_sum(8.0 * added), dt_safe=np.inf,
               element_safe=0, elem_added=added, dt_est_elem=est, dt_safe_elem=safe, status=status)
    elig = act & (V0 > 0.0)
    if elig.any():
        f = np.where(elig, factor(V0, k[:, 3], added), -np.inf)
        i = int(np.argmax(f))                             # the first of equal values
        out.update(max_factor_reached=float(f[i]), element_factor=i + 1 + element_offset)
    if act.any():
        i = int(np.argmin(safe))
        out.update(dt_safe=float(safe[i]), element_safe=i + 1 + element_offset)
    out["diag_M"] = np.repeat(nodal_mass(M0, m.elementmat, added), 3)
    return out
