"""Reference of the output node averages -- TEST INFRASTRUCTURE ONLY.

Written from the reference's lines (cal_node_stress_strain, v2/HAKAI_j.jl:3408-3486), not from the
oracle or the kernel, as nodal_ref.py is for the nodal update:

  node_average        :3428-3478 operation for operation in IEEE double
  node_average_exact  the five linear fields (stress, strain, eqps, triax averages) in exact
                      rationals, rounded once, with the magnitude sum the rounding bound is relative
                      to (the guard against a mistake node_average and the oracle could share)
  mises               :3477 on one stress six-vector; node_average applies it to the node average

Arrays are in the project's layout: elementmat (nE, 8) 1-based (Julia's 8 x nE), stress and strain
(8 nE, 6) (Julia's 6 x 8nE, transposed at :3410-3411), eqps and triax (8 nE,).

The rounding bound (COUNT_FIXED, average_bound)
-----------------------------------------------
For one node and one linear field let m be the number of scatter additions the node receives
(:3448-3451: one per (element, local node) pair that names it) and cnt its divisor (:3458). The
value is  x = (sum over those m pairs of (g_1 + ... + g_8) / 8) / cnt. Each Gauss-point value g
passes through

  7      additions of the element mean (:3435-3438: sum! starts from zeros(1,6) and 0.0 + g_1 is
         exact; sum() starts from g_1; the eight terms are added left to right)
  0      for "/ integ_num": a division by 8 is exact (barring underflow, below)
  m - 1  additions of the scatter (the first one adds to the 0.0 of zeros(nNode, 6): exact)
  1      division by cnt

so at most k = m + 7 roundings, each a factor (1 + e), |e| <= 2^-53 = u. The product of k such
factors is within gamma_k = k u / (1 - k u) of one, hence

  |x - X| <= gamma_(m + 7) * S,   S = (sum of |g| over the m pairs' 8 m Gauss points) / (8 cnt).

COUNT_FIXED = 8 is the part of k that does not depend on the node (7 + 1); k = m - 1 + COUNT_FIXED.
It is a count of operations, not a fitted figure. With every element listing 8 distinct nodes,
m = cnt.

Underflow: a sum of doubles that lands in the subnormal range is exact, so the additions add
nothing. The m divisions by 8 and the final division can round into the subnormal range, each with
an absolute error of at most 2^-1075; the first m are then carried through the sums (factors
(1 + e), covered by doubling) and divided by cnt. average_bound adds 2^-1074 * (m / cnt + 1).

Overflow is out of the bound's scope: a sum that overflows is +-Inf from there on (or NaN after
Inf - Inf), which node_average shows as a non-finite result; callers skip those.
"""
from __future__ import annotations

from fractions import Fraction

import numpy as np

COUNT_FIXED = 8                 # 7 additions of the element mean + 1 division by the divisor
U = Fraction(1, 2 ** 53)        # unit roundoff of double
TINY = Fraction(1, 2 ** 1074)   # smallest subnormal
INTEG_NUM = 8
FIELDS = ("node_stress", "node_strain", "node_eq_plastic_strain", "node_mises_stress", "node_triax_stress")
LINEAR = ("node_stress", "node_strain", "node_eq_plastic_strain", "node_triax_stress")


def mises(s6):
    """:3471-3477 on one six-vector (ox, oy, oz, txy, tyz, txz): x^2 is x * x, the sums go left to
    right, the third difference is (ox - oz)."""
    ox, oy, oz, txy, tyz, txz = (np.float64(v) for v in s6)
    with np.errstate(all="ignore"):
        return np.sqrt(0.5 * ((ox - oy) * (ox - oy) + (oy - oz) * (oy - oz) + (ox - oz) * (ox - oz)
                              + 6.0 * (txy * txy + tyz * tyz + txz * txz)))


def _arrays(nNode, elementmat, stress, strain, eqps, triax):
    em = np.asarray(elementmat, np.int64).reshape(-1, 8)
    nE = em.shape[0]
    st = np.asarray(stress, np.float64).reshape(nE, INTEG_NUM, 6)
    sn = np.asarray(strain, np.float64).reshape(nE, INTEG_NUM, 6)
    eq = np.asarray(eqps, np.float64).reshape(nE, INTEG_NUM)
    tx = np.asarray(triax, np.float64).reshape(nE, INTEG_NUM)
    assert em.size == 0 or (em.min() >= 1 and em.max() <= nNode)
    return em, nE, st, sn, eq, tx


def divisor(nNode, elementmat):
    """:3455-3459: inc_num[elementmat[:,i]] .+= 1 per element. The indexed update reads and writes
    every listed entry once, so a node an element lists twice still counts once for that element
    (numpy's fancy-index += has the same semantics)."""
    em = np.asarray(elementmat, np.int64).reshape(-1, 8)
    inc = np.zeros(nNode)
    for e in range(em.shape[0]):
        inc[em[e] - 1] += 1
    return inc


def node_average(nNode, elementmat, stress, strain, eqps, triax):
    """:3428-3478 in double, one IEEE operation per operation of the source. Returns the five
    fields under the names Solver.node_stress_strain() uses. A node no element lists is 0/0 = NaN
    in all five."""
    em, nE, st, sn, eq, tx = _arrays(nNode, elementmat, stress, strain, eqps, triax)
    with np.errstate(all="ignore"):
        # :3428-3440 element means: sum!(zeros(1,6), rows) / integ_num and sum(values) / integ_num
        e_st, e_sn = np.zeros((nE, 6)), np.zeros((nE, 6))
        for k in range(INTEG_NUM):
            e_st = e_st + st[:, k, :]
            e_sn = e_sn + sn[:, k, :]
        e_st = e_st / INTEG_NUM
        e_sn = e_sn / INTEG_NUM
        e_eq, e_tx = eq[:, 0].copy(), tx[:, 0].copy()
        for k in range(1, INTEG_NUM):
            e_eq = e_eq + eq[:, k]
            e_tx = e_tx + tx[:, k]
        e_eq = e_eq / INTEG_NUM
        e_tx = e_tx / INTEG_NUM
        # :3442-3453 scatter: element order, then local-node order
        n_st, n_sn = np.zeros((nNode, 6)), np.zeros((nNode, 6))
        n_eq, n_tx = np.zeros(nNode), np.zeros(nNode)
        for i in range(nE):
            for k in range(8):
                n = em[i, k] - 1
                n_st[n] = n_st[n] + e_st[i]
                n_sn[n] = n_sn[n] + e_sn[i]
                n_eq[n] = n_eq[n] + e_eq[i]
                n_tx[n] = n_tx[n] + e_tx[i]
        # :3455-3467
        inc = divisor(nNode, em)
        n_st = n_st / inc[:, None]
        n_sn = n_sn / inc[:, None]
        n_eq = n_eq / inc
        n_tx = n_tx / inc
        # :3469-3478
        n_mi = np.array([mises(n_st[i]) for i in range(nNode)]) if nNode else np.zeros(0)
    return dict(node_stress=n_st, node_strain=n_sn, node_eq_plastic_strain=n_eq, node_mises_stress=n_mi,
                node_triax_stress=n_tx)


def node_average_exact(nNode, elementmat, stress, strain, eqps, triax):
    """The four linear fields in exact rationals. Returns (value, S, m, cnt): value and S are dicts
    of the LINEAR names -> (nNode, width) object arrays of Fractions (width 6, 6, 1, 1; None where the
    node's divisor is zero or an input of the node is not finite), S the magnitude sum of the module
    docstring; m (nNode,) the scatter additions per node and cnt (nNode,) the divisor."""
    em, nE, st, sn, eq, tx = _arrays(nNode, elementmat, stress, strain, eqps, triax)
    src = dict(node_stress=st, node_strain=sn, node_eq_plastic_strain=eq[:, :, None],
               node_triax_stress=tx[:, :, None])
    cnt = divisor(nNode, em).astype(np.int64)
    pairs = [[] for _ in range(nNode)]
    for i in range(nE):
        for k in range(8):
            pairs[em[i, k] - 1].append(i)
    m = np.array([len(p) for p in pairs], np.int64)
    value, S = {}, {}
    for name, a in src.items():
        w = a.shape[2]
        # per element and component: the sum and the magnitude sum of its eight Gauss points
        tot = [[None] * w for _ in range(nE)]
        mag = [[None] * w for _ in range(nE)]
        for i in range(nE):
            for c in range(w):
                g = a[i, :, c]
                if np.isfinite(g).all():
                    f = [Fraction(float(x)) for x in g]
                    tot[i][c] = sum(f, Fraction(0))
                    mag[i][c] = sum((abs(x) for x in f), Fraction(0))
        v = np.full((nNode, w), None, object)
        s = np.full((nNode, w), None, object)
        for n in range(nNode):
            if cnt[n] == 0:
                continue
            for c in range(w):
                if any(tot[i][c] is None for i in pairs[n]):
                    continue
                v[n, c] = sum((tot[i][c] for i in pairs[n]), Fraction(0)) / (INTEG_NUM * int(cnt[n]))
                s[n, c] = sum((mag[i][c] for i in pairs[n]), Fraction(0)) / (INTEG_NUM * int(cnt[n]))
        value[name], S[name] = v, s
    return value, S, m, cnt


def same_bits(a, b):
    """The comparison rule of the output fields: the same shape, NaN at the same positions, and the
    same IEEE bits everywhere else (+-Inf and +-0 included). A NaN's sign and payload are not
    compared: no printed file shows them."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))


def rounded(value):
    """An exact field of node_average_exact rounded to double once (float(Fraction) rounds to
    nearest even); NaN where it is None."""
    return np.array([[np.nan if x is None else float(x) for x in row] for row in value])


def average_bound(S, m, cnt):
    """|node_average - exact| <= this for one value (exact rational): gamma_k * S with
    k = m - 1 + COUNT_FIXED roundings, plus the divisions that may underflow (module docstring)."""
    k = int(m) - 1 + COUNT_FIXED
    return k * U / (1 - k * U) * S + TINY * (Fraction(int(m), int(cnt)) + 1)
