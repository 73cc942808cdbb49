"""High-precision restatement of one hex8 element update -- TEST INFRASTRUCTURE.

Written from the formulas of cal_stress_hexa (v2/HAKAI_j.jl:1033-1371: Pusai table, Jacobians,
B-bar with |det| weights, Bfinal, D*de, J2 radial return, internal force, volume) and of the
invariant triaxiality, not from the oracle and not from numpy_ref: plain sums and products in
60-digit decimal arithmetic (the standard library's `decimal`, so it runs wherever the tests run),
no operation order to preserve, no fused multiply-adds, no structural zeros to skip. The inputs
are the FP64 positions, displacement increments, Gauss-point state and material tables, taken
exactly (every double is a finite decimal); everything derived from them -- 1/sqrt(3), the
elastic matrix, the hardening slopes -- is formed in high precision too. Outputs are rounded once
to FP64.

It is the yardstick for the oracle itself (tests/test_hp_ref.py) and for the fused GPU kernel,
whose sums are re-associated and cannot be bit-exact (tests/test_gpu_element_edges.py): errors
are counted in units of 2^-53 of a LOCAL scale, the largest high-precision magnitude within the
entry's own Gauss point (stress, strain) or element (Qe), never a whole-array maximum, so a wrong
small shear component or one wrong Gauss point cannot hide behind a large entry elsewhere.
"""
from decimal import Decimal, localcontext

import numpy as np

PREC = 60
# Node signs (v2/HAKAI_j.jl:1900-1907) and Gauss-point signs (:1913-1920: k bits = xi, eta, zeta)
DELTA = ((-1, -1, -1), (1, -1, -1), (1, 1, -1), (-1, 1, -1), (-1, -1, 1), (1, -1, 1), (1, 1, 1), (-1, 1, 1))
GP = ((-1, -1, -1), (-1, -1, 1), (-1, 1, -1), (-1, 1, 1), (1, -1, -1), (1, -1, 1), (1, 1, -1), (1, 1, 1))


def _D(x):
    return Decimal(float(x))   # exact


def pusai():
    """dN_i/d(xi, eta, zeta) at the 8 Gauss points (+-1/sqrt(3)): P[k][r][i], Decimal."""
    g = 1 / Decimal(3).sqrt()
    P = []
    for k in range(8):
        xi, eta, ze = (s * g for s in GP[k])
        rows = [[], [], []]
        for i in range(8):
            d = DELTA[i]
            rows[0].append(d[0] * (1 + eta * d[1]) * (1 + ze * d[2]) / 8)
            rows[1].append(d[1] * (1 + xi * d[0]) * (1 + ze * d[2]) / 8)
            rows[2].append(d[2] * (1 + xi * d[0]) * (1 + eta * d[1]) / 8)
        P.append(rows)
    return P


def _inv3(J):
    a, b, c = J[0]
    d, e, f = J[1]
    g, h, i = J[2]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    inv = [[(e * i - f * h) / det, (c * h - b * i) / det, (b * f - c * e) / det],
           [(f * g - d * i) / det, (a * i - c * g) / det, (c * d - a * f) / det],
           [(d * h - e * g) / det, (b * g - a * h) / det, (a * e - b * d) / det]]
    return det, inv


def element_update(X, du, sig, eps, eqps, ys, mat):
    """One active element. X (8, 3) positions, du (8, 3) displacement increments, sig/eps (8, 6),
    eqps/ys (8,) FP64; mat with young, poisson, plastic (rows: yield stress, eq. plastic strain).
    Returns a dict of FP64 arrays sig, eps, eqps, ys (8 Gauss points), Qe (24), V, triax (8), and
      q_minus_ys: per Gauss point the trial Mises stress minus the yield stress, RELATIVE to the yield
                  stress, as a float (None for an elastic material): how far the point is from the
                  yield surface, so a test can require that no rounding error decides the branch;
      plastic:    per Gauss point whether the radial return ran."""
    with localcontext() as ctx:
        ctx.prec = PREC
        P = pusai()
        X = [[_D(v) for v in row] for row in np.asarray(X, np.float64).reshape(8, 3)]
        du = [_D(v) for v in np.asarray(du, np.float64).reshape(24)]
        E, nu = _D(mat.young), _D(mat.poisson)
        c0 = E / (1 + nu) / (1 - 2 * nu)
        Dn, Do, Ds = c0 * (1 - nu), c0 * nu, c0 * (1 - 2 * nu) / 2
        G = E / 2 / (1 + nu)
        pl = [[_D(v) for v in row] for row in np.asarray(mat.plastic, np.float64).reshape(-1, 2)]
        npp = len(pl)
        Hd = [(pl[r + 1][0] - pl[r][0]) / (pl[r + 1][1] - pl[r][1]) for r in range(npp - 1)]

        # Jacobians, dN/dx and the volume
        det, P2 = [], []
        for k in range(8):
            J = [[sum(P[k][r][i] * X[i][c] for i in range(8)) for c in range(3)] for r in range(3)]
            dk, inv = _inv3(J)
            # x_c = sum_i N_i X[i][c]: J[r][c] = d x_c / d xi_r, and dN_i/dx_c = sum_r inv[c][r] dN_i/dxi_r
            P2.append([[sum(inv[c][r] * P[k][r][i] for r in range(3)) for i in range(8)] for c in range(3)])
            det.append(dk)
        V = sum(abs(d) for d in det)
        # B-bar: the |det|-weighted mean of dN_i/dx_c / 3 (cal_BVbar_hexa forms dN/dx with 1/|det|
        # and weights by |det|: sign(det) * |det| = det)
        BV = [[sum(P2[k][c][i] * det[k] for k in range(8)) / (3 * V) for c in range(3)] for i in range(8)]

        out_sig, out_eps, out_eq, out_ys, out_tri, margin, plastic = [], [], [], [], [], [], []
        Qe = [Decimal(0)] * 24
        for k in range(8):
            # Bfinal (6 x 24), Voigt (xx, yy, zz, xy, yz, xz), engineering shear
            B = [[Decimal(0)] * 24 for _ in range(6)]
            for i in range(8):
                px, py, pz = P2[k][0][i], P2[k][1][i], P2[k][2][i]
                B[0][3 * i] = px
                B[1][3 * i + 1] = py
                B[2][3 * i + 2] = pz
                B[3][3 * i], B[3][3 * i + 1] = py, px
                B[4][3 * i + 1], B[4][3 * i + 2] = pz, py
                B[5][3 * i], B[5][3 * i + 2] = pz, px
                for c in range(3):
                    t = BV[i][c] - P2[k][c][i] / 3
                    for r in range(3):
                        B[r][3 * i + c] += t
            de = [sum(B[r][j] * du[j] for j in range(24)) for r in range(6)]
            s0 = [_D(v) for v in sig[k]]
            tr = de[0] + de[1] + de[2]
            s = [s0[0] + (Dn - Do) * de[0] + Do * tr, s0[1] + (Dn - Do) * de[1] + Do * tr,
                 s0[2] + (Dn - Do) * de[2] + Do * tr, s0[3] + Ds * de[3], s0[4] + Ds * de[4], s0[5] + Ds * de[5]]
            eq_k, ys_k = _D(eqps[k]), _D(ys[k])
            did = False
            if npp > 0:
                mean = (s[0] + s[1] + s[2]) / 3
                dev = [s[0] - mean, s[1] - mean, s[2] - mean, s[3], s[4], s[5]]
                q = (Decimal(3) / 2 * (dev[0] ** 2 + dev[1] ** 2 + dev[2] ** 2
                                       + 2 * (dev[3] ** 2 + dev[4] ** 2 + dev[5] ** 2))).sqrt()
                margin.append(float((q - ys_k) / ys_k) if ys_k != 0 else float("inf"))
                if q > ys_k:
                    p = npp - 2                      # the segment rule: first row j >= 1 with eqps <= plastic[j, 2]
                    for j in range(1, npp):
                        if eq_k <= pl[j][1]:
                            p = j - 1
                            break
                    H = Hd[p]
                    dep = (q - ys_k) / (3 * G + H)
                    scale = (ys_k + H * dep) / q
                    s = [dev[0] * scale + mean, dev[1] * scale + mean, dev[2] * scale + mean,
                         dev[3] * scale, dev[4] * scale, dev[5] * scale]
                    eq_k = eq_k + dep
                    ys_k = ys_k + H * dep
                    did = True
            else:
                margin.append(None)
            plastic.append(did)
            out_sig.append([float(v) for v in s])
            out_eps.append([float(_D(eps[k][r]) + de[r]) for r in range(6)])
            out_eq.append(float(eq_k))
            out_ys.append(float(ys_k))
            # triaxiality, invariant form: mean stress over Mises stress of the final stress
            mean = (s[0] + s[1] + s[2]) / 3
            oeq = (((s[0] - s[1]) ** 2 + (s[1] - s[2]) ** 2 + (s[2] - s[0]) ** 2) / 2
                   + 3 * (s[3] ** 2 + s[4] ** 2 + s[5] ** 2)).sqrt()
            out_tri.append(0.0 if oeq < Decimal("1e-10") else float(mean / oeq))
            # internal force: det * Bfinal' * sigma (signed det, unit Gauss weights)
            for j in range(24):
                Qe[j] += det[k] * sum(B[r][j] * s[r] for r in range(6))
        return dict(sig=np.array(out_sig), eps=np.array(out_eps), eqps=np.array(out_eq), ys=np.array(out_ys),
                    Qe=np.array([float(v) for v in Qe]), V=float(V), triax=np.array(out_tri),
                    q_minus_ys=margin, plastic=plastic)


NAMES = ("stress", "strain", "eqps", "yield", "Qe", "volume")


def update(m, pos, dd, st, sn, eq, ys, flag=None, elements=None):
    """The element update of a whole (small) model in the layout of cal_stress_hexa's arrays: returns
    {stress (8nE, 6), strain (8nE, 6), eqps (8nE,), yield (8nE,), Qe (nE, 24), volume (nE,)}, the
    relative yield margins (8nE, NaN where none) and the list of elements computed (`elements`, default
    all with flag 1). Elements not computed keep their input state, Qe 0 and volume 0."""
    nE = m.nElement
    flag = np.ones(nE, np.int64) if flag is None else flag
    els = [e for e in (range(nE) if elements is None else elements) if flag[e] == 1]
    pos = np.asarray(pos, np.float64).reshape(-1, 3)
    dd = np.asarray(dd, np.float64).reshape(-1, 3)
    out = dict(stress=np.array(st, np.float64), strain=np.array(sn, np.float64), eqps=np.array(eq, np.float64))
    out["yield"] = np.array(ys, np.float64)
    out["Qe"] = np.zeros((nE, 24))
    out["volume"] = np.zeros(nE)
    margin = np.full(8 * nE, np.nan)
    for e in els:
        nodes = m.elementmat[e] - 1
        g = slice(8 * e, 8 * e + 8)
        r = element_update(pos[nodes], dd[nodes], st[g], sn[g], eq[g], ys[g], m.materials[m.element_material[e] - 1])
        out["stress"][g], out["strain"][g], out["eqps"][g], out["yield"][g] = r["sig"], r["eps"], r["eqps"], r["ys"]
        out["Qe"][e], out["volume"][e] = r["Qe"], r["V"]
        if r["q_minus_ys"][0] is not None:
            margin[g] = r["q_minus_ys"]
    return out, margin, els


def ulp_error(name, x, hp, elements):
    """E = max over the entries of the given elements of |x - hp| / (2^-53 * local scale); the local
    scale is the largest |hp| within the entry's own Gauss point (stress, strain: its 6 components;
    eqps, yield: the value itself) or element (Qe: its 24 components; volume: the value). An entry
    whose scale is 0 counts 0 if x equals hp and infinity otherwise."""
    x, hp = np.asarray(x, np.float64), np.asarray(hp, np.float64)
    els = np.asarray(list(elements), np.int64)
    if els.size == 0:
        return 0.0
    if name in ("Qe", "volume"):
        rows = els
    else:
        rows = (8 * els[:, None] + np.arange(8)[None, :]).reshape(-1)
    a, b = x[rows].reshape(rows.size, -1), hp[rows].reshape(rows.size, -1)
    scale = np.max(np.abs(b), axis=1, keepdims=True) * 2.0 ** -53
    diff = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(diff == 0, 0.0, diff / scale)
    return float(np.max(e))
