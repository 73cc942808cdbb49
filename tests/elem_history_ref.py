"""NumPy float64 restatement of hakai-fem_amd/csrc/hakai_elem_history_gp.hpp -- TEST INFRASTRUCTURE.

The element-set history's per-element values vectorised over elements, in the header's operation
order: every sum, product and division below is the header's, one rounding each, so the header
compiled for the host (tests/test_elem_history_cpu.py) and the kernel (tests/test_gpu_elem_history.py)
must give the same bits. Then the set record from per-element values: counts, extremes and ids exactly,
the sums as exactly rounded sums (math.fsum) next to the sum of the terms' magnitudes, which scales the
error bound of a floating-point summation of the same terms. No GPU, no library."""
import math

import numpy as np

import numpy_ref

NF = 24
NE = 20
U = 2.0 ** -53
SUMS = list(range(2, 19))        # record fields that are floating-point sums
EXACT = [0, 1, 19, 20, 21, 22, 23]
FIELDS = ("N_active", "N_deleted", "V", "V0", "S_xx", "S_yy", "S_zz", "S_xy", "S_yz", "S_zx", "E_xx", "E_yy", "E_zz",
          "E_xy", "E_yz", "E_zx", "EQ", "SE", "PD", "eqps_max", "eqps_max_elem", "mises_max", "mises_max_elem", "J_min")


def mat_consts(mt):
    """(G6, K2, yield0, npp, pl_eps, Hd) of a hakai.model.Material: build_devmat's and elem_hist_mat's
    operation order."""
    young, poisson = np.float64(mt.young), np.float64(mt.poisson)
    d1, d2 = 1.0 - poisson, poisson
    cc = young / (1.0 + poisson) / (1.0 - 2.0 * poisson)
    Dn, Do = cc * d1, cc * d2
    G = young / 2. / (1.0 + poisson)
    pl = np.asarray(mt.plastic if mt.plastic is not None else np.zeros((0, 2)), np.float64).reshape(-1, 2)
    return table_consts(6.0 * G, 2.0 * ((Dn + 2.0 * Do) / 3.0), pl)


def table_consts(G6, K2, pl):
    """The same from a *Plastic table (rows yield stress, plastic strain)."""
    pl = np.asarray(pl, np.float64).reshape(-1, 2)
    npp = pl.shape[0]
    Hd = np.array([(pl[r + 1, 0] - pl[r, 0]) / (pl[r + 1, 1] - pl[r, 1]) for r in range(npp - 1)])
    return np.float64(G6), np.float64(K2), np.float64(pl[0, 0] if npp else 0.0), npp, pl[:, 1].copy(), Hd


def wp(e, mat):
    """elem_hist_wp over an array of strains: the segment walk, whole segments then the one holding e."""
    _, _, y0, npp, pe, Hd = mat
    e = np.asarray(e, np.float64)
    w = np.zeros_like(e)
    if npp <= 0:
        return w
    nseg = npp - 1 if npp > 1 else 1
    y = np.full_like(e, y0)
    live = np.ones(e.shape, bool)
    for j in range(nseg):
        lo = pe[j]
        H = Hd[j] if npp > 1 else 0.0
        whole = (e > pe[j + 1]) if j + 1 < nseg else np.zeros(e.shape, bool)
        d = np.where(whole, pe[j + 1] if j + 1 < nseg else 0.0, e) - lo
        add = live & (d > 0.0)
        yn = y + H * d
        w = np.where(add, w + (0.5 * (y + yn)) * d, w)
        y = np.where(add, yn, y)
        live = live & whole
    return w


def q2(s):
    d0, d1, d2 = s[..., 0] - s[..., 1], s[..., 1] - s[..., 2], s[..., 2] - s[..., 0]
    n = (d0 * d0 + d1 * d1) + d2 * d2
    t = (s[..., 3] * s[..., 3] + s[..., 4] * s[..., 4]) + s[..., 5] * s[..., 5]
    return 0.5 * n + 3.0 * t


def we(s, mat):
    p = ((s[..., 0] + s[..., 1]) + s[..., 2]) / 3.0
    return q2(s) / mat[0] + (p * p) / mat[1]


def _det(P, x):
    acc = [[None] * 3 for _ in range(3)]
    for a in range(3):
        for b in range(3):
            v = P[a, 0] * x[:, 0, b]
            for i in range(1, 8):
                v = v + P[a, i] * x[:, i, b]
            acc[a][b] = v
    J = acc
    return (J[0][0] * J[1][1] * J[2][2] + J[0][1] * J[1][2] * J[2][0] + J[0][2] * J[1][0] * J[2][1] -
            J[0][0] * J[1][2] * J[2][1] - J[0][1] * J[1][0] * J[2][2] - J[0][2] * J[1][1] * J[2][0])


def elements(x, X, sig, eps, eqps, mats, mat_id):
    """(n, 20) per-element values. x, X: (n, 8, 3); sig, eps: (n, 8, 6); eqps: (n, 8); mats: a list of
    mat_consts tuples; mat_id: (n,) 0-based."""
    x, X = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(X, np.float64)
    sig, eps, eqps = (np.asarray(a, np.float64) for a in (sig, eps, eqps))
    n = x.shape[0]
    mat_id = np.asarray(mat_id)
    P = numpy_ref.pusai()
    t = np.zeros((8, 19, n))
    with np.errstate(all="ignore"):
        for k in range(8):
            det, det0 = _det(P[k], x), _det(P[k], X)
            a, a0 = np.where(det < 0.0, -det, det), np.where(det0 < 0.0, -det0, det0)
            t[k, 0], t[k, 1] = a, a0
            for c in range(6):
                t[k, 2 + c] = a * sig[:, k, c]
                t[k, 8 + c] = a * eps[:, k, c]
            t[k, 14] = a * eqps[:, k]
            qq = q2(sig[:, k])
            w_e, w_p = np.zeros(n), np.zeros(n)
            for i, m in enumerate(mats):
                sel = mat_id == i
                w_e[sel] = we(sig[sel, k], m)
                w_p[sel] = wp(eqps[sel, k], m)
            t[k, 15] = a * w_e
            t[k, 16] = a0 * w_p
            t[k, 17] = eqps[:, k]
            t[k, 18] = np.sqrt(qq)
        out = np.zeros((n, NE))
        S = ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))
        out[:, :17] = S[:17].T
        for j in (17, 18):
            m = np.zeros(n)
            for k in range(8):
                m = np.where(t[k, j] > m, t[k, j], m)
            out[:, j] = m
        out[:, 19] = out[:, 0] / out[:, 1]
    return out


def model_elements(m, disp, integ_stress, integ_strain, integ_eqps):
    """elements() of a hakai Model at a reference-layout state (disp 3nN, integ_* (8nE, ...))."""
    n = m.elementmat - 1
    nE = m.nElement
    X = m.coordmat[n]
    x = (m.coordmat + np.asarray(disp).reshape(-1, 3))[n]
    return elements(x, X, np.asarray(integ_stress).reshape(nE, 8, 6), np.asarray(integ_strain).reshape(nE, 8, 6),
                    np.asarray(integ_eqps).reshape(nE, 8), [mat_consts(mt) for mt in m.materials],
                    m.element_material - 1)


def fsum(a):
    return math.fsum(np.asarray(a, np.float64).ravel().tolist())


def record(pe, flag, deleted, sets, elem_offset=0):
    """The set record (S, 24) and the sums' magnitudes (S, 24) from per-element values pe (nE, 20),
    flag (nE,) (1 = active), deleted (nE,) bool and the caller's sets (1-based ids; set 0 = every
    element is added in front)."""
    nE = pe.shape[0]
    flag, deleted = np.asarray(flag), np.asarray(deleted, bool)
    sets = [np.arange(nE)] + [np.asarray(s, np.int64).ravel() - 1 for s in sets]
    val, mag = np.zeros((len(sets), NF)), np.zeros((len(sets), NF))
    for s, idx in enumerate(sets):
        idx = np.sort(idx)
        act = idx[flag[idx] == 1]
        val[s, 0], val[s, 1] = len(act), int(np.sum(deleted[idx]))
        for j in range(17):
            val[s, 2 + j] = fsum(pe[act, j])
            mag[s, 2 + j] = fsum(np.abs(pe[act, j]))
        val[s, 23] = np.inf
        if len(act):
            for f, j in ((19, 17), (21, 18)):
                v = pe[act, j]
                i = int(np.argmax(v))             # the first of equals: the lowest id
                val[s, f], val[s, f + 1] = v[i], act[i] + 1 + elem_offset
            J = pe[act, 19]
            J = J[J < np.inf]
            val[s, 23] = J.min() if len(J) else np.inf
    return val, mag


def tree_depth(nE):
    """Additions on the longest path of the kernel's tree over nE elements: 3 in a wave, 2 over the
    block's waves, then ceil(log2) over the 32-element chunks."""
    chunks = max(1, (nE + 31) // 32)
    return 5 + max(0, math.ceil(math.log2(chunks)))
