"""CPU proof of the reference-order element kernel's rewrites (elem_step_exact in
hakai-fem_amd/csrc/hakai_elem_exact.hpp), against the oracle's literal cal_stress_hexa
(oracle/hakai_oracle.c stress_one_element, v2/HAKAI_j.jl:1033-1371), BIT FOR BIT.

The kernel computes the reference's expressions with three rewrites that are exact by argument:
  * structural zeros of Bfinal (:1472-1490) and Dmat (:150-160) are dropped from the fma chains
    (fma(0, x, acc) == acc unless acc is a zero: only the sign of a zero intermediate can change)
    and the Jacobian sums start with their first product (0 + x == x up to the sign of a zero);
  * P2 = dN/dx is formed once per Gauss point for both cal_BVbar_hexa (1/|det|, weight |det|) and
    cal_Bfinal (1/det): (P2_abs/3)*|det| == (P2/3)*det exactly;
  * x/3 and a/b are correctly rounded without IEEE division sequences (div3, div_cr; their own
    check is tests/test_div3.py).
A C++ restatement of the kernel's arithmetic (one Gauss point after the other, the same operations
in the same order as the device lanes, g++ with fma and no contraction) is compared here with the
oracle on random elements AND on zero-rich ones (axis-aligned cubes whose Jacobians have exact
zero entries, zero displacement increments, zero stresses, +0/-0 inputs), where the dropped terms
meet zero accumulators. Every stored output must be bitwise identical, signed zeros included.
div3, div_cr and the hardening-segment search are not restated: the harness includes
hakai-fem_amd/csrc/hakai_exact_math.hpp, the header the kernel itself includes.
The GPU tests (tests/test_gpu_exact.py) then check the kernel itself against the oracle."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from hakai import mesh
import oracle as O
from util import bits, random_state, small_bar

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "hakai-fem_amd", "csrc")

SRC = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "hakai_exact_math.hpp" /* the kernel's own div3, div_cr, plastic_segment */
using hk::div3;
using hk::div_cr;

extern "C" {
/* One element, the kernel's arithmetic. pus[k][r][i] (192); X[i][3], du[i][3]; sig/eps [8][6],
   eqp/ys [8] in/out; Qe[24] out; mat: Dn, Do, Ds, G, npp, pl_eps[npp], Hd[npp-1]. */
void elem_exact(const double* pus, const double* X, const double* du, double* sig, double* eps, double* eqp,
                double* ys, double* Qe, double Dn, double Do, double Ds, double G, int npp, const double* pl_eps,
                const double* Hd, double* V_out) {
    double v[8], pd[8][8][3], fin[8][6];
    for (int k = 0; k < 8; ++k) {
        const double *P0 = pus + 24 * k, *P1 = P0 + 8, *P2 = P0 + 16;
        double J11 = P0[0] * X[0], J12 = P0[0] * X[1], J13 = P0[0] * X[2];
        double J21 = P1[0] * X[0], J22 = P1[0] * X[1], J23 = P1[0] * X[2];
        double J31 = P2[0] * X[0], J32 = P2[0] * X[1], J33 = P2[0] * X[2];
        for (int i = 1; i < 8; ++i) {
            const double X0 = X[3 * i], X1 = X[3 * i + 1], X2 = X[3 * i + 2];
            J11 += P0[i] * X0; J12 += P0[i] * X1; J13 += P0[i] * X2;
            J21 += P1[i] * X0; J22 += P1[i] * X1; J23 += P1[i] * X2;
            J31 += P2[i] * X0; J32 += P2[i] * X1; J33 += P2[i] * X2;
        }
        const double vv = J11 * J22 * J33 + J12 * J23 * J31 + J13 * J21 * J32 - J11 * J23 * J32 - J12 * J21 * J33 -
                          J13 * J22 * J31;
        const double div_v = 1.0 / vv;
        const double iJ11 = (J22 * J33 - J23 * J32) * div_v, iJ21 = (J23 * J31 - J21 * J33) * div_v;
        const double iJ31 = (J21 * J32 - J22 * J31) * div_v, iJ12 = (J13 * J32 - J12 * J33) * div_v;
        const double iJ22 = (J11 * J33 - J13 * J31) * div_v, iJ32 = (J12 * J31 - J11 * J32) * div_v;
        const double iJ13 = (J12 * J23 - J13 * J22) * div_v, iJ23 = (J13 * J21 - J11 * J23) * div_v;
        const double iJ33 = (J11 * J22 - J12 * J21) * div_v;
        for (int i = 0; i < 8; ++i) {
            pd[k][i][0] = iJ11 * P0[i] + iJ12 * P1[i] + iJ13 * P2[i];
            pd[k][i][1] = iJ21 * P0[i] + iJ22 * P1[i] + iJ23 * P2[i];
            pd[k][i][2] = iJ31 * P0[i] + iJ32 * P1[i] + iJ33 * P2[i];
        }
        v[k] = vv;
    }
    /* gp_all8 / gp_sum8: ordered over k from +0 */
    double V = 0.0 + fabs(v[0]);
    for (int k = 1; k < 8; ++k) V += fabs(v[k]);
    double bv[8][3];
    const double rV = 1.0 / V;
    for (int i = 0; i < 8; ++i)
        for (int c = 0; c < 3; ++c) {
            double s = 0.0 + div3(pd[0][i][c]) * v[0];
            for (int k = 1; k < 8; ++k) s += div3(pd[k][i][c]) * v[k];
            bv[i][c] = div_cr(s, V, rV);
        }
    double w[8][24];
    for (int k = 0; k < 8; ++k) {
        double de[6];
        for (int i = 0; i < 8; ++i) {
            const double u0 = du[3 * i], u1 = du[3 * i + 1], u2 = du[3 * i + 2];
            const double t0 = bv[i][0] - div3(pd[k][i][0]), t1 = bv[i][1] - div3(pd[k][i][1]),
                         t2 = bv[i][2] - div3(pd[k][i][2]);
            const double px = pd[k][i][0], py = pd[k][i][1], pz = pd[k][i][2];
            if (i == 0) {
                de[0] = (px + t0) * u0; de[1] = t0 * u0; de[2] = t0 * u0; de[3] = py * u0; de[4] = pz * u1;
                de[5] = pz * u0;
            } else {
                de[0] = fma(px + t0, u0, de[0]); de[1] = fma(t0, u0, de[1]); de[2] = fma(t0, u0, de[2]);
                de[3] = fma(py, u0, de[3]); de[5] = fma(pz, u0, de[5]); de[4] = fma(pz, u1, de[4]);
            }
            de[0] = fma(t1, u1, de[0]); de[1] = fma(py + t1, u1, de[1]); de[2] = fma(t1, u1, de[2]);
            de[3] = fma(px, u1, de[3]);
            de[0] = fma(t2, u2, de[0]); de[1] = fma(t2, u2, de[1]); de[2] = fma(pz + t2, u2, de[2]);
            de[4] = fma(py, u2, de[4]); de[5] = fma(px, u2, de[5]);
        }
        double* f = fin[k];
        const double* s0 = sig + 6 * k;
        f[0] = s0[0] + fma(Do, de[2], fma(Do, de[1], Dn * de[0]));
        f[1] = s0[1] + fma(Do, de[2], fma(Dn, de[1], Do * de[0]));
        f[2] = s0[2] + fma(Dn, de[2], fma(Do, de[1], Do * de[0]));
        f[3] = s0[3] + Ds * de[3];
        f[4] = s0[4] + Ds * de[4];
        f[5] = s0[5] + Ds * de[5];
        if (npp > 0) {
            const double mean = div3(f[0] + f[1] + f[2]);
            const double dev[6] = {f[0] - mean, f[1] - mean, f[2] - mean, f[3], f[4], f[5]};
            const double q = sqrt(1.5 * (dev[0] * dev[0] + dev[1] * dev[1] + dev[2] * dev[2] + 2.0 * (dev[3] * dev[3]) +
                                         2.0 * (dev[4] * dev[4]) + 2.0 * (dev[5] * dev[5])));
            if (q > ys[k]) {
                const double H = Hd[hk::plastic_segment(pl_eps, npp, eqp[k])];
                const double dep = (q - ys[k]) / (3.0 * G + H);
                const double s = ys[k] + H * dep;
                const double rq = 1.0 / q;
                for (int r = 0; r < 3; ++r) f[r] = div_cr(dev[r] * s, q, rq) + mean;
                for (int r = 3; r < 6; ++r) f[r] = div_cr(dev[r] * s, q, rq) + 0.0;
                eqp[k] = eqp[k] + dep;
                ys[k] = ys[k] + H * dep;
            }
        }
        for (int c = 0; c < 6; ++c) eps[6 * k + c] = eps[6 * k + c] + de[c];
        for (int i = 0; i < 8; ++i) {
            const double t0 = bv[i][0] - div3(pd[k][i][0]), t1 = bv[i][1] - div3(pd[k][i][1]),
                         t2 = bv[i][2] - div3(pd[k][i][2]);
            const double px = pd[k][i][0], py = pd[k][i][1], pz = pd[k][i][2];
            double a = (px + t0) * f[0];
            a = fma(t0, f[1], a); a = fma(t0, f[2], a); a = fma(py, f[3], a); a = fma(pz, f[5], a);
            w[k][3 * i] = v[k] * a;
            a = t1 * f[0];
            a = fma(py + t1, f[1], a); a = fma(t1, f[2], a); a = fma(px, f[3], a); a = fma(pz, f[4], a);
            w[k][3 * i + 1] = v[k] * a;
            a = t2 * f[0];
            a = fma(t2, f[1], a); a = fma(pz + t2, f[2], a); a = fma(py, f[4], a); a = fma(px, f[5], a);
            w[k][3 * i + 2] = v[k] * a;
        }
    }
    for (int j = 0; j < 24; ++j) {
        double s = 0.0 + w[0][j];
        for (int k = 1; k < 8; ++k) s += w[k][j];
        Qe[j] = s;
    }
    for (int k = 0; k < 8; ++k) memcpy(sig + 6 * k, fin[k], sizeof fin[k]);
    *V_out = V;
}
}
"""


@pytest.fixture(scope="module")
def emu(tmp_path_factory):
    d = tmp_path_factory.mktemp("exact")
    c, so = d / "exact.cpp", d / "exact.so"
    c.write_text(SRC)
    subprocess.run(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-mfma", "-shared", "-fPIC", "-I", CSRC,
                    "-o", str(so), str(c)], check=True)
    L = ctypes.CDLL(str(so))
    P = ctypes.c_void_p
    D = ctypes.c_double
    L.elem_exact.argtypes = [P, P, P, P, P, P, P, P, D, D, D, D, ctypes.c_int, P, P, P]
    return L


def _mat_consts(mt):
    """Dn, Do, Ds, G, pl_eps, Hd with the reference's host expressions (v2/HAKAI_j.jl:143-160,
    v2/readInpFile_j.jl:763-768), as the library and the oracle build them."""
    E, nu = mt.young, mt.poisson
    G = E / 2. / (1.0 + nu)
    c = E / (1.0 + nu) / (1.0 - 2.0 * nu)
    Dn, Do, Ds = c * (1.0 - nu), c * nu, c * ((1.0 - 2.0 * nu) / 2.0)
    pl = np.ascontiguousarray(mt.plastic, np.float64).reshape(-1, 2)
    npp = pl.shape[0]
    Hd = np.array([(pl[r + 1, 0] - pl[r, 0]) / (pl[r + 1, 1] - pl[r, 1]) for r in range(npp - 1)] or [0.0])
    return Dn, Do, Ds, G, npp, np.ascontiguousarray(pl[:, 1]) if npp else np.zeros(1), Hd


def _run_emu(L, m, pos, dd, st, sn, eq, ys):
    pus = np.zeros(192)
    O.lib().hko_pusai(pus.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    nE = m.nElement
    Qe = np.zeros((nE, 24))
    vol = np.zeros(nE)
    st, sn, eq, ys = st.copy(), sn.copy(), eq.copy(), ys.copy()
    for e in range(nE):
        mt = m.materials[m.element_material[e] - 1]
        Dn, Do, Ds, G, npp, ple, Hd = _mat_consts(mt)
        nodes = m.elementmat[e] - 1
        X = np.ascontiguousarray(pos[nodes])
        du = np.ascontiguousarray(dd.reshape(-1, 3)[nodes])
        s_e = np.ascontiguousarray(st[8 * e:8 * e + 8])
        n_e = np.ascontiguousarray(sn[8 * e:8 * e + 8])
        q_e = np.ascontiguousarray(eq[8 * e:8 * e + 8])
        y_e = np.ascontiguousarray(ys[8 * e:8 * e + 8])
        q = np.zeros(24)
        v = ctypes.c_double(0.0)
        L.elem_exact(pus.ctypes.data, X.ctypes.data, du.ctypes.data, s_e.ctypes.data, n_e.ctypes.data,
                     q_e.ctypes.data, y_e.ctypes.data, q.ctypes.data, Dn, Do, Ds, G, npp, ple.ctypes.data,
                     Hd.ctypes.data, ctypes.byref(v))
        st[8 * e:8 * e + 8], sn[8 * e:8 * e + 8], eq[8 * e:8 * e + 8], ys[8 * e:8 * e + 8] = s_e, n_e, q_e, y_e
        Qe[e] = q
        vol[e] = v.value
    return Qe, st, sn, eq, ys, vol


def _check(L, m, pos, dd, st, sn, eq, ys):
    o = O.Oracle(m)
    nE = m.nElement
    Qo = np.zeros((nE, 24))
    sto, sno, eqo, yso, vo = st.copy(), sn.copy(), eq.copy(), ys.copy(), np.zeros(nE)
    O.cal_stress_hexa(o, Qo, sto, sno, yso, eqo, np.ascontiguousarray(pos), dd, np.ones(nE, np.int64), vo)
    got = _run_emu(L, m, pos, dd, st, sn, eq, ys)
    for a, b, name in zip(got, (Qo, sto, sno, eqo, yso, vo), ("Qe", "stress", "strain", "eqps", "yield", "volume")):
        assert np.array_equal(bits(a), bits(b)), f"{name}: {np.max(np.abs(a - b))}"
    return got


@pytest.mark.parametrize("mat", ["ductile", "elastic"])
def test_random_elements(emu, mat):
    rng = np.random.default_rng(5)
    material = mesh.steel_ductile() if mat == "ductile" else mesh.steel_elastic()
    m = small_bar(4, 3, 6, material=material, perturb=0.05)
    st, sn, eq, ys = random_state(rng, m.nElement)
    pos = m.coordmat + rng.normal(0, 0.01, size=m.coordmat.shape)
    dd = rng.normal(0, 2e-3, size=3 * m.nNode)
    Qe, st2, _, eq2, _, _ = _check(emu, m, pos, dd, st, sn, eq, ys)
    if mat == "ductile":
        assert np.any(eq2 != eq)  # the radial return ran


def test_zero_rich_elements(emu):
    """Axis-aligned unit cubes (exact-zero Jacobian entries), zero and signed-zero displacement
    increments, zero and signed-zero stresses: the dropped structural-zero terms meet zero
    accumulators here, and the stored results must still be the oracle's bits."""
    rng = np.random.default_rng(7)
    m = small_bar(3, 2, 4, material=mesh.steel_ductile(), perturb=0.0)
    nE, nN = m.nElement, m.nNode
    pos = m.coordmat.copy()
    for case in range(6):
        dd = np.zeros(3 * nN)
        if case == 1:
            dd = -dd                                   # all -0
        elif case == 2:
            dd[2::3] = rng.normal(0, 1e-3, nN)          # only z moves
        elif case == 3:
            mask = rng.random(3 * nN) < 0.5
            dd[mask] = rng.normal(0, 1e-3, mask.sum())
            dd[~mask] = np.where(rng.random((~mask).sum()) < 0.5, 0.0, -0.0)
        elif case == 4:
            dd[0::3] = 1e-4                              # uniform x translation: de == 0 exactly?
        elif case == 5:
            dd = rng.normal(0, 2e-3, 3 * nN)
        st = np.zeros((8 * nE, 6))
        if case >= 3:
            st = rng.normal(0, 300, (8 * nE, 6))
            st[rng.random((8 * nE, 6)) < 0.3] = 0.0
        sn = np.zeros((8 * nE, 6))
        eq = np.zeros(8 * nE)
        ys = np.full(8 * nE, 755.0)
        _check(emu, m, pos, dd, st, sn, eq, ys)


def test_signed_zero_coordinates(emu):
    """Nodes on the coordinate planes stored as -0.0: products and Jacobian sums see -0 inputs."""
    m = small_bar(2, 2, 3, material=mesh.steel_ductile(), perturb=0.0)
    pos = m.coordmat.copy()
    pos[pos == 0.0] = -0.0
    rng = np.random.default_rng(9)
    dd = rng.normal(0, 1e-3, 3 * m.nNode)
    dd[rng.random(dd.size) < 0.3] = -0.0
    st, sn, eq, ys = random_state(rng, m.nElement)
    _check(emu, m, pos, dd, st, sn, eq, ys)
