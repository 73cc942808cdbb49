"""The element-set history (hakai_elem_history_*) on the CPU.

  * The arithmetic under test is the kernel's own: this file compiles
    hakai-fem_amd/csrc/hakai_elem_history_gp.hpp, the header hakai_elem_history.hip includes, and
    host/hakai_elem_history_host.cpp with a host compiler (no contraction).
  * Known answers on one unit cube with one Gauss-point state repeated: uniaxial stress s gives
    w_e = s^2 / (2E), hydrostatic p gives p^2 / (2K), pure shear tau gives tau^2 / (2G). The energy
    density takes about 12 operations from the stress and the sum over 8 equal points is exact up to
    the weights' roundings (about 30 operations in a_k): SE agrees with V times the formula to 64 u.
  * w_p against trapezoid areas in exact rationals (fractions) on the Tensile5e hardening table. All
    terms are positive, so relative errors add: a yield value y_j carries at most 4 roundings per
    segment walked (Hd, d, the product, the sum), a trapezoid 3 more (d, y + yn, the product; the
    halving is exact) and the running sum one per segment: (5 nseg + 4) u relative in all.
  * elem_history_ref (NumPy, the header's operation order) equals the compiled header BIT FOR BIT on
    random states on small_bar, a sheared and an inverted mesh.
  * hakai_elem_history_combine, the CSV round trip, the reader's element sets.
  * The energy gap (test_energy_gap_measured): on the oracle's trajectory of small_bar, 400 steps,
    max_k |W_int - (SE + PD)| / max_k W_int is 2.01e-02 (plastic; steel_ductile) and 8.01e-02
    (elastic). SE + PD is not W_int (the header comment of hakai_elem_history_gp.hpp lists why); the
    values are measured, deterministic for a given oracle build, and asserted with a factor 1.5."""
import ctypes
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import edge_cases
import elem_history_ref as R
from hakai import mesh
from hakai.solver import elem_history_combine, read_elem_history_csv, write_elem_history_csv
from history_ref import HistoryRef, prescribed_mask
from util import bitwise_equal, random_state, small_bar

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hakai-fem_amd")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC"]
U = 2.0 ** -53
GAP_PLASTIC, GAP_ELASTIC = 2.01e-02, 8.01e-02   # measured (module docstring)

# The harness only calls the header's functions; the host file is compiled as it is.
SRC = r"""
#include <stdint.h>
#include <stdarg.h>
#include <stdio.h>
#include "hakai_elem_history_gp.hpp"
namespace hkc {
char g_msg[512];
int fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return code;
}
}
extern "C" {
int mat_size() { return (int)sizeof(hk::ElemHistMat); }
void mat_make(double Dn, double Do, double G, double y0, int npp, const double* pe, const double* Hd, void* o) {
    *(hk::ElemHistMat*)o = hk::elem_hist_mat(Dn, Do, G, y0, npp, pe, Hd);
}
void mat_get(const void* m, double* o) {
    o[0] = ((const hk::ElemHistMat*)m)->G6;
    o[1] = ((const hk::ElemHistMat*)m)->K2;
}
double wp(double e, const void* m) { return hk::elem_hist_wp(e, *(const hk::ElemHistMat*)m); }
/* x, X: [n][8][3]; sig, eps: [n][8][6]; eqps: [n][8]; mats: the table; mat: [n]; out: [n][20] */
void run(const double* x, const double* X, const double* sig, const double* eps, const double* eqps,
         const void* mats, const int64_t* mat, int64_t n, double* out) {
    for (int64_t e = 0; e < n; ++e) {
        double a[8][3], b[8][3], s[8][6], t[8][6], q[8], o[hk::kEhElem];
        for (int i = 0; i < 8; ++i) {
            for (int c = 0; c < 3; ++c) {
                a[i][c] = x[24 * e + 3 * i + c];
                b[i][c] = X[24 * e + 3 * i + c];
            }
            for (int c = 0; c < 6; ++c) {
                s[i][c] = sig[48 * e + 6 * i + c];
                t[i][c] = eps[48 * e + 6 * i + c];
            }
            q[i] = eqps[8 * e + i];
        }
        hk::elem_hist_element(a, b, s, t, q, ((const hk::ElemHistMat*)mats)[mat[e]], o);
        for (int j = 0; j < hk::kEhElem; ++j) out[hk::kEhElem * e + j] = o[j];
    }
}
}
"""


class Header:
    def __init__(self, lib):
        self.lib = lib
        P, D, I = ctypes.c_void_p, ctypes.c_double, ctypes.c_int
        lib.mat_make.argtypes = [D, D, D, D, I, P, P, P]
        lib.mat_get.argtypes = [P, P]
        lib.wp.argtypes = [D, P]
        lib.wp.restype = D
        lib.run.argtypes = [P, P, P, P, P, P, P, ctypes.c_int64, P]
        lib.mat_make.restype = lib.mat_get.restype = lib.run.restype = None
        self.msize = lib.mat_size()

    def mats(self, materials):
        """The header's material table (bytes) of hakai Materials, from build_devmat's constants."""
        buf = np.zeros(self.msize * len(materials), np.uint8)
        for i, mt in enumerate(materials):
            young, poisson = np.float64(mt.young), np.float64(mt.poisson)
            cc = young / (1.0 + poisson) / (1.0 - 2.0 * poisson)
            Dn, Do, G = cc * (1.0 - poisson), cc * poisson, young / 2. / (1.0 + poisson)
            pl = np.asarray(mt.plastic, np.float64).reshape(-1, 2)
            self.table(buf[i * self.msize:], Dn, Do, G, pl)
        return buf

    def table(self, buf, Dn, Do, G, pl):
        pl = np.asarray(pl, np.float64).reshape(-1, 2)
        npp = pl.shape[0]
        pe = np.ascontiguousarray(pl[:, 1]) if npp else np.zeros(1)
        Hd = np.array([(pl[r + 1, 0] - pl[r, 0]) / (pl[r + 1, 1] - pl[r, 1]) for r in range(npp - 1)] + [0.0])
        self.lib.mat_make(Dn, Do, G, pl[0, 0] if npp else 0.0, npp, pe.ctypes.data, Hd.ctypes.data, buf.ctypes.data)
        return buf

    def elements(self, x, X, sig, eps, eqps, mats, mat_id):
        x, X, sig, eps, eqps = (np.ascontiguousarray(a, np.float64) for a in (x, X, sig, eps, eqps))
        mat_id = np.ascontiguousarray(mat_id, np.int64)
        n = x.shape[0]
        out = np.zeros((n, 20))
        self.lib.run(x.ctypes.data, X.ctypes.data, sig.ctypes.data, eps.ctypes.data, eqps.ctypes.data, mats.ctypes.data,
                     mat_id.ctypes.data, n, out.ctypes.data)
        return out


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    d = tmp_path_factory.mktemp("elem_history")
    c, so = d / "elem_history.cpp", d / "elem_history.so"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", os.path.join(PKG, "csrc"), "-o", str(so), str(c),
                    os.path.join(PKG, "host", "hakai_elem_history_host.cpp")], check=True)
    return Header(ctypes.CDLL(str(so)))


CUBE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)


# ---- known answers ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["uniaxial", "hydrostatic", "shear"])
def test_known_energy_densities(H, kind):
    mt = mesh.steel_ductile()
    E, nu = mt.young, mt.poisson
    K, G = E / (3 * (1 - 2 * nu)), E / (2 * (1 + nu))
    s = {"uniaxial": [0, 0, 317.0, 0, 0, 0], "hydrostatic": [-123.0] * 3 + [0] * 3, "shear": [0, 0, 0, 0, 77.5, 0]}[kind]
    want = {"uniaxial": 317.0 ** 2 / (2 * E), "hydrostatic": 123.0 ** 2 / (2 * K), "shear": 77.5 ** 2 / (2 * G)}[kind]
    sig = np.tile(np.array(s, np.float64), (1, 8, 1))
    pe = H.elements(CUBE[None], CUBE[None], sig, np.zeros((1, 8, 6)), np.zeros((1, 8)), H.mats([mt]), [0])[0]
    V, V0, SE, PD = pe[0], pe[1], pe[15], pe[16]
    assert abs(V - 1.0) <= 64 * U and bitwise_equal(V, V0) and PD == 0.0 and pe[19] == 1.0
    assert abs(SE - want * V) <= 64 * U * want
    q = {"uniaxial": 317.0, "hydrostatic": 0.0, "shear": math.sqrt(3) * 77.5}[kind]
    assert abs(pe[18] - q) <= 8 * U * max(q, 1.0) and pe[17] == 0.0
    assert np.all(np.abs(pe[2:8] - np.array(s) * V) <= 64 * U * np.abs(s))


def exact_wp(e, pl):
    """The area under the piecewise linear curve through the table rows from the first row's strain
    to e, the last segment continued, in exact rationals."""
    pl = [(Fraction(float(y)), Fraction(float(x))) for y, x in np.asarray(pl).reshape(-1, 2)]
    e = Fraction(float(e))
    if not pl or e <= pl[0][1]:
        return Fraction(0)
    if len(pl) == 1:
        return pl[0][0] * (e - pl[0][1])
    w = Fraction(0)
    for j in range(len(pl) - 1):
        (y0, x0), (y1, x1) = pl[j], pl[j + 1]
        last = j == len(pl) - 2
        hi = e if (last or e <= x1) else x1
        ye = y0 + (y1 - y0) / (x1 - x0) * (hi - x0)
        w += (y0 + ye) / 2 * (hi - x0)
        if hi == e:
            break
    return w


def test_wp_against_exact_trapezoids(H):
    pl = mesh.STEEL_PLASTIC
    buf = H.table(np.zeros(H.msize, np.uint8), 1.0, 1.0, 1.0, pl)
    ref = R.table_consts(6.0, 2.0, pl)
    pts = [0.0, 5e-324, 0.005, 5.0, 40.0]
    for x in pl[:, 1]:
        pts += [x, np.nextafter(x, -np.inf), np.nextafter(x, np.inf)]
    nseg = len(pl) - 1
    for e in pts:
        got, want = H.lib.wp(float(e), buf.ctypes.data), exact_wp(e, pl)
        assert bitwise_equal(got, R.wp(np.array([e]), ref)[0]), e
        assert abs(Fraction(got) - want) <= (5 * nseg + 4) * Fraction(U) * want, (e, got, float(want))
        assert got >= 0.0 and (got > 0.0) == (e > 0.0)
    elastic = H.table(np.zeros(H.msize, np.uint8), 1.0, 1.0, 1.0, np.zeros((0, 2)))
    assert H.lib.wp(0.3, elastic.ctypes.data) == 0.0
    one = H.table(np.zeros(H.msize, np.uint8), 1.0, 1.0, 1.0, [[755.0, 0.0]])      # one row: perfectly plastic
    for e in (0.0, 0.25, 3.0):
        assert abs(Fraction(H.lib.wp(e, one.ctypes.data)) - exact_wp(e, [[755.0, 0.0]])) <= 4 * Fraction(U) * 755 * 3
        assert bitwise_equal(H.lib.wp(e, one.ctypes.data), R.wp(np.array([e]), R.table_consts(6.0, 2.0, [[755.0, 0.0]]))[0])


# ---- header == NumPy, bit for bit -------------------------------------------------------------------
def mesh_case(kind):
    if kind == "small_bar":
        m = small_bar()
        rng = np.random.default_rng(11)
        pos = m.coordmat + rng.normal(0, 0.03, size=m.coordmat.shape)
    else:
        c = edge_cases.shape_case(kind)
        m, pos = c["m"], c["pos"]
    return m, np.ascontiguousarray(pos)


@pytest.mark.parametrize("kind", ["small_bar", "sheared", "inverted"])
def test_restatement_bitwise(H, kind):
    m, pos = mesh_case(kind)
    nE = m.nElement
    st, sn, eq, _ = random_state(np.random.default_rng(7), nE)
    eq[::5] = mesh.STEEL_PLASTIC[1 + (np.arange(len(eq[::5])) % 7), 1]    # some exactly on a breakpoint
    st[3] = -0.0
    st[4] = 5e-310                                                        # a subnormal stress
    n = m.elementmat - 1
    mats = list(m.materials)
    re_ = R.model_elements(m, (pos - m.coordmat).ravel(), st, sn, eq)
    # (the restatement forms x = coord + disp: give the header the same sum)
    x = (m.coordmat + (pos - m.coordmat))[n]
    he = H.elements(x, m.coordmat[n], st.reshape(nE, 8, 6), sn.reshape(nE, 8, 6), eq.reshape(nE, 8), H.mats(mats),
                    m.element_material - 1)
    assert bitwise_equal(he, re_), kind
    assert np.all(he[:, 0] >= 0) and np.all(he[:, 1] > 0) and np.all(he[:, 17] >= 0) and np.all(he[:, 18] >= 0)
    if len(np.asarray(m.materials[0].plastic).ravel()):
        assert np.any(he[:, 16] > 0)
    g, tab = np.zeros(2), H.mats(mats)
    H.lib.mat_get(tab.ctypes.data, g.ctypes.data)
    assert bitwise_equal(g, np.array(R.mat_consts(m.materials[0])[:2]))


# ---- combine ----------------------------------------------------------------------------------------
def part(steps, values):
    return dict(steps=np.asarray(steps, np.int64), values=np.asarray(values, np.float64))


def test_combine(H):
    rng = np.random.default_rng(2)
    n, S = 3, 2
    v = rng.normal(0, 1e3, size=(3, n, S, 24))
    v[..., 0:2] = rng.integers(0, 50, size=(3, n, S, 2))
    v[..., 19] = np.abs(v[..., 19])
    v[..., 21] = np.abs(v[..., 21])
    v[..., 20] = rng.integers(1, 1000, size=(3, n, S))
    v[..., 22] = rng.integers(1, 1000, size=(3, n, S))
    v[..., 23] = np.abs(v[..., 23])
    v[0, 0, 0, 19] = v[1, 0, 0, 19] = v[2, 0, 0, 19] = 7.0                     # a tie over three ranks
    v[0, 0, 0, 20], v[1, 0, 0, 20], v[2, 0, 0, 20] = 40.0, 12.0, 90.0
    v[0, 1, 1, 19:24] = (0.0, 0.0, 0.0, 0.0, np.inf)                           # rank 0: the set has no active element
    v[1, 1, 1, 19:21] = (0.0, 5.0)                                             # rank 1: one with eqps 0
    v[2, 2, 1, 0:24] = 0.0                                                     # record 2, set 1: empty on every rank
    v[0, 2, 1, 0:24] = v[1, 2, 1, 0:24] = 0.0
    v[:, 2, 1, 23] = np.inf
    steps = [0, 7, 14]
    parts = [part(steps, v[r]) for r in range(3)]
    one = elem_history_combine(parts[:1])
    assert bitwise_equal(one["values"], v[0]) and np.array_equal(one["steps"], steps)       # one rank: the identity
    c = elem_history_combine(parts)
    assert bitwise_equal(c["values"][..., :19], (v[0] + v[1] + v[2])[..., :19])              # ((p0 + p1) + p2)
    assert not bitwise_equal(c["values"][..., 2:19], (v[0] + (v[1] + v[2]))[..., 2:19])
    assert tuple(c["values"][0, 0, 19:21]) == (7.0, 12.0)                                    # a tie takes the lower id
    assert c["values"][1, 1, 20] != 0.0 and (c["values"][1, 1, 19], c["values"][1, 1, 20]) == max(
        [(v[r, 1, 1, 19], v[r, 1, 1, 20]) for r in (1, 2)], key=lambda t: (t[0], -t[1]))
    assert np.all(c["values"][2, 1, :23] == 0.0) and c["values"][2, 1, 23] == np.inf        # the empty set's sentinels
    assert bitwise_equal(c["values"][..., 23], v[..., 23].min(axis=0))
    for i in range(n):
        for s in range(S):
            for f in (19, 21):
                cand = [(v[r, i, s, f], -v[r, i, s, f + 1]) for r in range(3) if v[r, i, s, f + 1] > 0]
                if cand:
                    b = max(cand)
                    assert (c["values"][i, s, f], c["values"][i, s, f + 1]) == (b[0], -b[1])
    # mismatched steps: refused, the outputs untouched
    lib = H.lib
    st = np.array([[0, 7, 14], [0, 7, 15]], np.int64)
    vv = np.ascontiguousarray(v[:2])
    so, vo = np.full(3, -5, np.int64), np.full((n, S, 24), -5.0)
    lib.hakai_elem_history_combine.argtypes = [ctypes.c_int32, ctypes.c_int32, ctypes.c_int64] + [ctypes.c_void_p] * 4
    rc = lib.hakai_elem_history_combine(2, S, n, st.ctypes.data, vv.ctypes.data, so.ctypes.data, vo.ctypes.data)
    assert rc != 0 and np.all(so == -5) and np.all(vo == -5.0)
    assert lib.hakai_elem_history_combine(0, S, n, st.ctypes.data, vv.ctypes.data, so.ctypes.data, vo.ctypes.data) != 0
    assert lib.hakai_elem_history_combine(2, 17, n, st.ctypes.data, vv.ctypes.data, so.ctypes.data, vo.ctypes.data) != 0
    assert lib.hakai_elem_history_combine(2, S, n, None, vv.ctypes.data, so.ctypes.data, vo.ctypes.data) != 0
    assert np.all(so == -5) and np.all(vo == -5.0)


def test_csv_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    v = rng.normal(0, 1, size=(5, 3, 24)) * 10.0 ** rng.integers(-300, 300, size=(5, 3, 24))
    v[0, 0, 23] = np.inf
    v[1, 1, 5] = -0.0
    steps = np.arange(5) * 10
    p = tmp_path / "elem_history.csv"
    write_elem_history_csv(str(p), ["all", "inst1", "Part-1.grip"], steps, v, 1e-7)
    r = read_elem_history_csv(str(p))
    assert r["sets"] == ["all", "inst1", "Part-1.grip"] and np.array_equal(r["steps"], steps)
    assert bitwise_equal(r["values"], v) and bitwise_equal(r["time"], steps * 1e-7)
    head = open(p).readline().strip().split(",")
    assert head[:2] == ["step", "time"] and head[2:26] == ["all_" + f for f in R.FIELDS]


# ---- the reader's element sets ------------------------------------------------------------------------
def test_reader_element_sets(tmp_path):
    """Two instances, two materials, 13 *Elset ... instance= sets (lists, with and without `internal`,
    and `generate`): 17 candidates after "all", the last two reported dropped; ids global, 1-based."""
    import dataclasses
    import hakai
    from inp_writer import write_inp
    m0 = mesh.two_body_model(plate=(5, 5, 2), impactor=(3, 3, 2), v=-1e5, n_steps=300)
    n1 = 50
    assert m0.nElement == 68 and np.all(m0.element_instance[:n1] == 1) and np.all(m0.element_instance[n1:] == 2)
    emat = np.where(m0.element_instance == 1, 1, 2).astype(np.int64)
    m0 = dataclasses.replace(m0, materials=[mesh.steel_ductile(), mesh.steel_elastic()], element_material=emat)
    deck = write_inp(str(tmp_path / "sets.inp"), m0)
    lines, want = [], []
    for j in range(13):
        inst, e0 = (1, 0) if j % 2 == 0 else (2, n1)
        if j % 3 == 0:
            loc = [3 + j, 1, 2 + j]                                     # a list, unordered
            lines.append(f"*Elset, elset=Set-{j}, instance=P{inst}-1\n" + ", ".join(map(str, loc)) + "\n")
        elif j % 3 == 1:
            loc = [5, 6, 7 + j % 5]
            lines.append(f"*Elset, elset=Set-{j}, internal, instance=P{inst}-1\n" + ", ".join(map(str, loc)) + "\n")
        else:
            loc = list(range(2, 15, 3))
            lines.append(f"*Elset, elset=Set-{j}, instance=P{inst}-1, generate\n 2, 14, 3\n")
        want.append((f"P{inst}-1.Set-{j}", np.sort(np.array(loc)) + e0))
    text = open(deck).read()
    assert text.count("*End Assembly\n") == 1
    open(deck, "w").write(text.replace("*End Assembly\n", "".join(lines) + "*End Assembly\n"))
    m = hakai.read_inp(deck)
    names, sets, dropped = m.elem_history_sets
    assert names == ["all", "inst1", "inst2", "mat1", "mat2"] + [w[0] for w in want[:11]]
    assert dropped == [w[0] for w in want[11:]] and len(sets) == 15
    assert np.array_equal(sets[0], np.arange(1, n1 + 1)) and np.array_equal(sets[1], np.arange(n1 + 1, 69))
    assert np.array_equal(sets[2], sets[0]) and np.array_equal(sets[3], sets[1])
    for s, (_, ids) in zip(sets[4:], want):
        assert np.array_equal(s, ids)
    # the model itself is as before
    assert m.nElement == 68 and np.array_equal(m.elementmat, m0.elementmat)
    # room checks of the accessor
    L = hakai.lib()
    import ctypes as C
    from hakai import _abi
    out = C.POINTER(_abi.InpModelT)()
    _abi.check(L.hakai_inp_read(deck.encode(), C.byref(out)))
    try:
        ns, nd = C.c_int32(0), C.c_int32(0)
        off, el = np.zeros(16, np.int64), np.zeros(4, np.int64)
        assert L.hakai_inp_elem_history_sets(out, C.byref(ns), _abi.ptr(off, C.c_int64), _abi.ptr(el, C.c_int64), 4, None,
                                             0, C.byref(nd)) == _abi.HAKAI_ERR_ARG
        assert L.hakai_inp_elem_history_sets(out, C.byref(ns), _abi.ptr(off, C.c_int64), None, 0, C.create_string_buffer(8),
                                             8, C.byref(nd)) == _abi.HAKAI_ERR_ARG
        assert L.hakai_inp_elem_history_sets(out, C.byref(ns), _abi.ptr(off, C.c_int64), None, 0, None, 0,
                                             C.byref(nd)) == 0 and (ns.value, nd.value) == (15, 2)
    finally:
        L.hakai_inp_free(out)


# ---- the energy gap, measured -------------------------------------------------------------------------
def energy_history(m, n_steps):
    """Per state k = 0 .. n_steps-1 of the oracle's trajectory: W_int of history_ref's set 0 and SE, PD
    of the restatement's set 0."""
    import oracle as O
    o = O.Oracle(m)
    ref = HistoryRef(o.diag_M, prescribed_mask(m), [], m.dt)
    ref.seed(o.s["disp"], o.s["disp_pre"])
    W, SE, PD = [], [], []
    for t in range(1, n_steps + 1):
        disp, Q = o.s["disp"].copy(), o.s["Q"].copy()
        pe = R.model_elements(m, disp, o.s["integ_stress"], o.s["integ_strain"], o.s["integ_eq_plastic_strain"])
        val, _ = R.record(pe, o.s["element_flag"], np.zeros(m.nElement, bool), [])
        o.run(t, 1)
        v, _ = ref.step(o.s["disp"], disp, Q)
        W.append(v[0, 10])
        SE.append(val[0, 17])
        PD.append(val[0, 18])
    return np.array(W), np.array(SE), np.array(PD)


def test_energy_gap_measured():
    """max_k |W_int - (SE + PD)| / max_k W_int on small_bar, 400 steps of the oracle: 2.01e-02 plastic,
    8.01e-02 elastic (measured; asserted with a factor 1.5, which only has to cover the fma / no-fma
    freedom of the oracle build, bounded at 1e-10 on such decks)."""
    gaps = {}
    for name, mt in (("plastic", None), ("elastic", mesh.steel_elastic())):
        m = small_bar(material=mt)
        W, SE, PD = energy_history(m, 400)
        gaps[name] = float(np.max(np.abs(W - (SE + PD))) / np.max(W))
        if name == "plastic":
            assert PD[-1] > 0.0 and np.all(np.diff(PD) >= 0.0)
        else:
            assert np.all(PD == 0.0)
    print("energy gap:", gaps)
    assert gaps["plastic"] <= 1.5 * GAP_PLASTIC and gaps["elastic"] <= 1.5 * GAP_ELASTIC
    assert gaps["plastic"] >= GAP_PLASTIC / 1.5 and gaps["elastic"] >= GAP_ELASTIC / 1.5
