"""External loads (hakai_set_loads) on the CPU.

  * The arithmetic under test is the kernel's own: this file compiles
    hakai-fem_amd/csrc/hakai_loads_face.hpp (the header hakai_loads.hip includes) and the host planner
    hakai_loads_plan.cpp into a small stand-alone program (its own main, built with
    -fsanitize=address,undefined and no contraction) and holds both against loads_ref BIT FOR BIT:
    the face forces and the amplitude rule on random and special inputs, the planner's per-node lists
    on meshes with shared, repeated and interior faces, and each of the planner's refusals.
  * loads_ref itself is held against exact rationals (fractions.Fraction) on warped faces, within
    the rounding bound loads_ref's docstring derives from the operation count (9 u |pa| D^2).
  * Known answers, all exact: the six faces of a unit cube with dyadic coordinates give
    -p A n_out in quarters; on a parallelogram the h terms vanish and the corners share the load
    equally; the four corner forces sum to p times the area vector; the exact-rational forces of ALL
    exterior faces of a perturbed 2x2x2 bar at uniform p sum to exactly zero (a closed surface
    balances)."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import loads_ref as R
from hakai import mesh
from hakai.model import Loads, Model
from util import bitwise_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
CXXFLAGS = ["-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined"]

# The harness only moves bytes: it calls the header's and the planner's functions.
SRC = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "hakai_loads_face.hpp"
#include "hakai_loads_plan.hpp"

static std::vector<char> in;
static size_t at = 0;
template <class T> static std::vector<T> take(size_t n) {
    std::vector<T> v(n);
    if (at + n * sizeof(T) > in.size()) { std::fprintf(stderr, "short input\n"); std::exit(3); }
    if (n) std::memcpy(v.data(), in.data() + at, n * sizeof(T));
    at += n * sizeof(T);
    return v;
}
template <class T> static void put(FILE* f, const std::vector<T>& v) {
    const int64_t n = (int64_t)v.size();
    std::fwrite(&n, sizeof n, 1, f);
    if (n) std::fwrite(v.data(), sizeof(T), v.size(), f);
}

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    FILE* fi = std::fopen(argv[2], "rb");
    if (!fi) return 2;
    char buf[1 << 16];
    size_t got;
    while ((got = std::fread(buf, 1, sizeof buf, fi)) > 0) in.insert(in.end(), buf, buf + got);
    std::fclose(fi);
    FILE* fo = std::fopen(argv[3], "wb");
    if (!fo) return 2;
    const std::string mode = argv[1];
    if (mode == "face") {  // n; x[n][4][3]; pa[n] -> F[n][4][3]
        const int64_t n = take<int64_t>(1)[0];
        const std::vector<double> x = take<double>(12 * n), pa = take<double>(n);
        std::vector<double> out(12 * n);
        for (int64_t i = 0; i < n; ++i) {
            double c[4][3], F[3];
            for (int q = 0; q < 4; ++q)
                for (int k = 0; k < 3; ++k) c[q][k] = x[12 * i + 3 * q + k];
            for (int a = 0; a < 4; ++a) {
                hk::loads_face_corner(c, a, pa[i], F);
                for (int k = 0; k < 3; ++k) out[12 * i + 3 * a + k] = F[k];
            }
        }
        put(fo, out);
    } else if (mode == "amp") {  // rows, nq; t[rows]; v[rows]; ct[nq] -> value[nq]
        const std::vector<int64_t> h = take<int64_t>(2);
        const std::vector<double> t = take<double>(h[0]), v = take<double>(h[0]), ct = take<double>(h[1]);
        std::vector<double> out(h[1]);
        for (int64_t i = 0; i < h[1]; ++i) out[i] = hk::loads_amp((int)h[0], t.data(), v.data(), ct[i]);
        put(fo, out);
    } else if (mode == "nodes") {  // the face table -> 24 columns
        std::vector<int32_t> out;
        for (int f = 0; f < 6; ++f)
            for (int a = 0; a < 4; ++a) out.push_back(hk::loads_code_node(hk::loads_face_code(f), a));
        put(fo, out);
    } else if (mode == "plan") {
        const std::vector<int64_t> h = take<int64_t>(7);  // nN nE n_amp n_cload n_grav n_press rows
        const std::vector<int32_t> conn = take<int32_t>(8 * h[1]);
        const std::vector<int32_t> amp_n = take<int32_t>(h[2]);
        const std::vector<int64_t> amp_off = take<int64_t>(h[2]);
        const std::vector<double> amp_t = take<double>(h[6]), amp_v = take<double>(h[6]);
        const std::vector<int64_t> cdof = take<int64_t>(h[3]);
        const std::vector<double> cval = take<double>(h[3]);
        const std::vector<int32_t> camp = take<int32_t>(h[3]);
        const std::vector<double> gacc = take<double>(3 * h[4]);
        const std::vector<int32_t> gamp = take<int32_t>(h[4]);
        const std::vector<int64_t> pel = take<int64_t>(h[5]);
        const std::vector<int32_t> pface = take<int32_t>(h[5]);
        const std::vector<double> pval = take<double>(h[5]);
        const std::vector<int32_t> pamp = take<int32_t>(h[5]);
        hakai_loads_t L;
        L.n_amp = (int32_t)h[2]; L.amp_n = amp_n.data(); L.amp_off = amp_off.data();
        L.amp_time = amp_t.data(); L.amp_value = amp_v.data();
        L.n_cload = h[3]; L.cload_dof = cdof.data(); L.cload_value = cval.data(); L.cload_amp = camp.data();
        L.n_grav = (int32_t)h[4]; L.grav_accel = gacc.data(); L.grav_amp = gamp.data();
        L.n_press = h[5]; L.press_elem = pel.data(); L.press_face = pface.data(); L.press_value = pval.data();
        L.press_amp = pamp.data();
        hk::LoadsPlan P;
        std::string err;
        const int rc = hk::loads_plan(L, h[0], h[1], conn.data(), P, err);
        put(fo, std::vector<int32_t>{rc});
        put(fo, P.cl_ptr); put(fo, P.cl_comp); put(fo, P.cl_amp); put(fo, P.cl_val);
        put(fo, P.pr_ptr); put(fo, P.pr_ent); put(fo, P.pr_elem); put(fo, P.pr_code);
        put(fo, P.amp_off); put(fo, P.amp_t);
    } else {
        return 2;
    }
    std::fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("loads")
    c, exe = d / "loads_check.cpp", d / "loads_check"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", CSRC, "-o", str(exe), str(c), os.path.join(CSRC, "hakai_loads_plan.cpp")],
                   check=True)
    n = [0]

    def run(mode, *arrays):
        n[0] += 1
        fi, fo = d / f"in{n[0]}.bin", d / f"out{n[0]}.bin"
        fi.write_bytes(b"".join(np.ascontiguousarray(a).tobytes() for a in arrays))
        subprocess.run([str(exe), mode, str(fi), str(fo)], check=True)   # a sanitizer report fails the run
        return fo.read_bytes()
    return run


def unpack(raw, dtypes):
    out, at = [], 0
    for dt in dtypes:
        n = int(np.frombuffer(raw, np.int64, 1, at)[0])
        at += 8
        out.append(np.frombuffer(raw, dt, n, at).copy())
        at += n * np.dtype(dt).itemsize
    assert at == len(raw)
    return out


def header_faces(prog, x, pa):
    x, pa = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(pa, np.float64)
    raw = prog("face", np.array([len(pa)], np.int64), x, pa)
    return unpack(raw, [np.float64])[0].reshape(len(pa), 4, 3)


def warped_faces(n, seed):
    """Unit-ish quads in a random plane position, every corner perturbed out of plane and in it."""
    rng = np.random.default_rng(seed)
    base = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)
    x = base[None] * rng.uniform(0.2, 3.0, size=(n, 1, 3)) + rng.normal(0, 0.15, size=(n, 4, 3))
    x += rng.uniform(-50, 50, size=(n, 1, 3))
    return x, rng.normal(0, 100.0, size=n)


# ---- header == NumPy, bit for bit ------------------------------------------------------------------

def test_face_table(prog):
    got = unpack(prog("nodes"), [np.int32])[0].reshape(6, 4)
    assert np.array_equal(got, np.array(R.FACE_NODES))


def test_faces_bitwise(prog):
    x, pa = warped_faces(1000, 3)
    x[0, 1] = x[0, 0]                       # an edge collapsed
    x[1, :] = x[1, 0]                       # the whole face collapsed: zero area
    pa[2], pa[3] = 0.0, -0.0
    x[4] = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64)   # flat: -0.0 components
    got = header_faces(prog, x, pa)
    ref = np.array([R.face_corners(xi, p) for xi, p in zip(x, pa)])
    assert bitwise_equal(got, ref)
    assert np.all(got[1] == 0.0) and np.all(got[2] == 0.0) and np.all(got[3] == 0.0)


TABLES = {"two_point": ([0.0, 1e-5], [0.0, 1.0]),
          "multi_point": ([0.0, 1e-6, 3e-6, 1e-5], [0.0, 1.0, 0.25, 2.0]),
          "stepped": ([0.0, 2e-6, 2e-6, 1e-5], [0.0, 0.0, 1.0, 1.0]),
          "non_monotonic": ([0.0, 4e-6, 2e-6, 1e-5], [1.0, -1.0, 3.0, 0.5]),
          "late_start": ([2e-6, 4e-6, 8e-6], [0.5, 1.5, -0.5])}


@pytest.mark.parametrize("name", sorted(TABLES))
def test_amplitude_bitwise(prog, name):
    t, v = (np.array(a, np.float64) for a in TABLES[name])
    ct = np.concatenate([t, np.nextafter(t, -1), np.nextafter(t, 1), [-1e-6, 0.5e-6, 2.5e-6, 5e-6, 2e-5, 1.0]])
    raw = prog("amp", np.array([len(t), len(ct)], np.int64), t, v, ct)
    got = unpack(raw, [np.float64])[0]
    ref = np.array([R.amp_value(t, v, c) for c in ct])
    assert bitwise_equal(got, ref)
    import nodal_ref                                        # the rule of the *Boundary amplitudes
    assert bitwise_equal(ref, np.array([nodal_ref.amplitude(t, v, c) for c in ct]))
    assert R.amp_value(t, v, t[0]) == v[0]
    if name == "late_start":                                # before the table: the first segment extrapolated
        assert R.amp_value(t, v, 0.0) == 0.5 + (1.5 - 0.5) * (0.0 - 2e-6) / (4e-6 - 2e-6)


# ---- NumPy against exact rationals ------------------------------------------------------------------

def test_faces_against_rationals():
    x, pa = warped_faces(300, 7)
    worst = Fraction(0)
    for xi, p in zip(x, pa):
        got, ex, bound = R.face_corners(xi, p), R.face_exact(xi, p), R.face_bound(xi, p)
        for a in range(4):
            for c in range(3):
                err = abs(Fraction(float(got[a, c])) - ex[a][c])
                assert err <= bound, (float(err), float(bound))
                worst = max(worst, err / bound)
        # the four corners carry p times the area vector, 4 g1 x g2 = 1/2 (x2 - x0) x (x3 - x1)
        X = [[Fraction(float(v)) for v in row] for row in xi]
        d1 = [X[2][c] - X[0][c] for c in range(3)]
        d2 = [X[3][c] - X[1][c] for c in range(3)]
        area = [(d1[1] * d2[2] - d1[2] * d2[1]) / 2, (d1[2] * d2[0] - d1[0] * d2[2]) / 2,
                (d1[0] * d2[1] - d1[1] * d2[0]) / 2]
        for c in range(3):
            assert sum(ex[a][c] for a in range(4)) == Fraction(float(p)) * area[c]
    print(f"face forces: worst error {float(worst):.3f} of the bound")


# ---- known answers -----------------------------------------------------------------------------------

CUBE = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]], np.float64)
N_OUT = np.array([[0, 0, -1], [0, 0, 1], [0, -1, 0], [1, 0, 0], [0, 1, 0], [-1, 0, 0]], np.float64)


@pytest.mark.parametrize("scale,shift", [(1.0, 0.0), (0.5, 3.0), (4.0, -16.0)])
def test_unit_cube_faces_exact(prog, scale, shift):
    """Dyadic coordinates: every operation is exact, so face k gives exactly -p A n_out / 4 per corner.
    This is the geometric definition that decides the face table."""
    X = CUBE * scale + shift
    p, A = 3.0, scale * scale
    for k in range(6):
        x = X[list(R.FACE_NODES[k])]
        assert np.all(np.abs(x @ N_OUT[k] - (x @ N_OUT[k])[0]) == 0.0), "the four nodes lie on the face"
        F = R.face_corners(x, p)
        want = np.tile(-p * A * N_OUT[k] / 4.0, (4, 1))
        assert np.array_equal(F, want), (k, F)
        assert np.array_equal(header_faces(prog, x[None], [p])[0], want)


def test_parallelogram_h_terms_vanish():
    x0, a, b = np.array([1.0, 2.0, -0.5]), np.array([2.0, 0.5, 0.25]), np.array([-0.5, 1.5, 1.0])
    x = np.array([x0, x0 + a, x0 + a + b, x0 + b])
    F = R.face_corners(x, 2.0)
    want = 2.0 * np.cross(a, b) / 4.0      # dyadic: exact
    assert np.array_equal(F, np.tile(want, (4, 1)))


def exterior_faces(m):
    seen = {}
    for e in range(m.nElement):
        for k in range(6):
            key = tuple(sorted(m.elementmat[e][list(R.FACE_NODES[k])]))
            seen.setdefault(key, []).append((e + 1, k + 1))
    return [v[0] for v in seen.values() if len(v) == 1]


def test_closed_surface_balances_exactly():
    m = mesh.bar_model(2, 2, 2, mesh.steel_elastic(), 0.0, perturb=0.08, seed=9, n_steps=10)
    faces = exterior_faces(m)
    assert len(faces) == 24
    tot = [Fraction(0)] * 3
    for e, k in faces:
        x = m.coordmat[m.elementmat[e - 1][list(R.FACE_NODES[k - 1])] - 1]
        ex = R.face_exact(x, 7.25)
        for a in range(4):
            for c in range(3):
                tot[c] += ex[a][c]
    assert tot == [0, 0, 0]


# ---- the planner ----------------------------------------------------------------------------------------

def plan_case():
    m = mesh.bar_model(2, 3, 2, mesh.steel_elastic(), 0.0, perturb=0.03, seed=4, n_steps=10)
    rng = np.random.default_rng(12)
    ext = exterior_faces(m)
    pe = [e for e, _ in ext] + [1, 1, 5, 5, 12]          # exterior, then interior ones and a face twice
    pf = [k for _, k in ext] + [2, 2, 4, 6, 1]
    n_cl = 40
    ld = Loads(amps=[TABLES["two_point"], TABLES["multi_point"]],
               cload_dof=rng.integers(1, 3 * m.nNode + 1, n_cl), cload_value=rng.normal(0, 1, n_cl),
               cload_amp=rng.integers(-1, 2, n_cl), grav_accel=[[0, 0, -9.81e3], [1.0, 0, 0]], grav_amp=[-1, 1],
               press_elem=pe, press_face=pf, press_value=rng.normal(0, 5, len(pe)),
               press_amp=rng.integers(-1, 2, len(pe)))
    ld.cload_dof[:3] = 7                                    # several entries on one dof
    return m, ld


def run_plan(prog, m, ld, nN=None, nE=None):
    s, keep = ld.c()
    amp_n = np.array([len(t) for t, _ in ld.amps], np.int32)
    amp_off = np.concatenate([[0], np.cumsum(amp_n)[:-1]]).astype(np.int64) if len(amp_n) else np.zeros(0, np.int64)
    at = np.concatenate([t for t, _ in ld.amps] + [np.zeros(0)])
    av = np.concatenate([v for _, v in ld.amps] + [np.zeros(0)])
    head = np.array([m.nNode if nN is None else nN, m.nElement if nE is None else nE, len(ld.amps),
                     len(ld.cload_dof), len(ld.grav_accel), len(ld.press_elem), len(at)], np.int64)
    raw = prog("plan", head, (m.elementmat - 1).astype(np.int32), amp_n, amp_off, at, av, ld.cload_dof,
               ld.cload_value, ld.cload_amp, ld.grav_accel, ld.grav_amp, ld.press_elem, ld.press_face,
               ld.press_value, ld.press_amp)
    i32 = np.int32
    return unpack(raw, [i32, i32, i32, i32, np.float64, i32, i32, i32, i32, i32, np.float64])


def test_planner_lists_bitwise(prog):
    m, ld = plan_case()
    rc, cl_ptr, cl_comp, cl_amp, cl_val, pr_ptr, pr_ent, pr_elem, pr_code, amp_off, amp_t = run_plan(prog, m, ld)
    assert rc[0] == 0
    ref = R.plan(m, ld)
    for got, want in zip((cl_ptr, cl_comp, cl_amp, cl_val, pr_ptr, pr_ent), ref):
        assert bitwise_equal(got, np.ascontiguousarray(want, got.dtype))
    assert np.array_equal(pr_elem, ld.press_elem - 1)
    assert np.array_equal(amp_off, [0, 2]) and len(amp_t) == 6
    for k, face in enumerate(ld.press_face):
        assert [(pr_code[k] >> (3 * a)) & 7 for a in range(4)] == list(R.FACE_NODES[face - 1])
    counts = np.diff(pr_ptr)
    assert {2, 3, 4, 5, 6} <= set(counts)                           # lists of every length up to 6
    for n in range(m.nNode):                                        # ascending entry order per node
        assert np.all(np.diff(pr_ent[pr_ptr[n]:pr_ptr[n + 1]]) > 0)


def test_planner_empty_kinds(prog):
    m, _ = plan_case()
    out = run_plan(prog, m, Loads(grav_accel=[[0, 0, -1.0]]))
    assert out[0][0] == 0 and all(len(a) == 0 for a in out[1:9])


BAD = {"dof_zero": dict(cload_dof=[0], cload_value=[1.0]),
       "dof_past_end": dict(cload_dof=[3 * 36 + 1], cload_value=[1.0]),
       "cload_nan": dict(cload_dof=[1], cload_value=[np.nan]),
       "cload_amp": dict(cload_dof=[1], cload_value=[1.0], cload_amp=[2]),
       "cload_amp_low": dict(cload_dof=[1], cload_value=[1.0], cload_amp=[-2]),
       "grav_inf": dict(grav_accel=[[0, np.inf, 0]]),
       "grav_amp": dict(grav_accel=[[0, 1.0, 0]], grav_amp=[5]),
       "elem_zero": dict(press_elem=[0], press_face=[1], press_value=[1.0]),
       "elem_past_end": dict(press_elem=[13], press_face=[1], press_value=[1.0]),
       "face_zero": dict(press_elem=[1], press_face=[0], press_value=[1.0]),
       "face_seven": dict(press_elem=[1], press_face=[7], press_value=[1.0]),
       "press_inf": dict(press_elem=[1], press_face=[1], press_value=[-np.inf]),
       "press_amp": dict(press_elem=[1], press_face=[1], press_value=[1.0], press_amp=[2]),
       "one_row_table": dict(amps=[([0.0], [1.0])], grav_accel=[[0, 0, 1.0]]),
       "table_nan": dict(amps=[([0.0, np.nan], [1.0, 1.0])], grav_accel=[[0, 0, 1.0]])}


@pytest.mark.parametrize("name", sorted(BAD))
def test_planner_refusals(prog, name):
    m, _ = plan_case()
    assert m.nNode == 36 and m.nElement == 12
    kw = dict(amps=[TABLES["two_point"], TABLES["multi_point"]])
    kw.update(BAD[name])
    assert run_plan(prog, m, Loads(**kw))[0][0] == -1
