"""Rigid walls (hakai_set_walls) on the CPU.

  * The arithmetic under test is the kernel's own: this file compiles
    hakai-fem_amd/csrc/hakai_walls_node.hpp (the header hakai_loads.hip includes) and the host planner
    hakai_walls_plan.cpp into a small stand-alone program (its own main, built with
    -fsanitize=address,undefined and no contraction) and holds both against walls_ref BIT FOR BIT: the
    normalisation, the frame, the gap and the node force on random and special inputs, the planner's
    normals, table and masks, and each of the planner's refusals.
  * walls_ref itself is held against 60-digit decimal arithmetic within the bounds its docstring
    derives from the operation count.
  * Known answers with dyadic inputs, exact or within counted roundings."""
import os
import subprocess

import numpy as np
import pytest

import walls_ref as R
from hakai import mesh
from hakai.model import Walls
from util import bitwise_equal
from walls_cases import TABLES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
CXXFLAGS = ["-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined"]
U = 2.0 ** -53

# The harness only moves bytes: it calls the header's and the planner's functions.
SRC = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "hakai_walls_node.hpp"
#include "hakai_walls_plan.hpp"

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
    if (mode == "norm") {  // n; normal[n][3] -> n[n][3], len[n]
        const int64_t n = take<int64_t>(1)[0];
        const std::vector<double> a = take<double>(3 * n);
        std::vector<double> out(3 * n), len(n);
        for (int64_t i = 0; i < n; ++i) {
            double x[3] = {a[3 * i], a[3 * i + 1], a[3 * i + 2]}, y[3];
            len[i] = hk::walls_normalise(x, y);
            for (int c = 0; c < 3; ++c) out[3 * i + c] = y[c];
        }
        put(fo, out);
        put(fo, len);
    } else if (mode == "frame") {  // n; origin[n][3]; motion[n][3]; s0[n]; sm[n]; dt[n] -> o[n][3], vw[n][3]
        const int64_t n = take<int64_t>(1)[0];
        const std::vector<double> og = take<double>(3 * n), mo = take<double>(3 * n), s0 = take<double>(n),
                                  sm = take<double>(n), dt = take<double>(n);
        std::vector<double> o(3 * n), vw(3 * n);
        for (int64_t i = 0; i < n; ++i) {
            double a[3], b[3];
            hk::walls_frame(&og[3 * i], &mo[3 * i], s0[i], sm[i], dt[i], a, b);
            for (int c = 0; c < 3; ++c) o[3 * i + c] = a[c], vw[3 * i + c] = b[c];
        }
        put(fo, o);
        put(fo, vw);
    } else if (mode == "force") {
        // n; coord[n][3]; u[n][3]; um[n][3]; m[n]; dt[n]; o[n][3]; vw[n][3]; nrm[n][3]; par[n][4]
        //   -> g[n], F[n][3] (zeros where d = -g is not > 0)
        const int64_t n = take<int64_t>(1)[0];
        const std::vector<double> co = take<double>(3 * n), u = take<double>(3 * n), um = take<double>(3 * n),
                                  m = take<double>(n), dt = take<double>(n), o = take<double>(3 * n),
                                  vw = take<double>(3 * n), nr = take<double>(3 * n), par = take<double>(4 * n);
        std::vector<double> g(n), F(3 * n, 0.0);
        for (int64_t i = 0; i < n; ++i) {
            double c3[3], u3[3], m3[3], o3[3], v3[3], f3[3];
            for (int c = 0; c < 3; ++c)
                c3[c] = co[3 * i + c], u3[c] = u[3 * i + c], m3[c] = um[3 * i + c], o3[c] = o[3 * i + c], v3[c] = vw[3 * i + c];
            g[i] = hk::walls_gap(c3, u3, o3, &nr[3 * i]);
            const double d = -g[i];
            if (d > 0.0) {
                hk::walls_force(d, u3, m3, m[i], dt[i], v3, &nr[3 * i], par[4 * i], par[4 * i + 1], par[4 * i + 2],
                                par[4 * i + 3], f3);
                for (int c = 0; c < 3; ++c) F[3 * i + c] = f3[c];
            }
        }
        put(fo, g);
        put(fo, F);
    } else if (mode == "plan") {
        const std::vector<int64_t> h = take<int64_t>(5);  // nN n_amp rows n_wall n_nodes
        const std::vector<int32_t> amp_n = take<int32_t>(h[1]);
        const std::vector<int64_t> amp_off = take<int64_t>(h[1]);
        const std::vector<double> amp_t = take<double>(h[2]), amp_v = take<double>(h[2]);
        const size_t nw = h[3] < 0 ? 0 : (size_t)h[3];
        const std::vector<double> og = take<double>(3 * nw), nr = take<double>(3 * nw), mo = take<double>(3 * nw);
        const std::vector<int32_t> amp = take<int32_t>(nw);
        const std::vector<double> st = take<double>(nw), sc = take<double>(nw), da = take<double>(nw), fr = take<double>(nw);
        const std::vector<int64_t> off = take<int64_t>(nw + 1), nodes = take<int64_t>(h[4]);
        hakai_walls_t W;
        W.n_amp = (int32_t)h[1]; W.amp_n = amp_n.data(); W.amp_off = amp_off.data();
        W.amp_time = amp_t.data(); W.amp_value = amp_v.data();
        W.n_wall = (int32_t)h[3]; W.origin = og.data(); W.normal = nr.data(); W.motion = mo.data(); W.amp = amp.data();
        W.stiffness = st.data(); W.scale = sc.data(); W.damping = da.data(); W.friction = fr.data();
        W.node_off = off.data(); W.nodes = nodes.data();
        hk::WallsPlan P;
        std::string err;
        const int rc = hk::walls_plan(W, h[0], P, err);
        put(fo, std::vector<int32_t>{rc, P.n_wall});
        put(fo, P.tab); put(fo, P.amp); put(fo, P.mask); put(fo, P.amp_off); put(fo, P.amp_t);
    } else {
        return 2;
    }
    std::fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("walls")
    c, exe = d / "walls_check.cpp", d / "walls_check"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", CSRC, "-o", str(exe), str(c), os.path.join(CSRC, "hakai_walls_plan.cpp")],
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


F64 = np.float64


def header_force(prog, coord, u, um, m, dt, o, vw, n, par):
    """(g, F) of the header for one (node, wall) pair per row."""
    k = len(m)
    arrs = [np.ascontiguousarray(a, F64) for a in (coord, u, um, m, dt, o, vw, n, par)]
    g, F = unpack(prog("force", np.array([k], np.int64), *arrs), [F64, F64])
    return g, F.reshape(k, 3)


def ref_force(coord, u, um, m, dt, o, vw, n, par):
    """The same rows through walls_ref, one row at a time (each row has its own wall)."""
    k = len(m)
    g, F = np.zeros(k), np.zeros((k, 3))
    for i in range(k):
        c, a, b = (np.asarray(x, F64)[i:i + 1] for x in (coord, u, um))
        g[i] = R.gap(c, a, np.asarray(o, F64)[i], np.asarray(n, F64)[i])[0]
        d = -g[i]
        if d > 0.0:
            F[i] = R.node_force(np.array([d]), a, b, np.asarray(m, F64)[i:i + 1], dt[i], np.asarray(vw, F64)[i],
                                np.asarray(n, F64)[i], *np.asarray(par, F64)[i])[0]
    return g, F


def random_rows(k, seed):
    """Nodes near a randomly oriented moving plane, about half of them through it."""
    rng = np.random.default_rng(seed)
    nrm = np.array([R.normalise(v)[0] for v in rng.normal(0, 1, (k, 3))])
    o = rng.uniform(-5, 5, (k, 3))
    depth = rng.normal(0, 1e-3, k)
    tang = rng.normal(0, 1, (k, 3))
    coord = o + tang - np.sum(tang * nrm, axis=1)[:, None] * nrm + depth[:, None] * nrm
    u = rng.normal(0, 1e-4, (k, 3))
    dt = np.full(k, 1e-7) * rng.uniform(0.5, 2.0, k)
    um = u - rng.normal(0, 5.0, (k, 3)) * dt[:, None]
    m = rng.uniform(1e-9, 1e-6, k)
    vw = rng.normal(0, 2.0, (k, 3))
    par = np.stack([rng.uniform(0, 1e6, k), rng.uniform(0, 1.0, k), rng.uniform(0, 0.5, k), rng.uniform(0, 0.6, k)],
                   axis=1)
    return coord, u, um, m, dt, o, vw, nrm, par


# ---- header == NumPy, bit for bit --------------------------------------------------------------------

def test_normalise_bitwise(prog):
    rng = np.random.default_rng(1)
    a = rng.normal(0, 1, (500, 3)) * 10.0 ** rng.uniform(-8, 8, (500, 1))
    a[0], a[1], a[2], a[3] = (0, 0, 1), (0, -2, 0), (1, 2, 2), (-0.0, 0.0, 5e-324)
    n, ln = unpack(prog("norm", np.array([len(a)], np.int64), a), [F64, F64])
    ref = [R.normalise(v) for v in a]
    assert bitwise_equal(n.reshape(-1, 3), np.array([r[0] for r in ref]))
    assert bitwise_equal(ln, np.array([r[1] for r in ref]))


def test_frame_bitwise(prog):
    rng = np.random.default_rng(2)
    k = 400
    og, mo = rng.normal(0, 3, (k, 3)), rng.normal(0, 1, (k, 3))
    s0, sm, dt = rng.normal(0, 1, k), rng.normal(0, 1, k), rng.uniform(1e-8, 1e-6, k)
    mo[0] = 0.0
    sm[1] = s0[1]                                      # a wall at rest: vw = +-0.0
    mo[2] = (-0.0, 0.0, -1.0)
    o, vw = unpack(prog("frame", np.array([k], np.int64), og, mo, s0, sm, dt), [F64, F64])
    ref = [R.frame(og[i], mo[i], s0[i], sm[i], dt[i]) for i in range(k)]
    assert bitwise_equal(o.reshape(k, 3), np.array([r[0] for r in ref]))
    assert bitwise_equal(vw.reshape(k, 3), np.array([r[1] for r in ref]))


def test_force_bitwise_random_and_special(prog):
    rows = [np.array(a) for a in random_rows(3000, 5)]
    coord, u, um, m, dt, o, vw, nrm, par = rows
    um[0] = u[0]; vw[0] = 0.0                           # no slip at all: s == 0, no NaN
    m[1] = 0.0; par[1, 0] = 0.0                          # zero mass and zero stiffness
    par[2, 2:] = 0.0                                    # no damping, no friction
    u[3] = -0.0; um[3] = -0.0
    par[4, 3] = 1e9                                     # stick for certain
    par[5, 3] = 1e-12                                   # slip for certain
    um[6] = u[6] - np.array([1e6, 1e6, 1e6]) * nrm[6] * dt[6]   # separating fast: non-adhesive
    par[6, 2] = 0.5
    g, F = header_force(prog, *rows)
    rg, rF = ref_force(*rows)
    assert bitwise_equal(g, rg) and bitwise_equal(F, rF)
    assert 0.3 < np.mean(g < 0) < 0.7 and not np.any(np.isnan(F))
    assert np.any(F[g < 0] != 0.0) and np.all(F[g >= 0] == 0.0)


# ---- NumPy against 60-digit arithmetic -----------------------------------------------------------------

def test_restatement_against_high_precision():
    coord, u, um, m, dt, o, vw, nrm, par = random_rows(400, 11)
    worst = {"gap": 0.0, "force": 0.0, "frame": 0.0}
    n_force = 0
    for i in range(len(m)):
        g = R.gap(coord[i:i + 1], u[i:i + 1], o[i], nrm[i])[0]
        X = max(abs(coord[i, c]) + abs(u[i, c]) + abs(o[i, c]) for c in range(3))
        err = abs(float(R.gap_hp(coord[i], u[i], o[i], nrm[i]) - R._D(g)))
        assert err <= R.GAP_COUNT * U * X
        worst["gap"] = max(worst["gap"], err / (R.GAP_COUNT * U * X))
        d = -g
        if d > 0.0:
            n_force += 1
            F = R.node_force(np.array([d]), u[i:i + 1], um[i:i + 1], m[i:i + 1], dt[i], vw[i], nrm[i], *par[i])[0]
            hp = R.node_force_hp(d, u[i], um[i], m[i], dt[i], vw[i], nrm[i], *par[i])
            bound = R.node_force_bound(d, u[i], um[i], m[i], dt[i], vw[i], *par[i])
            for c in range(3):
                err = abs(float(hp[c] - R._D(F[c])))
                assert err <= bound, (i, c, err, bound)
                worst["force"] = max(worst["force"], err / bound)
        s0, sm = par[i, 1], par[i, 2]
        fo, fv = R.frame(o[i], vw[i], s0, sm, dt[i])
        ho, hv = R.frame_hp(o[i], vw[i], s0, sm, dt[i])
        for c in range(3):
            bo = 2 * U * (abs(o[i, c]) + abs(vw[i, c] * s0)) * (1 + 1e-9)
            assert abs(float(ho[c] - R._D(fo[c]))) <= bo
            assert abs(float(hv[c] - R._D(fv[c]))) <= 3 * U * abs(float(hv[c])) * (1 + 1e-9)
    assert n_force > 100
    print("worst error as a fraction of the bound:", worst)


# ---- known answers ---------------------------------------------------------------------------------------

def one(coord, u, um, m, dt, o, vw, n, par):
    g, F = ref_force(*[np.array([a], F64) for a in (coord, u, um)], np.array([m]), np.array([dt]),
                     *[np.array([a], F64) for a in (o, vw, n, par)])
    return g[0], F[0]


Z = (0.0, 0.0, 0.0)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("a,b", [(10, -7), (0, -20), (25, -3)])
def test_axis_wall_penalty_exact(prog, axis, a, b):
    """stiffness 2^a, penetration 2^b, no damping, no friction, node at rest: exactly 2^(a+b) n."""
    n = np.eye(3)[axis]
    coord = (1.0, 2.0, 3.0) - 2.0 ** b * n
    args = (coord, Z, Z, 0.5, 2.0 ** -23, (1.0, 2.0, 3.0), Z, n, (2.0 ** a, 0.0, 0.0, 0.0))
    g, F = one(*args)
    assert g == -2.0 ** b and np.array_equal(F, 2.0 ** (a + b) * n)
    hg, hF = header_force(prog, *[[x] for x in args])
    assert hg[0] == g and np.array_equal(hF[0], F)


def test_on_and_above_the_plane_give_nothing():
    par = (1024.0, 0.5, 0.25, 0.5)
    for z in (0.0, -0.0, 2.0 ** -30, 1.0):
        g, F = one((0.5, 0.5, z), Z, (0.0, 0.0, 1e-3), 1.0, 2.0 ** -20, Z, Z, (0.0, 0.0, 1.0), par)
        assert g >= 0.0 and np.all(F == 0.0)
    g, F = one((0.5, 0.5, -(2.0 ** -30)), Z, Z, 1.0, 2.0 ** -20, Z, Z, (0.0, 0.0, 1.0), par)
    assert g < 0.0 and F[2] > 0.0


def test_non_adhesive():
    """A node leaving fast enough that k d - c vn < 0 gets exactly 0, not a pull."""
    dt, m, k, d = 2.0 ** -10, 4.0, 1024.0, 2.0 ** -8
    c = 2 * 0.5 * np.sqrt(m * k)                       # 64
    vn = 1.0                                            # k d = 4 < c vn = 64
    g, F = one((0.0, 0.0, -d), Z, (0.0, 0.0, -vn * dt), m, dt, Z, Z, (0.0, 0.0, 1.0), (k, 0.0, 0.5, 0.5))
    assert g == -d and c == 64.0 and np.all(F == 0.0)
    g, F = one((0.0, 0.0, -d), Z, (0.0, 0.0, vn * dt), m, dt, Z, Z, (0.0, 0.0, 1.0), (k, 0.0, 0.5, 0.0))
    assert np.array_equal(F, (0.0, 0.0, k * d + c * vn))    # approaching: the damper adds


def test_stick_stops_the_slip_in_one_step():
    dt, m, k, d = 2.0 ** -10, 3.0, 2.0 ** 20, 2.0 ** -6
    vt = np.array([0.3, -0.7, 0.0])
    g, F = one((0.0, 0.0, -d), Z, -vt * dt, m, dt, Z, Z, (0.0, 0.0, 1.0), (k, 0.0, 0.0, 0.9))
    v = (np.zeros(3) - (-vt * dt)) / dt                 # what the definition forms
    assert 0.9 * k * d > m * np.linalg.norm(v) / dt
    want = -(m / dt) * v
    assert np.all(np.abs(F[:2] - want[:2]) <= 2 * 2.0 ** -52 * np.abs(want[:2]) + 0.0)   # T / s and * vt round
    assert F[2] == k * d


def test_slip_direction_three_four_five():
    dt, m, k, d, mu, vv = 2.0 ** -10, 2.0 ** 10, 2.0 ** 10, 2.0 ** -6, 0.25, 2.0
    um = -np.array([3.0, 4.0, 0.0]) * vv * dt          # v = (6, 8, 0) exactly, s = 10
    g, F = one((0.0, 0.0, -d), Z, um, m, dt, Z, Z, (0.0, 0.0, 1.0), (k, 0.0, 0.0, mu))
    N = k * d
    assert mu * N < m * 10.0 / dt and F[2] == N
    want = -mu * N * np.array([0.6, 0.8])
    # T / s is exact here (4 / 10 rounds once), times vt rounds once: two roundings
    assert np.all(np.abs(F[:2] - want) <= 2 * 2.0 ** -52 * np.abs(want))


def test_zero_slip_and_zero_mass():
    g, F = one((0.0, 0.0, -0.25), Z, Z, 2.0, 0.5, Z, Z, (0.0, 0.0, 1.0), (8.0, 0.0, 0.5, 0.5))
    assert np.array_equal(F, (0.0, 0.0, 2.0)) and not np.any(np.isnan(F))
    g, F = one((0.0, 0.0, -0.25), Z, (1e-3, 0.0, 0.0), 0.0, 0.5, Z, Z, (0.0, 0.0, 1.0), (0.0, 0.5, 0.5, 0.5))
    assert g < 0 and np.all(F == 0.0)                   # k = 0 and m = 0: nothing to push with


def test_oblique_normal_in_thirds(prog):
    n, ln = R.normalise((1.0, 2.0, 2.0))
    assert ln == 3.0
    for got, want in zip(n, (1 / 3, 2 / 3, 2 / 3)):
        assert abs(got - want) <= 2.0 ** -53 * want * 2   # one rounding (of the quotient)
    hn, hl = unpack(prog("norm", np.array([1], np.int64), np.array([1.0, 2.0, 2.0])), [F64, F64])
    assert bitwise_equal(hn, n) and hl[0] == 3.0


def test_moving_wall_velocity_of_a_ramp():
    """A ramp table s(tau) = slope * tau: vw = motion * slope to the counted roundings (two amplitude
    values with four roundings each on top of tau's one, a difference, a quotient, a product)."""
    w = Walls(origin=[[0, 0, 0]], normal=[[0, 0, 1]], motion=[[0.5, -2.0, 3.0]], amp=[0],
              amps=[([0.0, 1e-3], [0.0, 2.0])])
    slope, dt = 2.0 / 1e-3, 1e-7
    for t in (1, 2, 3, 50, 1000):
        o, vw = R.wall_frame(w, 0, t, dt)
        s0 = slope * (t - 1) * dt
        # each amplitude value errs by <= 5 u s0; their difference is s0 - sm = slope dt, so the
        # quotient errs relatively by <= 10 u s0 / (slope dt) + 2 u = (10 (t - 1) + 2) u, +1 u for the product
        rel = (10 * max(t - 1, 1) + 3) * U
        assert np.all(np.abs(vw - w.motion[0] * slope) <= rel * np.abs(w.motion[0] * slope))
        assert np.all(np.abs(o - w.motion[0] * s0) <= 7 * U * np.abs(w.motion[0] * s0))
    o, vw = R.wall_frame(w, 0, 1, dt)                   # t = 1: taum < 0, the first segment extrapolated
    assert np.all(o == 0.0) and np.all(vw != 0.0)


# ---- the planner -------------------------------------------------------------------------------------------

def plan_walls(n_node, seed=3):
    rng = np.random.default_rng(seed)
    nodes = [np.zeros(0, np.int64), rng.choice(n_node, 9, replace=False) + 1, np.array([5, 5, 7, 5, n_node, 1]),
             np.zeros(0, np.int64)]
    return Walls(origin=rng.normal(0, 1, (4, 3)), normal=[[0, 0, 1], [1, 2, 2], [-3, 0.5, 1e-3], [0, -1e-100, 0]],
                 motion=rng.normal(0, 1, (4, 3)), amp=[-1, 1, 0, -1], stiffness=[0, 1e3, 5.0, 0],
                 scale=[0.5, 0, 0.25, 1.0], damping=[0, 0.1, 0, 0.5], friction=[0, 0.3, 0.0, 1.5], nodes=nodes,
                 amps=[TABLES["two_point"], TABLES["multi_point"]])


def run_plan(prog, n_node, w, n_wall=None):
    amp_n = np.array([len(t) for t, _ in w.amps], np.int32)
    amp_off = np.concatenate([[0], np.cumsum(amp_n)[:-1]]).astype(np.int64) if len(amp_n) else np.zeros(0, np.int64)
    at = np.concatenate([t for t, _ in w.amps] + [np.zeros(0)])
    av = np.concatenate([v for _, v in w.amps] + [np.zeros(0)])
    off = np.concatenate([[0], np.cumsum([len(x) for x in w.nodes])]).astype(np.int64)
    nodes = np.concatenate(list(w.nodes) + [np.zeros(0, np.int64)]).astype(np.int64)
    nw = w.n_wall if n_wall is None else n_wall
    head = np.array([n_node, len(w.amps), len(at), nw, len(nodes)], np.int64)
    raw = prog("plan", head, amp_n, amp_off, at, av, w.origin, w.normal, w.motion, w.amp, w.stiffness, w.scale,
               w.damping, w.friction, off, nodes)
    return unpack(raw, [np.int32, F64, np.int32, np.uint32, np.int32, F64])


def test_planner_table_and_masks_bitwise(prog):
    w = plan_walls(40)
    rc, tab, amp, mask, amp_off, amp_t = run_plan(prog, 40, w)
    assert list(rc) == [0, 4]
    tab = tab.reshape(4, 13)
    assert bitwise_equal(tab[:, 0:3], np.array([R.normalise(v)[0] for v in w.normal]))
    assert bitwise_equal(tab[:, 3:6], w.origin) and bitwise_equal(tab[:, 6:9], w.motion)
    assert bitwise_equal(tab[:, 9:13], np.stack([w.stiffness, w.scale, w.damping, w.friction], axis=1))
    assert np.array_equal(amp, w.amp) and np.array_equal(amp_off, [0, 2]) and len(amp_t) == 6
    assert np.array_equal(mask, R.masks(40, w))
    assert mask[4] & 4 and bin(int(mask[4])).count("1") >= 3    # node 5: listed three times, one bit; plus the all-node walls
    assert np.all(mask & 1) and np.all(mask & 8) and np.sum((mask & 4) != 0) == 4


def test_planner_all_nodes_needs_no_mask(prog):
    w = Walls(origin=[[0, 0, 0], [1, 0, 0]], normal=[[0, 0, 1], [1, 0, 0]])
    rc, tab, amp, mask, _, _ = run_plan(prog, 40, w)
    assert list(rc) == [0, 2] and len(mask) == 0 and np.array_equal(amp, [-1, -1])
    assert np.array_equal(tab.reshape(2, 13)[:, 9:13], [[0, 0.5, 0, 0]] * 2)      # the defaults
    rc = run_plan(prog, 40, Walls())[0]
    assert list(rc) == [0, 0]


def test_planner_thirty_two_walls(prog):
    w = Walls(origin=np.zeros((32, 3)), normal=np.tile([0.0, 0, 1], (32, 1)), nodes=[[k + 1] for k in range(32)])
    rc, _, _, mask, _, _ = run_plan(prog, 40, w)
    assert list(rc) == [0, 32]
    assert np.array_equal(mask[:32], 1 << np.arange(32, dtype=np.uint64)) and np.all(mask[32:] == 0)


def bad_walls():
    base = dict(origin=[[0, 0, 0]], normal=[[0, 0, 1]])
    amps = [TABLES["two_point"]]
    B = {"node_zero": dict(base, nodes=[[0]]), "node_past_end": dict(base, nodes=[[41]]),
         "normal_zero": dict(base, normal=[[0, 0, 0]]), "normal_negative_zero": dict(base, normal=[[-0.0, 0.0, -0.0]]),
         "normal_nan": dict(base, normal=[[0, np.nan, 1]]), "normal_inf": dict(base, normal=[[np.inf, 0, 1]]),
         "origin_inf": dict(base, origin=[[0, np.inf, 0]]), "motion_nan": dict(base, motion=[[np.nan, 0, 0]]),
         "amp_high": dict(base, amp=[1], amps=amps), "amp_low": dict(base, amp=[-2], amps=amps),
         "amp_without_tables": dict(base, amp=[0]),
         "one_row_table": dict(base, amp=[0], amps=[([0.0], [1.0])]),
         "table_nan": dict(base, amp=[0], amps=[([0.0, np.nan], [1.0, 1.0])]),
         "thirty_three": dict(origin=np.zeros((33, 3)), normal=np.tile([0.0, 0, 1], (33, 1)))}
    for name in ("stiffness", "scale", "damping", "friction"):
        B[name + "_negative"] = dict(base, **{name: [-1e-300]})
        B[name + "_nan"] = dict(base, **{name: [np.nan]})
        B[name + "_inf"] = dict(base, **{name: [np.inf]})
    return B


BAD = bad_walls()


@pytest.mark.parametrize("name", sorted(BAD))
def test_planner_refusals(prog, name):
    w = Walls(**BAD[name])
    assert run_plan(prog, 40, w)[0][0] == -1 and not R.valid(40, w)


def test_planner_refuses_a_negative_count(prog):
    assert run_plan(prog, 40, Walls(), n_wall=-1)[0][0] == -1 and not R.valid(40, Walls(), n_wall=-1)


def test_planner_accepts_what_the_restatement_accepts(prog):
    """Random walls, some with one defect: the planner's verdict is the restatement's."""
    rng = np.random.default_rng(21)
    seen = set()
    for _ in range(60):
        w = plan_walls(40, seed=int(rng.integers(1 << 30)))
        defect = int(rng.integers(0, 8))
        k = int(rng.integers(0, 4))
        if defect == 1:
            w.normal[k] = 0.0
        elif defect == 2:
            w.nodes[1][0] = 41
        elif defect == 3:
            w.friction[k] = -w.friction[k] - 1.0
        elif defect == 4:
            w.amp[k] = 2
        elif defect == 5:
            w.origin[k, 1] = np.inf
        elif defect == 6:
            w.normal[k] = (1e-170, 1e-170, 0.0)              # its square underflows: the length is 0
        elif defect == 7:
            w.normal[k] = (1e200, 0.0, 1e200)                # its square overflows: the length is inf
        ok = run_plan(prog, 40, w)[0][0] == 0
        assert ok == R.valid(40, w), defect
        seen.add((defect, ok))
    assert {(0, True), (1, False), (6, False), (7, False)} <= seen


def test_whole_model_sum_order_and_lists():
    """wall_force on a mesh: three oblique walls in a corner add in index order, and the order matters."""
    m = mesh.bar_model(3, 3, 4, mesh.steel_elastic(), 0.0, perturb=0.05, seed=2, n_steps=10)
    rng = np.random.default_rng(8)
    disp = rng.normal(0, 0.05, 3 * m.nNode)
    pre = disp - rng.normal(0, 1e-6, 3 * m.nNode)
    c = m.coordmat.mean(axis=0)
    w = Walls(origin=[c, c, c], normal=[[1, 0.2, 0.1], [0.1, 1, 0.3], [0.2, 0.1, 1]], stiffness=[1e5, 2e5, 3e5],
              damping=[0.1, 0.2, 0.3], friction=[0.3, 0.2, 0.1])
    diag = np.repeat(rng.uniform(1e-7, 2e-7, m.nNode), 3)
    f = R.wall_force(m, w, diag, disp, pre, 3, 1e-7)
    fr = R.wall_force(m, w, diag, disp, pre, 3, 1e-7, reverse=True)
    assert np.any(f != fr) and np.allclose(f, fr, rtol=1e-12, atol=0)
    some = Walls(origin=[c], normal=[[1, 0.2, 0.1]], stiffness=[1e5], nodes=[[1, 2, 3]])
    fs = R.wall_force(m, some, diag, disp, pre, 3, 1e-7).reshape(-1, 3)
    assert np.all(fs[3:] == 0.0)
