"""Selective mass scaling (hakai_mass_scale) on the CPU.

  * The element rule under test is the kernel's own: this file compiles
    hakai-fem_amd/csrc/hakai_mass_scale_elem.hpp, the header hakai_mass_scale.hip and
    hakai_stable_dt.hip include, into a small stand-alone program (its own main, built with
    -fsanitize=address,undefined and no contraction) and holds it against mass_scale_ref (NumPy) BIT
    FOR BIT: a unit cube, a perturbed cube, a sliver at 1/20 thickness, an inverted element, an exactly
    collapsed Gauss point (unfixable), V0 <= 0, a capped element, added_prev above and below the need,
    and 200 random elements.
  * The chain from kappa and m0 to dt_safe is held against exact rational arithmetic within the
    rounding count of mass_scale_ref's docstring: (dt_safe / 2)^2 >= h^2 (1 - u)^8, and no more than
    (1 + u)^8 above where the call set the mass. (kappa and m0 themselves are hakai_stable_dt's,
    pinned against dense eigensolves by tests/test_stable_dt_cpu.py.)
  * The guarantee by eigenvalues: meshes with one squeezed layer, the target 0.9 of the regular
    elements' dt_safe; the unscaled 2 / omega_max is below the target (the case is not vacuous) and
    with the scaled nodal masses it is >= dt_target (1 - 1e-9), the eigensolver's allowance of
    tests/test_stable_dt_cpu.py.
  * Idempotence, monotonicity, the no-op, and the bound on mass_added against math.fsum."""
import math
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import mass_scale_ref as MR
import numpy_ref
import stable_dt_ref as R
from hakai import mesh
from hakai.model import Material
from util import bitwise_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
CXXFLAGS = ["-std=c++17", "-O2", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
            "-fno-sanitize-recover=undefined"]
U = 2.0 ** -53
SAFE1 = 1.0 - 2.0 ** -40

# The harness only moves bytes: it calls the header's functions.
SRC = r"""
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "hakai_mass_scale_elem.hpp"
/* in: int64 n, double dt_target, safety, max_factor, then x[n][8][3], X[n][8][3], mats[n][4] =
   (c, Kb, two_mu, rho8), prev[n]; out: half, then added[n], status[n], factor[n], est[n], safe[n] */
int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* fi = std::fopen(argv[1], "rb");
    if (!fi) return 3;
    int64_t n = 0;
    double par[3];
    if (std::fread(&n, sizeof n, 1, fi) != 1 || std::fread(par, sizeof(double), 3, fi) != 3) return 3;
    std::vector<double> x(24 * n), X(24 * n), mats(4 * n), prev(n), out(1 + 5 * n);
    if (n && (std::fread(x.data(), 8, x.size(), fi) != x.size() || std::fread(X.data(), 8, X.size(), fi) != X.size() ||
              std::fread(mats.data(), 8, mats.size(), fi) != mats.size() ||
              std::fread(prev.data(), 8, prev.size(), fi) != prev.size()))
        return 3;
    std::fclose(fi);
    const double half = hk::mass_half(par[0], par[1]);
    out[0] = half;
    for (int64_t e = 0; e < n; ++e) {
        double a[8][3], b[8][3];
        for (int i = 0; i < 8; ++i)
            for (int c = 0; c < 3; ++c) {
                a[i][c] = x[24 * e + 3 * i + c];
                b[i][c] = X[24 * e + 3 * i + c];
            }
        hk::StableMat m;
        m.c = mats[4 * e]; m.Kb = mats[4 * e + 1]; m.two_mu = mats[4 * e + 2]; m.rho8 = mats[4 * e + 3];
        int status = -1;
        double factor, est, safe;
        out[1 + e] = hk::mass_element(a, b, m, half, par[2], prev[e], &status, &factor, &est, &safe);
        out[1 + n + e] = status;
        out[1 + 2 * n + e] = factor;
        out[1 + 3 * n + e] = est;
        out[1 + 4 * n + e] = safe;
    }
    FILE* fo = std::fopen(argv[2], "wb");
    if (!fo || std::fwrite(out.data(), 8, out.size(), fo) != out.size()) return 4;
    std::fclose(fo);
    return 0;
}
"""


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    d = tmp_path_factory.mktemp("mass_scale")
    c, exe = d / "mass_scale_check.cpp", d / "mass_scale_check"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", CSRC, "-o", str(exe), str(c)], check=True)
    count = [0]

    def run(x, X, mats, prev, dt_target, safety, max_factor):
        count[0] += 1
        fi, fo = d / f"in{count[0]}.bin", d / f"out{count[0]}.bin"
        n = len(prev)
        arrays = [np.array([n], np.int64), np.array([dt_target, safety, max_factor], np.float64)]
        arrays += [np.ascontiguousarray(a, np.float64) for a in (x, X, mats, prev)]
        fi.write_bytes(b"".join(a.tobytes() for a in arrays))
        subprocess.run([str(exe), str(fi), str(fo)], check=True)      # a sanitizer report fails the run
        o = np.frombuffer(fo.read_bytes(), np.float64)
        return dict(half=o[0], added=o[1:1 + n], status=o[1 + n:1 + 2 * n].astype(np.int64),
                    factor=o[1 + 2 * n:1 + 3 * n], est=o[1 + 3 * n:1 + 4 * n], safe=o[1 + 4 * n:1 + 5 * n])
    return run


def ref_elements(x, X, mats, prev, dt_target, safety, max_factor):
    x, X, k = (np.ascontiguousarray(a, np.float64) for a in (x, X, mats))
    V, gg, ss, V0, Amax = MR.sums(x, X)
    half = MR.half_of(dt_target, safety)
    added, status = MR.need(V, gg, ss, V0, k[:, 1], k[:, 2], k[:, 3], half, max_factor, prev)
    est, safe = MR.finish_added(V, gg, ss, V0, Amax, k[:, 0], k[:, 1], k[:, 2], k[:, 3], added)
    fac = np.where(V0 > 0.0, MR.factor(V0, k[:, 3], added), 0.0)
    with np.errstate(all="ignore"):
        kappa = (k[:, 1] * V) * gg + k[:, 2] * ss
    return dict(half=half, added=added, status=status, factor=fac, est=est, safe=safe, kappa=kappa, m0=k[:, 3] * V0,
                V0=V0, V=V)


def same(got, ref):
    assert bitwise_equal(np.float64(got["half"]), np.float64(ref["half"]))
    for key in ("added", "factor", "est", "safe"):
        assert bitwise_equal(got[key], ref[key]), key
    assert np.array_equal(got["status"], ref["status"])


STEEL = R.stable_mat(210000.0, 0.3, 7.8e-9, 1.0)
CUBE = 0.5 * (numpy_ref.DELTA + 1.0)                    # the unit cube, C3D8 node order


def collapsed_gauss_point(k=0):
    """Current positions with J's first row EXACTLY zero at Gauss point k, so a_k = 0 and s_k = +inf
    while the other Gauss points keep a volume: the xi-edges 4-5 and 7-6 have length 0 (their two
    terms cancel exactly, P[0][i] of an edge's ends being exact negatives), edge 0-1 is (wB, 0, 0) and
    edge 3-2 is (-wA, 0, 0) with wA = |P_k[0][0]|, wB = |P_k[0][3]|: wA wB - wB wA = 0 in floating point."""
    P = numpy_ref.pusai()[k]
    wA, wB = abs(P[0, 0]), abs(P[0, 3])
    x = np.array([[0, 0, 0], [wB, 0, 0], [-wA, 1, 0], [0, 1, 0], [0, 0, 1], [0, 0, 1], [0, 1, 1], [0, 1, 1]], float)
    return x


def special_cases():
    """name -> (x, X, prev, dt_target, safety, max_factor, expected status)"""
    rng = np.random.default_rng(3)
    out = {}
    dt_cube = float(ref_elements(CUBE[None], CUBE[None], [STEEL], [0.0], 1.0, 1.0, 1.0)["safe"][0])
    out["unit_cube_below_target"] = (CUBE, CUBE, 0.0, 2.0 * dt_cube, 0.9, np.inf, MR.OK)
    out["unit_cube_above_target"] = (CUBE, CUBE, 0.0, 0.5 * dt_cube, 0.9, np.inf, MR.OK)
    pert = CUBE + rng.normal(0, 0.08, size=(8, 3))
    out["perturbed_cube"] = (pert + rng.normal(0, 0.01, size=(8, 3)), pert, 0.0, dt_cube, 0.9, np.inf, MR.OK)
    sliver = CUBE * np.array([1.0, 1.0, 0.05])
    out["sliver_1_20"] = (sliver, sliver, 0.0, dt_cube, SAFE1, np.inf, MR.OK)
    inv = CUBE[[4, 5, 6, 7, 0, 1, 2, 3]]
    out["inverted"] = (inv, inv, 0.25e-9, dt_cube, 0.9, np.inf, MR.UNFIXABLE)
    out["collapsed_gauss_point"] = (collapsed_gauss_point(), CUBE, 0.5e-9, dt_cube, 0.9, np.inf, MR.UNFIXABLE)
    out["flat_V_zero"] = (CUBE * np.array([1.0, 1.0, 0.0]), CUBE, 0.0, dt_cube, 0.9, np.inf, MR.UNFIXABLE)
    out["V0_zero"] = (CUBE, CUBE * np.array([1.0, 1.0, 0.0]), 0.0, dt_cube, 0.9, np.inf, MR.UNFIXABLE)
    out["capped"] = (sliver, sliver, 0.0, dt_cube, 0.9, 1.5, MR.CAPPED)
    out["capped_at_one"] = (sliver, sliver, 0.0, dt_cube, 0.9, 1.0, MR.CAPPED)
    a = float(ref_elements(sliver[None], sliver[None], [STEEL], [0.0], dt_cube, 0.9, np.inf)["added"][0])
    assert a > 0
    out["prev_above"] = (sliver, sliver, 2.0 * a, dt_cube, 0.9, np.inf, MR.OK)
    out["prev_below"] = (sliver, sliver, 0.5 * a, dt_cube, 0.9, np.inf, MR.OK)
    out["prev_equal"] = (sliver, sliver, a, dt_cube, 0.9, np.inf, MR.OK)
    return out


SPECIAL = special_cases()


@pytest.mark.parametrize("name", list(SPECIAL))
def test_special_cases_bitwise(prog, name):
    x, X, prev, dt, s, mf, status = SPECIAL[name]
    args = (x[None], X[None], np.array([STEEL]), np.array([prev]), dt, s, mf)
    got, ref = prog(*args), ref_elements(*args)
    same(got, ref)
    assert got["status"][0] == status
    added = got["added"][0]
    if status == MR.UNFIXABLE:
        assert added == prev
    if name == "collapsed_gauss_point":
        assert np.isinf(ref["kappa"][0]) and ref["V"][0] > 0 and ref["V0"][0] > 0 and got["safe"][0] == 0.0
    if name == "unit_cube_above_target":
        assert added == 0.0 and got["factor"][0] == 1.0
        plain = R.elements(x[None], X[None], *STEEL)
        assert bitwise_equal(got["est"], plain[0]) and bitwise_equal(got["safe"], plain[1])   # added == 0: stable_finish's bits
    if name in ("unit_cube_below_target", "sliver_1_20", "perturbed_cube"):
        assert added > 0 and got["safe"][0] >= dt and got["factor"][0] > 1.0
    if name == "capped":
        assert got["factor"][0] == pytest.approx(1.5, rel=1e-15) and got["safe"][0] < dt
    if name == "capped_at_one":
        assert added == 0.0
    if name in ("prev_above", "prev_equal"):
        assert added == prev
    if name == "prev_below":
        assert added == 2.0 * prev


def random_elements(n, seed):
    rng = np.random.default_rng(seed)
    X = 0.5 * numpy_ref.DELTA[None] + rng.normal(0, 0.12, size=(n, 8, 3))
    X = X * rng.uniform(0.05, 20.0, size=(n, 1, 3)) + rng.normal(0, 50.0, size=(n, 1, 3))
    F = np.eye(3) + rng.normal(0, 0.25, size=(n, 3, 3))
    x = np.einsum("nij,nkj->nki", F, X) + rng.normal(0, 0.02, size=(n, 8, 3))
    x[::7] = X[::7]                                      # some undeformed
    x[5::50, :, 2] = 0.0                                 # some flattened into the plane z = 0: V = 0 exactly
    mats = np.array([R.stable_mat(rng.uniform(1e3, 1e6), rng.uniform(0.0, 0.499), rng.uniform(1e-9, 1e-5),
                                  rng.choice([1.0, 100.0])) for _ in range(n)])
    return x, X, mats, rng


@pytest.mark.parametrize("safety,max_factor", [(0.9, np.inf), (SAFE1, np.inf), (1.0, 3.0)])
def test_random_elements_bitwise(prog, safety, max_factor):
    x, X, k, rng = random_elements(200, 23)
    free = ref_elements(x, X, k, np.zeros(200), 1.0, 1.0, 1.0)
    dt = float(np.median(free["safe"][free["safe"] > 0]))                 # about half the elements are below
    none = ref_elements(x, X, k, np.zeros(200), dt, safety, max_factor)
    prev = none["added"] * rng.choice([0.0, 0.5, 1.0, 2.0], size=200)      # below, at and above the need
    args = (x, X, k, prev, dt, safety, max_factor)
    got, ref = prog(*args), ref_elements(*args)
    same(got, ref)
    st = got["status"]
    assert (st == MR.UNFIXABLE).sum() >= 4 and (st == MR.OK).sum() > 100
    assert ((st == MR.CAPPED).sum() > 0) == np.isfinite(max_factor)
    assert np.all(got["added"] >= prev) and np.all(got["added"] >= 0)
    if safety <= SAFE1:
        assert np.all(got["safe"][st == MR.OK] >= dt)                      # the guarantee, element by element


def test_chain_against_exact_rationals():
    """From the float kappa and m0 to dt_safe in exact rational arithmetic: the squared half step
    (dt_safe / 2)^2 is within (1 -+ u)^8 of h^2 = (dt / (2 safety))^2 where the call set the mass."""
    x, X, k, _ = random_elements(200, 29)
    free = ref_elements(x, X, k, np.zeros(200), 1.0, 1.0, 1.0)
    dt = float(np.quantile(free["safe"][free["safe"] > 0], 0.8))
    lo, hi = (1 - Fraction(U)) ** 8, (1 + Fraction(U)) ** 8
    checked = 0
    for s in (0.9, SAFE1, 1.0):
        r = ref_elements(x, X, k, np.zeros(200), dt, s, np.inf)
        h2 = (Fraction(dt) / (2 * Fraction(s))) ** 2
        for e in np.nonzero((r["status"] == MR.OK) & (r["added"] > 0))[0]:
            half2 = (Fraction(float(r["safe"][e])) / 2) ** 2
            assert h2 * lo <= half2 <= h2 * hi, (e, s)
            # and the added mass itself: a = kappa h^2 - m0 within 4 roundings of kappa h^2
            a, p = Fraction(float(r["added"][e])), Fraction(float(r["kappa"][e])) * h2
            assert abs(a - (p - Fraction(float(r["m0"][e])))) <= 5 * Fraction(U) * p, (e, s)
            checked += 1
    assert checked > 300


# ---- the guarantee against a dense eigensolve -------------------------------------------------------

P = numpy_ref.pusai()


def element_K(xe, mat):
    """K_e (24, 24) at node positions xe (8, 3): element_update's Qe for unit increments
    (tests/test_stable_dt_cpu.py's)."""
    z6, z1 = np.zeros((8, 6)), np.zeros(8)
    K = np.zeros((24, 24))
    for j in range(24):
        du = np.zeros(24)
        du[j] = 1.0
        K[:, j] = numpy_ref.element_update(xe.T, du, z6, z6, z1, z1, mat)[4]
    return K


def dt_true(x, elem, mat, M):
    """2 / omega_max of K (at x) against the nodal masses M (nN,), free-free."""
    nN = x.shape[0]
    K = np.zeros((3 * nN, 3 * nN))
    for e in range(elem.shape[0]):
        n = elem[e] - 1
        dof = (3 * n[:, None] + np.arange(3)[None]).ravel()
        K[np.ix_(dof, dof)] += element_K(x[n], mat)
    s = 1.0 / np.sqrt(np.repeat(M, 3))
    lam = np.linalg.eigvalsh(0.5 * (K + K.T) * s[:, None] * s[None, :])
    return 2.0 / np.sqrt(lam[-1])


def scale_mesh(x, X, elem, mat, dt_target, safety, max_factor=np.inf, prev=None):
    """mass_scale_ref on a bare mesh: (record arrays, M0, M)."""
    k = np.tile(R.stable_mat(mat.young, mat.poisson, mat.density, 1.0), (elem.shape[0], 1))
    n = elem - 1
    prev = np.zeros(len(elem)) if prev is None else prev
    r = ref_elements(x[n], X[n], k, prev, dt_target, safety, max_factor)
    M0 = MR.nodal_mass(np.zeros(x.shape[0]), elem, r["m0"])              # the lumped mass, hakai_lumped_mass's order
    return r, M0, MR.nodal_mass(M0, elem, r["added"])


def squeezed(nx, ny, nz, layer, ratio, perturb=0.0, seed=0):
    """A bar whose node layers above `layer` are drawn down so that element layer `layer` keeps
    `ratio` of its thickness."""
    c, e = mesh.hex_bar(nx, ny, nz, perturb=perturb, seed=seed)
    z = c[:, 2].copy()
    c[:, 2] = np.where(z > layer + 0.5, z - (1.0 - ratio), z)
    return c, e


def check_guarantee(x, X, elem, mat, regular, safety):
    free, M0, _ = scale_mesh(x, X, elem, mat, 1.0, 1.0, 1.0)             # max_factor 1: nothing is added
    dt_target = 0.9 * float(np.min(free["safe"][regular]))
    before = dt_true(x, elem, mat, M0)
    assert before < dt_target                                             # not vacuous: the step is unstable unscaled
    r, M0b, M = scale_mesh(x, X, elem, mat, dt_target, safety)
    assert bitwise_equal(M0, M0b) and np.all(M >= M0) and (r["added"] > 0).any()
    assert not (r["added"][regular] > 0).any()                            # selective: the regular elements keep their mass
    after = dt_true(x, elem, mat, M)
    print(f"dt_true {before:.6e} -> {after:.6e}, target {dt_target:.6e}, min dt_safe {r['safe'].min():.6e}, "
          f"mass x {M.sum() / M0.sum():.4f}")
    assert r["safe"].min() >= dt_target
    assert after >= dt_target * (1.0 - 1e-9)


@pytest.mark.parametrize("nu", (0.0, 0.3, 0.45, 0.499))
def test_guarantee_squeezed_layer(nu):
    mat = Material("elastic", 7.8e-9, 210000.0, nu)
    c, e = squeezed(2, 2, 5, 2, 0.1)
    regular = np.ones(len(e), bool)
    regular[8:12] = False                                                 # element layer 2 (hex_bar counts z slowest)
    zc = c[e - 1][:, :, 2]
    assert np.all((zc.max(axis=1) - zc.min(axis=1) < 0.5) == ~regular)
    check_guarantee(c, c, e, mat, regular, SAFE1)


@pytest.mark.parametrize("seed", range(6))
def test_guarantee_random_meshes(seed):
    """Random small jittered, scaled and sheared meshes with one squeezed layer; nu and the safety drawn
    per mesh. (The layer's nodes take half their mass from the regular neighbours, so the unscaled
    critical step falls only like the root of the thickness ratio: 0.02 .. 0.06 puts it below the target.)"""
    rng = np.random.default_rng(300 + seed)
    nx, ny = (int(v) for v in rng.integers(1, 3, size=2))
    nz = int(rng.integers(3, 5))
    layer = int(rng.integers(0, nz))
    X, e = squeezed(nx, ny, nz, layer, float(rng.uniform(0.02, 0.06)), perturb=float(rng.uniform(0, 0.02)), seed=seed)
    zc = X[e - 1][:, :, 2]
    regular = zc.max(axis=1) - zc.min(axis=1) > 0.6
    assert 0 < regular.sum() < len(e)
    X = X * float(rng.uniform(0.5, 2.0))
    x = X @ (np.eye(3) + rng.normal(0, 0.05, size=(3, 3))).T              # a deformed current state
    mat = Material("elastic", 7.8e-9, 210000.0, float(rng.uniform(0.0, 0.499)))
    check_guarantee(x, X, e, mat, regular, float(rng.choice([0.9, SAFE1])))


# ---- smaller properties ---------------------------------------------------------------------------------

def test_idempotent_and_monotone():
    mat = Material("elastic", 7.8e-9, 210000.0, 0.3)
    c, e = squeezed(2, 2, 5, 1, 0.2, perturb=0.05, seed=4)
    free, M0, _ = scale_mesh(c, c, e, mat, 1.0, 1.0, 1.0)
    dt = float(np.quantile(free["safe"], 0.6))
    a, _, Ma = scale_mesh(c, c, e, mat, dt, 0.9)
    b, _, Mb = scale_mesh(c, c, e, mat, dt, 0.9, prev=a["added"])         # the same call again
    assert bitwise_equal(a["added"], b["added"]) and bitwise_equal(Ma, Mb) and not (b["added"] > a["added"]).any()
    x2 = 1.25 * c                                                         # dilated at the same mass: kappa grows with the length
    d, _, Md = scale_mesh(x2, c, e, mat, dt, 0.9, prev=a["added"])
    assert np.all(d["added"] >= a["added"]) and (d["added"] > a["added"]).any() and np.all(Md >= Ma)
    x3 = 0.8 * c                                                          # shrunk: less needed, nothing taken back
    f, _, Mf = scale_mesh(x3, c, e, mat, dt, 0.9, prev=d["added"])
    assert bitwise_equal(f["added"], d["added"]) and bitwise_equal(Mf, Md)
    g, _, Mg = scale_mesh(c, c, e, mat, 0.5 * dt, 0.9, prev=d["added"])   # a smaller target: nothing taken back either
    assert bitwise_equal(g["added"], d["added"])


def test_target_below_every_element_changes_no_bit():
    mat = Material("elastic", 7.8e-9, 210000.0, 0.3)
    c, e = squeezed(2, 3, 4, 1, 0.2, perturb=0.1, seed=6)
    free, M0, _ = scale_mesh(c, c, e, mat, 1.0, 1.0, 1.0)
    r, _, M = scale_mesh(c, c, e, mat, 0.9 * 0.999 * float(free["safe"].min()), 0.9)
    assert not r["added"].any() and bitwise_equal(M, M0)
    assert bitwise_equal(r["safe"], free["safe"]) and bitwise_equal(r["est"], free["est"])
    assert np.all(r["factor"] == 1.0)


@pytest.mark.parametrize("n", [0, 1, 2, 3, 31, 32, 33, 1000, 8193])
def test_mass_added_tree_bound(n):
    rng = np.random.default_rng(n)
    v = 8.0 * np.where(rng.random(n) < 0.3, 0.0, rng.lognormal(-20, 3, size=n))
    tree, exact = MR.tree_sum(v), math.fsum(v)
    levels = math.ceil(math.log2(n)) if n > 1 else 0
    assert abs(tree - exact) <= levels * U * exact * (1 + 1e-6) + 0.0
    if n in (1, 2):
        assert tree == exact
    # zero padding to whole 32-element blocks and to a power of two is the same tree, the same bits
    pad = np.concatenate([v, np.zeros((-n) % 32)])
    assert MR.tree_sum(pad) == tree
    if n:
        full = np.concatenate([v, np.zeros(2 ** math.ceil(math.log2(max(n, 1))) - n)])
        assert MR.tree_sum(full) == tree
