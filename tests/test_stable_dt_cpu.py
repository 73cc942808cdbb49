"""The stable-time-step diagnostic (hakai_stable_dt) on the CPU.

  * The element arithmetic under test is the kernel's own: this file compiles
    hakai-fem_amd/csrc/hakai_stable_dt_elem.hpp, the header hakai_stable_dt.hip includes, with a host
    compiler (no contraction) and holds it against stable_dt_ref (NumPy) BIT FOR BIT on the shape
    cases of edge_cases (aspect 1:100, sheared, collapsed corner, left-handed, offset by 1e6) and on
    1000 random distorted elements.
  * An independent pin of the formulas: numpy_ref.element_update with an elastic material gives K_e
    column by column; K and the lumped mass are assembled and 2 / omega_max comes from a dense
    eigensolve. dt_safe <= dt_true (1 + 1e-9) on every case -- the slack is the eigensolver's rounding
    (order n 2^-53) and nothing else -- and on axis-aligned bricks at nu = 0 dt_est = dt_true to 1e-9
    (seen: 1e-15), which pins volume, face areas and wave speed together. The observed ratios go to
    profiles/stable_dt_tightness.json and are not asserted: they describe the estimator.
  * hakai_stable_dt_combine, the CSV round trip, and gather_stable_dt over gloo (world 2 and 3)."""
import ctypes
import json
import os
import socket
import subprocess

import numpy as np
import pytest
import torch.distributed as tdist      # (torch before the library loads, as test_dist_cpu.py has it)
import torch.multiprocessing as mp

import edge_cases
import numpy_ref
import stable_dt_ref as R
from hakai import mesh
from hakai.model import Material
from hakai.solver import read_stable_dt_csv, stable_dt_combine, write_stable_dt_csv
from util import bitwise_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC"]

# The harness only calls the header's functions.
SRC = r"""
#include <stdint.h>
#include "hakai_stable_dt_elem.hpp"
extern "C" {
void mat(double young, double poisson, double density, double mass_scaling, double* o) {
    const hk::StableMat m = hk::stable_mat(young, poisson, density, mass_scaling);
    o[0] = m.c; o[1] = m.Kb; o[2] = m.two_mu; o[3] = m.rho8;
}
/* x, X: [n][8][3]; mats: [n][4] = (c, Kb, two_mu, rho8) */
void run(const double* x, const double* X, const double* mats, int64_t n, double* est, double* safe) {
    for (int64_t e = 0; e < n; ++e) {
        double a[8][3], b[8][3];
        for (int i = 0; i < 8; ++i)
            for (int c = 0; c < 3; ++c) {
                a[i][c] = x[24 * e + 3 * i + c];
                b[i][c] = X[24 * e + 3 * i + c];
            }
        hk::StableMat m;
        m.c = mats[4 * e]; m.Kb = mats[4 * e + 1]; m.two_mu = mats[4 * e + 2]; m.rho8 = mats[4 * e + 3];
        hk::stable_element(a, b, m, est + e, safe + e);
    }
}
}
"""


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    d = tmp_path_factory.mktemp("stable_dt")
    c, so = d / "stable_dt.cpp", d / "stable_dt.so"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", CSRC, "-o", str(so), str(c)], check=True)
    lib = ctypes.CDLL(str(so))
    P, D = ctypes.c_void_p, ctypes.c_double
    lib.mat.argtypes = [D, D, D, D, P]
    lib.run.argtypes = [P, P, P, ctypes.c_int64, P, P]
    lib.mat.restype = lib.run.restype = None
    return lib


def header_elements(H, x, X, mats):
    x, X, mats = (np.ascontiguousarray(a, np.float64) for a in (x, X, mats))
    n = x.shape[0]
    est, safe = np.zeros(n), np.zeros(n)
    H.run(x.ctypes.data, X.ctypes.data, mats.ctypes.data, n, est.ctypes.data, safe.ctypes.data)
    return est, safe


def header_mat(H, *a):
    o = np.zeros(4)
    H.mat(*[float(v) for v in a], o.ctypes.data)
    return o


# ---- header == NumPy, bit for bit ----------------------------------------------------------------

def test_material_constants_bitwise(H):
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = (rng.uniform(1e3, 1e6), rng.uniform(0.0, 0.499), rng.uniform(1e-9, 1e-5), rng.choice([1.0, 100.0, 37.5]))
        assert bitwise_equal(header_mat(H, *a), np.array(R.stable_mat(*a)))


@pytest.mark.parametrize("kind", edge_cases.SHAPES)
def test_shape_cases_bitwise(H, kind):
    c = edge_cases.shape_case(kind)
    m = c["m"]
    n = m.elementmat - 1
    x, X = c["pos"][n], m.coordmat[n]
    k = np.tile(R.stable_mat(m.materials[0].young, m.materials[0].poisson, m.materials[0].density, 1.0), (len(n), 1))
    for cur in (x, X):                               # the case's positions as the current state, and at rest
        he, hs = header_elements(H, cur, X, k)
        re_, rs = R.elements(cur, X, k[:, 0], k[:, 1], k[:, 2], k[:, 3])
        assert bitwise_equal(he, re_) and bitwise_equal(hs, rs), kind
        assert np.all(np.isfinite(he)) and np.all(np.isfinite(hs))
    if kind == "inverted":                           # left-handed at rest: V0 <= 0 reports 0 for both
        he, hs = header_elements(H, X, X, k)
        assert np.all(he[::2] == 0.0) and np.all(hs[::2] == 0.0) and np.all(he[1::2] > 0) and np.all(hs[1::2] > 0)


def random_elements(n, seed):
    rng = np.random.default_rng(seed)
    X = 0.5 * numpy_ref.DELTA[None] + rng.normal(0, 0.12, size=(n, 8, 3))
    X = X * rng.uniform(0.05, 20.0, size=(n, 1, 3)) + rng.normal(0, 50.0, size=(n, 1, 3))
    F = np.eye(3) + rng.normal(0, 0.25, size=(n, 3, 3))
    x = np.einsum("nij,nkj->nki", F, X) + rng.normal(0, 0.02, size=(n, 8, 3))
    x[::7] = X[::7]                                  # some undeformed
    x[5::50, :, 2] = 0.0                             # some flattened into the plane z = 0: V = 0 exactly
    mats = np.array([R.stable_mat(rng.uniform(1e3, 1e6), rng.uniform(0.0, 0.499), rng.uniform(1e-9, 1e-5),
                                  rng.choice([1.0, 100.0])) for _ in range(n)])
    return x, X, mats


def test_random_elements_bitwise(H):
    x, X, k = random_elements(1000, 17)
    he, hs = header_elements(H, x, X, k)
    re_, rs = R.elements(x, X, k[:, 0], k[:, 1], k[:, 2], k[:, 3])
    assert bitwise_equal(he, re_) and bitwise_equal(hs, rs)
    assert np.all(he[5::50] == 0.0) and np.all(hs[5::50] == 0.0)
    live = he > 0
    assert live.sum() > 900 and np.all(np.isfinite(he)) and np.all(hs[live] > 0)


# ---- the bound against a dense eigensolve ----------------------------------------------------------

P = numpy_ref.pusai()


def element_K(xe, mat):
    """K_e (24, 24) at current node positions xe (8, 3): element_update's Qe for unit increments."""
    z6, z1 = np.zeros((8, 6)), np.zeros(8)
    K = np.zeros((24, 24))
    for j in range(24):
        du = np.zeros(24)
        du[j] = 1.0
        K[:, j] = numpy_ref.element_update(xe.T, du, z6, z6, z1, z1, mat)[4]
    return K


def dt_true(x, X, elem, mat, mass_scaling=1.0):
    """2 / omega_max of K (at x) against the lumped mass (from X) times mass_scaling, free-free."""
    nN = x.shape[0]
    K, M = np.zeros((3 * nN, 3 * nN)), np.zeros(nN)
    for e in range(elem.shape[0]):
        n = elem[e] - 1
        Ke = element_K(x[n], mat)
        dof = (3 * n[:, None] + np.arange(3)[None]).ravel()
        K[np.ix_(dof, dof)] += Ke
        V0 = sum(np.linalg.det(P[k] @ X[n]) for k in range(8))
        M[n] += mat.density * V0 / 8.0 * mass_scaling
    s = 1.0 / np.sqrt(np.repeat(M, 3))
    lam = np.linalg.eigvalsh(0.5 * (K + K.T) * s[:, None] * s[None, :])
    return 2.0 / np.sqrt(lam[-1])


def mesh_results(x, X, elem, mat, mass_scaling=1.0):
    k = np.tile(R.stable_mat(mat.young, mat.poisson, mat.density, mass_scaling), (elem.shape[0], 1))
    est, safe = R.elements(x[elem - 1], X[elem - 1], k[:, 0], k[:, 1], k[:, 2], k[:, 3])
    return est.min(), safe.min()


def eig_meshes():
    """name -> (x, X, elementmat, axis-aligned bricks)"""
    out = {}
    c, e = mesh.hex_bar(1, 1, 1)
    out["cube"] = (c, c, e, True)
    c, e = mesh.hex_bar(3, 3, 6)
    out["cubes_3x3x6"] = (c, c, e, True)
    c, e = mesh.hex_bar(4, 4, 4)
    c = c * np.array([1.0, 0.5, 0.25])
    out["bricks_4x4x4"] = (c, c, e, True)
    c, e = mesh.hex_bar(3, 3, 3, perturb=0.2, seed=7)
    out["jittered_3x3x3"] = (c, c, e, False)
    c, e = mesh.hex_bar(3, 3, 3, perturb=0.05, seed=8)
    F = np.array([[1.0, 0.3, 0.2], [0.0, 0.8, 0.1], [0.0, 0.0, 0.6]])
    out["sheared_compressed_3x3x3"] = (c @ F.T, c, e, False)   # mass from the undeformed mesh
    return out


MESHES = eig_meshes()
NUS = (0.0, 0.3, 0.45, 0.499)
RATIOS = {}


@pytest.mark.parametrize("nu", NUS)
@pytest.mark.parametrize("name", list(MESHES))
def test_dt_safe_is_a_lower_bound(name, nu):
    x, X, elem, bricks = MESHES[name]
    mat = Material("elastic", 7.8e-9, 210000.0, nu)
    true = dt_true(x, X, elem, mat)
    est, safe = mesh_results(x, X, elem, mat)
    RATIOS[f"{name}/nu={nu}"] = dict(dt_true=true, dt_safe_over_true=safe / true, dt_est_over_true=est / true)
    print(f"{name} nu={nu}: dt_true {true:.9e} dt_safe/dt_true {safe / true:.6f} dt_est/dt_true {est / true:.6f}")
    assert 0.0 < safe <= true * (1.0 + 1e-9)
    if bricks and nu == 0.0:
        print(f"   |dt_est - dt_true| / dt_true = {abs(est - true) / true:.3e}")
        assert abs(est - true) <= 1e-9 * true


@pytest.mark.parametrize("seed", range(12))
def test_dt_safe_random_meshes(seed):
    """Random small meshes: stretch, shear, jitter, nu and mass scaling drawn per mesh."""
    rng = np.random.default_rng(100 + seed)
    nx, ny, nz = rng.integers(1, 3, size=3)
    X, elem = mesh.hex_bar(int(nx), int(ny), int(nz), perturb=float(rng.uniform(0, 0.2)), seed=seed)
    X = X * rng.uniform(0.2, 3.0, size=3)
    F = np.eye(3) + rng.normal(0, 0.15, size=(3, 3))
    x = X @ F.T
    ms = float(rng.choice([1.0, 100.0]))
    mat = Material("elastic", 7.8e-9, 210000.0, float(rng.uniform(0.0, 0.499)))
    true = dt_true(x, X, elem, mat, mass_scaling=ms)
    est, safe = mesh_results(x, X, elem, mat, mass_scaling=ms)
    RATIOS[f"random_{seed}"] = dict(dt_true=true, dt_safe_over_true=safe / true, dt_est_over_true=est / true)
    print(f"random {seed}: dt_safe/dt_true {safe / true:.6f} dt_est/dt_true {est / true:.6f}")
    assert 0.0 < safe <= true * (1.0 + 1e-9)


def test_write_tightness_profile():
    """Not an assertion on the ratios: the ranges seen by the tests above, for the record."""
    if len(RATIOS) < len(MESHES) * len(NUS) + 12:
        return                                        # a partial session: nothing to record
    s = [v["dt_safe_over_true"] for v in RATIOS.values()]
    e = [v["dt_est_over_true"] for v in RATIOS.values()]
    doc = dict(what="dt_safe / dt_true and dt_est / dt_true of tests/test_stable_dt_cpu.py's eigensolve cases "
                    "(dt_true = 2 / omega_max of the assembled B-bar stiffness against the lumped mass, free-free)",
               dt_safe_over_true=[min(s), max(s)], dt_est_over_true=[min(e), max(e)], cases=RATIOS)
    try:
        with open(os.path.join(ROOT, "profiles", "stable_dt_tightness.json"), "w") as fh:
            json.dump(doc, fh, indent=1, sort_keys=True)
            fh.write("\n")
    except OSError:
        pass                                          # a read-only tree: the record is optional


# ---- combine, CSV, gather ---------------------------------------------------------------------------

def rec(est, ee, safe, es, na=0, ne=0, ns=0):
    return dict(dt_est=est, element_est=ee, dt_safe=safe, element_safe=es, n_active=na, n_est_below=ne,
                n_safe_below=ns)


def test_combine():
    inf = float("inf")
    a, b, c = rec(2.0, 7, 1.0, 3, 10, 1, 2), rec(2.0, 5, 1.5, 40, 20, 3, 4), rec(3.0, 90, 1.0, 2, 5, 0, 1)
    assert stable_dt_combine([a, b, c]) == rec(2.0, 5, 1.0, 2, 35, 4, 7)      # ties: the lower element id
    assert stable_dt_combine([c, b, a]) == rec(2.0, 5, 1.0, 2, 35, 4, 7)
    assert stable_dt_combine([a]) == a
    empty = rec(inf, 0, inf, 0)
    assert stable_dt_combine([empty, a, empty]) == a                            # an empty rank does not win
    assert stable_dt_combine([empty, rec(inf, 4, inf, 9, 1)]) == rec(inf, 4, inf, 9, 1)
    assert stable_dt_combine([empty, empty]) == empty
    assert stable_dt_combine([rec(0.0, 12, 0.0, 12, 1, 1, 1), a]) == rec(0.0, 12, 0.0, 12, 11, 2, 3)


def test_csv_round_trip(tmp_path):
    inf = float("inf")
    recs = [rec(5e-324, 1, 2.2250738585072014e-308, 2 ** 40, 3, 1, 2), rec(inf, 0, inf, 0),
            rec(0.1 + 0.2, 17, 1.7976931348623157e308, 9, 2 ** 33, 5, 6), rec(0.0, 3, 1e-7 / 3, 4, 1, 1, 1)]
    steps = [0, 2, 4, 10 ** 6]
    p = tmp_path / "stable_dt.csv"
    write_stable_dt_csv(p, steps, recs, 1e-7 / 7)
    head = open(p).readline().strip()
    assert head == "step,time,d_time,dt_est,element_est,dt_safe,element_safe,n_active,n_est_below,n_safe_below"
    back = read_stable_dt_csv(p)
    assert back["records"] == recs and list(back["steps"]) == steps
    assert bitwise_equal(back["d_time"], np.full(4, 1e-7 / 7))
    assert bitwise_equal(back["time"], np.array(steps, np.float64) * (1e-7 / 7))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_records(rank, n=3):
    inf = float("inf")
    out = [rec(1.0 + rank + i, 100 * rank + i + 1, 5e-324 * (rank + 1), 100 * rank + 2, 10 + rank, i, rank)
           for i in range(n - 1)]
    return out + [rec(inf, 0, inf, 0)]


def _gather_worker(rank, world, port, ret):
    from hakai.run import gather_stable_dt
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        got = gather_stable_dt(tdist, None, rank, world, _rank_records(rank))
        ret[rank] = got
    finally:
        tdist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_stable_dt_gloo(world):
    ctx = mp.get_context("spawn")
    ret = ctx.Manager().dict()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, ret)) for r in range(world)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(120)
        assert p.exitcode == 0
    assert ret[0] == [_rank_records(r) for r in range(world)]
    assert all(ret[r] is None for r in range(1, world))
    combined = [stable_dt_combine(list(p)) for p in zip(*ret[0])]
    assert combined[0] == rec(1.0, 1, 5e-324, 2, sum(10 + r for r in range(world)), 0, sum(range(world)))
    assert combined[-1] == rec(float("inf"), 0, float("inf"), 0)
