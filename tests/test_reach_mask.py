"""reach_mask (hakai-fem_amd/csrc/hakai_contact_cells.hpp), the one approximate filter of the contact
search, against its defining property. The function under test is the kernel's own: this file
compiles the header the contact kernels include with a host compiler (no contraction, as the kernel
file is built); the reference side is a plain numpy restatement of the reference's two tests and
never calls the header.

Property. For a candidate with first-node cell mj, sphere (c, Rmax) and a grid (amn, ddiv): every
point p with m(p) = ceil((p - amn) / ddiv) in double, |m(p) - mj| <= 1 on every axis and
sqrt(dx^2 + dy^2 + dz^2) < Rmax in double (d = p - c, no contraction) -- that is, every i-node the
reference's cell test and sphere test (v2/HAKAI_j.jl:2496-2536) let through -- has the bit of its
cell m(p) - mj set. A cleared bit there is a silently lost contact event.

Classes: Rmax / ddiv in {0.05, 0.4, 1, 3} x |amn| in {0, 1, 2^20, 2^40} x ddiv in {2^-10, 0.6, 1.1,
1e3}; the centre c anywhere in the first-node cell, its faces and corners included, and (a quarter
of the configurations) up to Rmax away from a first node in that cell, as a triangle's centroid is.
Points: for each of the 27 cells the point of the cell nearest to c moved 0..4 ulps into the cell and
out of it; points on 64 rays from c at distance Rmax (1 - k 2^-52), k = 0..7; uniform random points
in the sphere's bounding cube and in the 27-cell block. Every trial is evaluated; every class must
yield at least 1000 (point, cell) pairs that pass the two tests, so none is vacuous.

Tightness. A ball with Rmax <= 0.4 ddiv meets at most two cells per axis, so its mask has at most 8
bits wherever the widenings of the cull are small against the slack ddiv - 2 Rmax >= 0.2 ddiv. The
widenings are the documented ones, per box face 1e-9 ddiv + 1e-12 (|amn| + |m| ddiv) and on the
radius 1e-9 (Rmax + ddiv): the bound is asserted where twice their sum is below a tenth of the
slack. That holds in every class but three, |amn| = 2^40 with ddiv = 2^-10, 0.6 and 1.1, where the
term 1e-12 |amn| = 1.1 alone exceeds the cell: at such coordinates a double resolves 2^-12, a
quarter of the smallest cell, and the cull deliberately keeps everything (asserted as such: the
exemption is exactly those three).
"""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "hakai-fem_amd", "csrc")
CXXFLAGS = ["-std=c++17", "-O2", "-ffp-contract=off", "-shared", "-fPIC"]

SRC = r"""
#include <stdint.h>
#include "hakai_contact_cells.hpp"
extern "C" {
void masks(int64_t n, const int64_t* mj, const double* c, const double* Rmax, const double* amn, const double* ddiv,
           uint32_t* out) {
    for (int64_t i = 0; i < n; ++i) {
        const long long m[3] = {(long long)mj[3 * i], (long long)mj[3 * i + 1], (long long)mj[3 * i + 2]};
        out[i] = hk::reach_mask(m, c + 3 * i, Rmax[i], amn + 3 * i, ddiv[i]);
    }
}
void cells(int64_t n, const double* p, const double* amn, const double* ddiv, int64_t* out) {
    for (int64_t i = 0; i < n; ++i) out[i] = hk::cell_index(p[i], amn[i], ddiv[i]);
}
}
"""

RATIOS = (0.05, 0.4, 1.0, 3.0)
AMAGS = (0.0, 1.0, 2.0 ** 20, 2.0 ** 40)
DDIVS = (2.0 ** -10, 0.6, 1.1, 1e3)
ALL = (1 << 27) - 1
N_CFG = 48


@pytest.fixture(scope="module")
def L(tmp_path_factory):
    d = tmp_path_factory.mktemp("reach_mask")
    c, so = d / "cells.cpp", d / "cells.so"
    c.write_text(SRC)
    subprocess.run(["g++", *CXXFLAGS, "-I", CSRC, "-o", str(so), str(c)], check=True)
    return ctypes.CDLL(str(so))


def _masks(L, mj, c, Rmax, amn, ddiv):
    n = len(Rmax)
    mj = np.ascontiguousarray(mj, np.int64)
    c, amn = np.ascontiguousarray(c, np.float64), np.ascontiguousarray(amn, np.float64)
    Rmax = np.ascontiguousarray(Rmax, np.float64)
    dd = np.full(n, ddiv, np.float64)
    out = np.zeros(n, np.uint32)
    P = ctypes.c_void_p
    L.masks(ctypes.c_int64(n), P(mj.ctypes.data), P(c.ctypes.data), P(Rmax.ctypes.data), P(amn.ctypes.data),
            P(dd.ctypes.data), P(out.ctypes.data))
    return out


def _move(x, steps):
    """x moved steps ulps (integer array, either sign), elementwise."""
    x = x.copy()
    for k in range(1, int(np.max(np.abs(steps))) + 1):
        up = np.nextafter(x, np.inf)
        dn = np.nextafter(x, -np.inf)
        x = np.where(steps >= k, up, np.where(steps <= -k, dn, x))
    return x


_LATTICE = np.array([d for d in itertools.product((-1.0, 0.0, 1.0), repeat=3) if any(d)])


def _configs(rng, ratio, amag, ddiv):
    """N_CFG candidates of one class: (mj, c, Rmax, amn)."""
    n = N_CFG
    amn = amag * rng.choice([-1.0, 1.0], (n, 3)) * np.where(rng.random((n, 3)) < 0.5, 1.0, rng.uniform(0.5, 1, (n, 3)))
    mj = rng.choice([-3, -1, 0, 1, 2, 7, 40, 1000], (n, 3)).astype(np.int64)
    # u = 0: the cell's upper face (in the cell), u = 1: its lower face, else inside
    kind = rng.integers(0, 3, (n, 3))
    u = np.where(kind == 0, 0.0, np.where(kind == 1, 1.0, rng.random((n, 3))))
    u[0], u[1] = 0.0, 1.0                                    # two whole corners
    c = amn + (mj - u) * ddiv
    Rmax = ratio * ddiv * np.where(rng.random(n) < 0.5, 1.0, 1.0 - 2.0 ** -rng.integers(2, 50, n))
    far = np.arange(n) >= 3 * n // 4                          # c up to Rmax from a first node in the cell
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    c = np.where(far[:, None], c + dirs * (Rmax * rng.random(n))[:, None], c)
    return mj, c, Rmax, amn


def _points(rng, mj, c, Rmax, amn, ddiv):
    """Trial points (n_cfg, P, 3) of the three generators."""
    n = len(Rmax)
    out = []
    # 1. nearest point of each of the 27 cells, 0..4 ulps into the cell and out of it
    k = np.array(list(itertools.product((-1, 0, 1), repeat=3)))[:, ::-1]          # (27, 3), dx fastest
    m = (mj[:, None, :] + k[None, :, :]).astype(np.float64)                       # (n, 27, 3)
    lo = amn[:, None, :] + (m - 1.0) * ddiv
    hi = amn[:, None, :] + m * ddiv
    cc = np.broadcast_to(c[:, None, :], m.shape)
    q = np.clip(cc, lo, hi)
    inward = np.where(cc < lo, 1, np.where(cc > hi, -1, 0))
    for j in range(-4, 5):
        out.append(_move(q, inward * j))
    # 2. rays from c at distance Rmax (1 - k 2^-52)
    dirs = np.concatenate([_LATTICE / np.linalg.norm(_LATTICE, axis=1, keepdims=True),
                           (lambda g: g / np.linalg.norm(g, axis=1, keepdims=True))(rng.normal(size=(38, 3)))])
    for j in range(8):
        dist = Rmax * (1.0 - j * 2.0 ** -52)
        out.append(c[:, None, :] + dirs[None, :, :] * dist[:, None, None])
    # 3. uniform in the sphere's bounding cube and in the 27-cell block
    out.append(c[:, None, :] + rng.uniform(-1.05, 1.05, (n, 400, 3)) * Rmax[:, None, None])
    out.append(amn[:, None, :] + (mj[:, None, :] + rng.uniform(-2.0, 1.0, (n, 200, 3))) * ddiv)
    return np.concatenate(out, axis=1)


def _passing(p, mj, c, Rmax, amn, ddiv):
    """The reference's two tests, restated: (passes (n, P), bit index of the point's cell (n, P))."""
    m = np.ceil((p - amn[:, None, :]) / ddiv)
    dm = m - mj[:, None, :]
    near = np.all(np.abs(dm) <= 1.0, axis=2)
    d = p - c[:, None, :]
    dist = np.sqrt(d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2])
    ok = near & (dist < Rmax[:, None])
    bit = np.where(near, (dm[..., 0] + 1) + 3 * (dm[..., 1] + 1) + 9 * (dm[..., 2] + 1), 0).astype(np.int64)
    return ok, bit


def _tight_expected(ratio, amag, ddiv):
    """Is twice the documented widening below a tenth of the slack 0.2 ddiv? (module docstring)"""
    widen = 1e-9 * ddiv + 1e-12 * (amag + 1001.0 * ddiv) + 1e-9 * (ratio * ddiv + ddiv)
    return 2.0 * widen < 0.1 * 0.2 * ddiv


@pytest.mark.parametrize("amag", AMAGS)
@pytest.mark.parametrize("ratio", RATIOS)
def test_no_reachable_cell_is_dropped(L, ratio, amag):
    for ddiv in DDIVS:
        rng = np.random.default_rng([int(ratio * 100), int(np.log2(amag + 1)), int(np.log2(ddiv) + 20)])
        mj, c, Rmax, amn = _configs(rng, ratio, amag, ddiv)
        p = _points(rng, mj, c, Rmax, amn, ddiv)
        ok, bit = _passing(p, mj, c, Rmax, amn, ddiv)
        mask = _masks(L, mj, c, Rmax, amn, ddiv).astype(np.int64)
        kept = (mask[:, None] >> bit) & 1
        bad = ok & (kept == 0)
        where = np.argwhere(bad)
        assert not bad.any(), (
            f"ddiv {ddiv}: {bad.sum()} reachable cells dropped; first: mj {mj[where[0][0]]} c {c[where[0][0]]!r} "
            f"Rmax {Rmax[where[0][0]]!r} amn {amn[where[0][0]]!r} p {p[where[0][0], where[0][1]]!r}")
        assert ok.sum() >= 1000, f"ddiv {ddiv}: only {ok.sum()} passing (point, cell) pairs"
        if ratio <= 0.4:
            bits = np.array([bin(int(x)).count("1") for x in mask])
            if _tight_expected(ratio, amag, ddiv):
                assert bits.max() <= 8, f"ddiv {ddiv}: a ball narrower than a cell reaches {bits.max()} cells"
            else:
                assert amag == 2.0 ** 40 and ddiv in (2.0 ** -10, 0.6, 1.1)


def test_nan_geometry_keeps_every_cell(L):
    nan = float("nan")
    mj = np.array([[0, 0, 0], [3, -2, 7], [1, 1, 1], [5, 5, 5]], np.int64)
    c = np.array([[nan, 0.1, 0.1], [nan, nan, nan], [0.5, 0.5, 0.5], [nan, nan, nan]])
    Rmax = np.array([0.01, 0.01, nan, nan])
    amn = np.zeros((4, 3))
    m = _masks(L, mj, c, Rmax, amn, 1.1)
    assert m[1] == ALL and m[2] == ALL and m[3] == ALL
    # one NaN coordinate: that axis cannot cull, the others still may; every cell of the other
    # axes' reach is kept along it
    assert m[0] != 0 and all(((m[0] >> b) & 1) == ((m[0] >> (b - b % 3)) & 1) for b in range(27))


def test_cell_index_is_the_reference_expression(L):
    """cell_index is ceil((p - amn) / ddiv) in double, at exact cell faces and one ulp to either side."""
    rng = np.random.default_rng(5)
    ddiv = rng.choice(DDIVS, 4000)
    amn = rng.choice(AMAGS, 4000) * rng.choice([-1.0, 1.0], 4000)
    m = rng.integers(-5, 1000, 4000).astype(np.float64)
    p = _move(amn + m * ddiv, rng.integers(-2, 3, 4000))
    out = np.zeros(4000, np.int64)
    P = ctypes.c_void_p
    L.cells(ctypes.c_int64(4000), P(p.ctypes.data), P(amn.ctypes.data), P(ddiv.ctypes.data), P(out.ctypes.data))
    assert np.array_equal(out, np.ceil((p - amn) / ddiv).astype(np.int64))
