"""Inputs of the element-kernel edge suite (tests/test_gpu_element_edges.py) and the CPU side of its
checks -- TEST INFRASTRUCTURE. Everything here runs without a GPU, so tests/test_hp_ref.py can
hold the oracle against the high-precision reference on the very cases the GPU suite uses.

A case is a dict: m (Model), pos (nN, 3), dd (3 nN), st, sn (8 nE, 6), eq, ys (8 nE), flag (nE)."""
import functools

import numpy as np

from hakai import mesh
from hakai.model import Material, Model
import hp_ref
import numpy_ref
import oracle as O
from util import random_state, small_bar

NAMES = hp_ref.NAMES


# ---- running a case on the CPU -----------------------------------------------------------------

def oracle_update(c):
    """cal_stress_hexa of the oracle on a case -> {stress, strain, eqps, yield, Qe, volume}."""
    m = c["m"]
    nE = m.nElement
    out = dict(stress=c["st"].copy(), strain=c["sn"].copy(), eqps=c["eq"].copy(), Qe=np.zeros((nE, 24)),
               volume=np.zeros(nE))
    out["yield"] = c["ys"].copy()
    O.cal_stress_hexa(O.Oracle(m), out["Qe"], out["stress"], out["strain"], out["yield"], out["eqps"],
                      np.ascontiguousarray(c["pos"]), np.ascontiguousarray(c["dd"]), c["flag"], out["volume"])
    return out


def numpy_ref_update(c):
    m, nE = c["m"], c["m"].nElement
    out = dict(stress=c["st"].copy(), strain=c["sn"].copy(), eqps=c["eq"].copy(), Qe=np.zeros((nE, 24)),
               volume=np.zeros(nE))
    out["yield"] = c["ys"].copy()
    dd = c["dd"].reshape(-1, 3)
    for e in np.flatnonzero(c["flag"] == 1):
        n, g = m.elementmat[e] - 1, slice(8 * e, 8 * e + 8)
        r = numpy_ref.element_update(c["pos"][n].T, dd[n].reshape(-1), c["st"][g], c["sn"][g], c["eq"][g], c["ys"][g],
                                     m.materials[m.element_material[e] - 1])
        out["stress"][g], out["strain"][g], out["eqps"][g], out["yield"][g], out["Qe"][e], out["volume"][e] = r
    return out


def hp_update(c):
    """(high-precision outputs, relative yield margins, elements computed) of a case."""
    return hp_ref.update(c["m"], c["pos"], c["dd"], c["st"], c["sn"], c["eq"], c["ys"], c["flag"])


def errors(got, hp, els):
    """{quantity: E} in units of 2^-53 of the local high-precision scale (hp_ref.ulp_error)."""
    return {k: hp_ref.ulp_error(k, got[k], hp[k], els) for k in NAMES}


MARGIN = 2.0 ** -40


def assert_clear_of_yield_surface(margin):
    """No Gauss point within 2^-40 (relative) of the yield surface: there the FP64 codes and the
    high-precision reference may take different branches for a rounding error, and the point would
    have to be excluded. The seeds are chosen so that none is."""
    a = np.abs(margin[~np.isnan(margin)])
    assert a.size == 0 or a.min() > MARGIN, f"a Gauss point sits {a.min():.3e} (relative) from the yield surface"


# ---- the base inputs (the existing drop-in test's) and the floor ---------------------------------

def base_case(mat):
    """tests/test_gpu_exact.py::test_exact_dropin_bitexact's inputs: 4x3x5 bar, seed 11."""
    rng = np.random.default_rng(11)
    material = mesh.steel_ductile() if mat == "ductile" else mesh.steel_elastic()
    m = small_bar(4, 3, 5, material=material, perturb=0.05)
    st, sn, eq, ys = random_state(rng, m.nElement)
    pos = m.coordmat + rng.normal(0, 0.01, size=m.coordmat.shape)
    dd = rng.normal(0, 2e-3, size=3 * m.nNode)
    flag = np.ones(m.nElement, np.int64)
    flag[[2, 7]] = 0
    return dict(m=m, pos=pos, dd=dd, st=st, sn=sn, eq=eq, ys=ys, flag=flag)


@functools.lru_cache(maxsize=None)
def base_errors(mat):
    """({quantity: E_oracle}, {quantity: E_numpy_ref}) on the base inputs, all active elements."""
    c = base_case(mat)
    hp, margin, els = hp_update(c)
    assert_clear_of_yield_surface(margin)
    return errors(oracle_update(c), hp, els), errors(numpy_ref_update(c), hp, els)


@functools.lru_cache(maxsize=None)
def oracle_floor():
    """The largest E_oracle over both materials, all elements and all six quantities of the base
    inputs: what the FP64 reference itself is off by where nothing is hard. An edge case's fused
    error is held against 8 x max(E_oracle of that case, this floor)."""
    return max(max(base_errors(mat)[0].values()) for mat in ("ductile", "elastic"))


# ---- materials -----------------------------------------------------------------------------------

def table_material(name, rows, young=210000., poisson=0.3, ductile=None):
    return Material(name, 7.8e-09, young, poisson, np.array(rows, np.float64).reshape(-1, 2),
                    np.zeros((0, 3)) if ductile is None else np.array(ductile, np.float64).reshape(-1, 3))


def rows_table(n, y0=755.0):
    """An n-row hardening table: strains 0 .. ~1.3, concave, strictly increasing stress."""
    j = np.arange(n, dtype=np.float64)
    eps = 0.01 * j * (1.0 + j / 32.0)
    return np.stack([y0 + 350.0 * (1.0 - np.exp(-3.0 * eps)) + 20.0 * eps, eps], axis=1)


def eleven_materials():
    """Elastic, 2-row, 8-row and 64-row tables and seven more: above the 8 the pipelined kernel
    stages in LDS, so every table is read from global memory."""
    mats = [mesh.steel_elastic(), table_material("two_rows", [[755., 0.], [1100., 4.]]),
            table_material("steel_eight_rows", mesh.STEEL_PLASTIC),   # (no ductile table: nothing is deleted)
            table_material("sixty_four_rows", rows_table(64))]
    for i in range(7):
        mats.append(table_material(f"rows_{3 + 4 * i}", rows_table(3 + 4 * i, 600.0 + 40.0 * i),
                                   young=150000. + 20000. * i, poisson=0.2 + 0.03 * i))
    return mats


def _with(m, **kw):
    d = dict(coordmat=m.coordmat, elementmat=m.elementmat, element_material=m.element_material,
             materials=m.materials, bc=m.bc, ic_dofs=m.ic_dofs, ic_values=m.ic_values, d_time=m.d_time,
             end_time=m.end_time, name=m.name)
    d.update(kw)
    return Model(**d)


def _case(m, seed, pos=None, dd=None, stress=300.0, dd_scale=2e-3, flag=None):
    rng = np.random.default_rng(seed)
    st, sn, eq, ys = random_state(rng, m.nElement, scale=stress)
    pos = m.coordmat.copy() if pos is None else pos
    dd = rng.normal(0, dd_scale, size=3 * m.nNode) if dd is None else dd
    flag = np.ones(m.nElement, np.int64) if flag is None else flag
    return dict(m=m, pos=np.ascontiguousarray(pos), dd=np.ascontiguousarray(dd), st=st, sn=sn, eq=eq, ys=ys,
                flag=flag)


# ---- 1. sizes ------------------------------------------------------------------------------------

SIZES = {1: (1, 1, 1), 7: (1, 1, 7), 8: (2, 2, 2), 9: (1, 3, 3), 31: (1, 1, 31), 32: (2, 4, 4), 33: (1, 3, 11),
         65: (1, 5, 13)}


def size_case(nE, seed=21):
    """nE elements (a wave holds 8, a block 32), flags 0 and 1 mixed inside every wave."""
    m = small_bar(*SIZES[nE], material=mesh.steel_ductile(), perturb=0.05)
    assert m.nElement == nE
    flag = np.ones(nE, np.int64)
    flag[1::3] = 0                      # elements 1, 4, 7 of the first wave, and so on
    c = _case(m, seed + nE, flag=flag)
    c["pos"] = m.coordmat + np.random.default_rng(seed).normal(0, 0.01, size=m.coordmat.shape)
    return c


# ---- 2. mixed materials in one wave ----------------------------------------------------------------

def mixed_materials_case(seed=31):
    base = small_bar(1, 3, 11, material=mesh.steel_ductile(), perturb=0.05)
    mats = eleven_materials()
    m = _with(base, materials=mats, element_material=(np.arange(base.nElement) % len(mats)) + 1)
    c = _case(m, seed, stress=400.0)
    rng = np.random.default_rng(seed + 1)
    # eqps spread over each element's own table, yield stresses on the table's scale
    for e in range(m.nElement):
        pl = np.asarray(mats[m.element_material[e] - 1].plastic).reshape(-1, 2)
        g = slice(8 * e, 8 * e + 8)
        if len(pl):
            c["eq"][g] = rng.uniform(0, 1.2 * pl[-1, 1], 8)
            c["ys"][g] = pl[0, 0] * rng.uniform(0.6, 1.1, 8)
    return c


# ---- 3. hardening breakpoints ---------------------------------------------------------------------

def breakpoint_materials():
    return [mesh.steel_ductile(),
            table_material("perfectly_plastic", [[755., 0.], [755., 1.]]),                        # H = 0
            table_material("softening_segment", [[755., 0.], [800., 0.1], [780., 0.2], [900., 1.]])]  # one H < 0


def breakpoint_case(seed=41):
    """eqps exactly on every row of the element's table, one ulp either side, beyond the last row and
    0, with a stress state that yields at every Gauss point."""
    mats = breakpoint_materials()
    base = small_bar(2, 2, 3, material=mats[0], perturb=0.05)             # 12 elements: 4 per material
    m = _with(base, materials=mats, element_material=np.repeat([1, 2, 3], 4))
    c = _case(m, seed, stress=900.0)
    c["ys"][:] = 400.0
    for mi, mt in enumerate(mats):
        rows = np.asarray(mt.plastic)[:, 1]
        vals = np.concatenate([rows, np.nextafter(rows, -np.inf), np.nextafter(rows, np.inf),
                               [2.0 * rows[-1] + 1.0, 0.0]])
        gps = np.arange(32 * mi, 32 * mi + 32)
        assert len(vals) <= 32
        c["eq"][gps] = np.resize(vals, 32)
    return c


# ---- 4. shapes ------------------------------------------------------------------------------------

SHAPES = ("aspect_100", "sheared", "collapsed_face", "inverted", "offset_1e6")


def _collapse_corner(X, ratio=1e-6):
    """Move node 0 of one element towards its opposite corner until the Jacobian determinant at the
    Gauss point next to it is `ratio` of the mean of the other seven."""
    P = numpy_ref.pusai()
    X = X.copy()
    a, far = X[0].copy(), X[6].copy()

    def dets(t):
        Y = X.copy()
        Y[0] = a + t * (far - a)
        return np.array([np.linalg.det(P[k] @ Y) for k in range(8)]), Y

    lo, hi = 0.0, 1.0                   # det at GP 0 is positive at t = 0 and negative at t = 1
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        d, _ = dets(mid)
        if d[0] > ratio * np.mean(d[1:]):
            lo = mid
        else:
            hi = mid
    d, Y = dets(lo)
    assert 0 < d[0] < 4 * ratio * np.mean(d[1:]) and np.all(d[1:] > 0)
    return Y


def shape_case(kind, seed=51):
    m = small_bar(2, 2, 2, material=mesh.steel_ductile(), perturb=0.05)
    pos = m.coordmat + np.random.default_rng(seed).normal(0, 0.01, size=m.coordmat.shape)
    if kind == "aspect_100":
        pos = pos * np.array([1.0, 1.0, 100.0])
    elif kind == "sheared":
        pos = pos + np.outer(pos[:, 2], [0.7, 0.0, 0.0]) + np.outer(pos[:, 1], [0.3, 0.0, 0.0])
    elif kind == "collapsed_face":
        # a single free-standing element so that moving its corner bends no neighbour
        m = small_bar(1, 1, 1, material=mesh.steel_ductile(), perturb=0.05)
        pos = _collapse_corner(m.coordmat[m.elementmat[0] - 1])
        full = m.coordmat.copy()
        full[m.elementmat[0] - 1] = pos
        pos = full
    elif kind == "inverted":
        em = m.elementmat.copy()
        em[::2] = em[::2][:, [4, 5, 6, 7, 0, 1, 2, 3]]       # every other element left-handed: det < 0
        m = _with(m, elementmat=em)
    elif kind == "offset_1e6":
        pos = pos + 1.0e6
    else:
        raise ValueError(kind)
    return _case(m, seed + 1, pos=pos)


# ---- 5. rigid increments --------------------------------------------------------------------------

RIGID = ("translation", "rotation", "translation_offset_1e6", "rotation_offset_1e6")


def rigid_case(kind, seed=61):
    """d_disp a rigid motion: the strain increment is cancellation only."""
    m = small_bar(2, 2, 2, material=mesh.steel_ductile(), perturb=0.05)
    pos = m.coordmat + np.random.default_rng(seed).normal(0, 0.01, size=m.coordmat.shape)
    if kind.endswith("offset_1e6"):
        pos = pos + 1.0e6
    if kind.startswith("translation"):
        dd = np.tile([1.0e-3, -2.0e-3, 0.5e-3], m.nNode)
    else:
        w = np.array([1.0e-4, -2.0e-4, 1.5e-4])
        dd = np.cross(w, pos - pos.mean(axis=0)).reshape(-1)
    return _case(m, seed + 1, pos=pos, dd=dd)


# ---- 6. unit scaling ------------------------------------------------------------------------------

def scaled(c, k):
    """The case in stress units 2^k times smaller: Young's modulus, the plastic tables' stresses, the
    input stresses and yield stresses times 2^k. Stress, yield stress and Qe of the result scale by
    2^k exactly; strain, eqps and volume do not change."""
    s = np.ldexp(1.0, k)
    m = c["m"]
    mats = [Material(mt.name, mt.density, mt.young * s, mt.poisson,
                     np.asarray(mt.plastic).reshape(-1, 2) * np.array([s, 1.0]), mt.ductile) for mt in m.materials]
    d = dict(c)
    d.update(m=_with(m, materials=mats), st=c["st"] * s, ys=c["ys"] * s)
    return d


SCALED_BY = dict(stress=True, strain=False, eqps=False, Qe=True, volume=False)
SCALED_BY["yield"] = True


def scaling_case(seed=71):
    m = small_bar(1, 3, 3, material=mesh.steel_ductile(), perturb=0.05)
    pos = m.coordmat + np.random.default_rng(seed).normal(0, 0.01, size=m.coordmat.shape)
    return _case(m, seed + 1, pos=pos)


# ---- 7. deletion knife edge -----------------------------------------------------------------------

KNIFE = 0.375
BELOW = 2.0 ** -30

DUCTILE_TABLES = {
    # name: (ductile rows (fracture strain, triaxiality, rate), the fracture strain at triaxiality 1/3)
    "flat_segment": ([[0.375, 0., 30.], [0.375, 1., 30.], [0.875, 2., 30.]], 0.375),
    "single_row": ([[0.375, 0., 30.]], 0.375),
    # the smallest fracture strain on interior rows: du_floor must not skip what the table reaches
    "interior_minimum": ([[0.875, 0., 30.], [0.375, 0.25, 30.], [0.375, 0.5, 30.], [0.875, 2., 30.]], 0.375),
    # triaxiality rows in decreasing order: no bracket ever matches and the last row applies
    "decreasing_rows": ([[0.375, 2., 30.], [0.5, 1., 30.], [0.875, 0., 30.]], 0.875),
}


def knife_cases():
    """(id, table name, sigma_zz, eqps of the 8 Gauss points of every element, elements deleted of 12).
    Dyadic values only: the ordered 8-term average is exact."""
    out = []
    for name, (_, fr) in DUCTILE_TABLES.items():
        out.append((f"{name}-at", name, 300.0, np.full(8, fr), 12))
        out.append((f"{name}-below", name, 300.0, np.full(8, fr - BELOW), 0))
    one = np.zeros(8)
    one[5] = 8 * KNIFE
    out.append(("flat_segment-one_point-at", "flat_segment", 300.0, one.copy(), 12))
    one[5] = 8 * (KNIFE - BELOW)
    out.append(("flat_segment-one_point-below", "flat_segment", 300.0, one.copy(), 0))
    out.append(("flat_segment-compression", "flat_segment", -300.0, np.full(8, 3.0), 0))
    return out


def knife_model(table):
    mat = table_material("knife", [[2000., 0.], [2100., 1.]], ductile=DUCTILE_TABLES[table][0])
    return mesh.bar_model(2, 2, 3, mat, 0.0, perturb=0.0, d_time=1e-7, n_steps=10, name="knife_edge")
