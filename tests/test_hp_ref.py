"""The oracle (oracle/hakai_oracle.c) and numpy_ref against a 60-digit restatement of the element
update (tests/hp_ref.py), on the existing drop-in inputs (both materials, every active element)
and on the inputs of the GPU edge suite. This pins the oracle a third way, at a few tens of units
of 2^-53 of each Gauss point's / element's OWN scale, and yields the floor the GPU edge suite holds
the fused kernel against (edge_cases.oracle_floor).

Bounds (from the arithmetic, not from the results). An entry of the strain increment is a sum of 24
products B*du; each B entry comes out of ~12 roundings (8-term Jacobian sums, the cofactor inverse,
a 3-term product sum, the B-bar correction), the products and the sum add ~24 more half-units.
Aligned worst case: a few hundred units of the largest term; independent roundings: about
sqrt(24 * 12) * 1/2 ~ 8 to 17 units. ORACLE_BOUND = 64 lies between: four times the statistical
figure, so a healthy code passes with room, and far below what any wrong term (a whole unit of the
FIRST place of a component) would cost. numpy_ref goes through LAPACK solves (pivoted LU, a few times
the roundings of the cofactor form): 4 x 64. eqps is different in kind: the plastic increment is
(q - ys) / (3G + H), a DIFFERENCE of two stresses, so an error of u units in q becomes
u * q / (q - ys) units of the increment, and the increment's share of the stored eqps carries it;
the bound for a Gauss point's eqps is therefore BOUND * (1 + q/(q - ys) * d_eqps/eqps), formed from
the high-precision values."""
import numpy as np
import pytest

import edge_cases as EC
import hp_ref
import oracle as O

ORACLE_BOUND = 64.0
NUMPY_REF_BOUND = 4 * ORACLE_BOUND


def _eqps_excess(c, got, hp, margin, els, bound):
    """max over plastic Gauss points of (error of eqps in units) / (its bound)."""
    worst = 0.0
    for e in els:
        for g in range(8 * e, 8 * e + 8):
            d = abs(got["eqps"][g] - hp["eqps"][g])
            if d == 0:
                continue
            mg = margin[g]
            assert mg > 0 and hp["eqps"][g] > 0, "eqps moved at a Gauss point the reference calls elastic"
            amp = (1 + mg) / mg * (hp["eqps"][g] - c["eq"][g]) / hp["eqps"][g]
            worst = max(worst, d / (2.0 ** -53 * hp["eqps"][g]) / (bound * (1 + amp)))
    return worst


def _hold(c, got, bound, what):
    hp, margin, els = EC.hp_update(c)
    EC.assert_clear_of_yield_surface(margin)
    E = EC.errors(got, hp, els)
    print(what, {k: round(v, 2) for k, v in E.items()})
    for k in ("stress", "strain", "yield", "Qe", "volume"):
        assert E[k] <= bound, f"{what}: {k} off by {E[k]:.1f} units of 2^-53 of its local scale (bound {bound})"
    x = _eqps_excess(c, got, hp, margin, els, bound)
    assert x <= 1.0, f"{what}: eqps at {x:.2f} of its bound"
    # inactive elements: state untouched, no force
    for e in np.flatnonzero(c["flag"] == 0):
        g = slice(8 * e, 8 * e + 8)
        assert np.array_equal(got["stress"][g], c["st"][g]) and np.array_equal(got["eqps"][g], c["eq"][g])
        assert not got["Qe"][e].any()
    return E


@pytest.mark.parametrize("mat", ["ductile", "elastic"])
def test_oracle_and_numpy_ref_on_the_dropin_inputs(mat):
    c = EC.base_case(mat)
    _hold(c, EC.oracle_update(c), ORACLE_BOUND, f"oracle/{mat}")
    _hold(c, EC.numpy_ref_update(c), NUMPY_REF_BOUND, f"numpy_ref/{mat}")
    if mat == "ductile":
        hp, _, _ = EC.hp_update(c)
        assert np.any(hp["eqps"] != c["eq"]) and np.any(hp["eqps"] == c["eq"])   # both branches taken


def test_floor_is_a_few_tens_of_units():
    f = EC.oracle_floor()
    print("floor", f, EC.base_errors("ductile")[0], EC.base_errors("elastic")[0])
    assert 1.0 < f <= 2 * ORACLE_BOUND   # (eqps may use its amplified bound)


def test_pusai_table_against_the_oracle():
    P = hp_ref.pusai()
    with hp_ref.localcontext() as ctx:
        ctx.prec = hp_ref.PREC
        hp = np.array([[[float(P[k][r][i]) for i in range(8)] for r in range(3)] for k in range(8)])
    # every entry is +-(1/8)(1 +- g)(1 +- g): three roundings and that of g in the FP64 table
    assert np.max(np.abs(O.pusai() - hp) / np.abs(hp)) <= 4 * 2.0 ** -53


def test_segment_rule_on_the_breakpoints():
    """eqps exactly on a row of the table belongs to the segment BELOW it (eqps <= plastic[j, 2]); one
    ulp above, to the next. With the yield surface far away the only way to get the wrong segment is
    the wrong rule, and a wrong hardening slope shows in eqps and yield far above rounding."""
    c = EC.breakpoint_case()
    got = EC.oracle_update(c)
    hp, margin, els = EC.hp_update(c)
    assert np.nanmin(margin) > 0.05, "every Gauss point yields, clear of the surface"
    assert np.all(hp["eqps"] > c["eq"])
    _hold(c, got, ORACLE_BOUND, "oracle/breakpoints")
    # the slopes on either side of a row differ, so do the results of the two neighbours of a row
    eq = c["eq"][:32]
    on_row = np.flatnonzero(eq == 0.01)[0]
    above = np.flatnonzero(eq == np.nextafter(0.01, 1))[0]
    d_on, d_above = hp["yield"][on_row] - 400.0, hp["yield"][above] - 400.0
    assert d_on != d_above


@pytest.mark.parametrize("build", [lambda: EC.size_case(9), lambda: EC.size_case(65), EC.mixed_materials_case,
                                   EC.scaling_case, lambda: EC.scaled(EC.scaling_case(), 400),
                                   lambda: EC.scaled(EC.scaling_case(), -400)],
                         ids=["size9", "size65", "mixed_materials", "scaling_base", "scaled_up", "scaled_down"])
def test_oracle_on_well_shaped_edge_inputs(build):
    c = build()
    _hold(c, EC.oracle_update(c), ORACLE_BOUND, "oracle")


@pytest.mark.parametrize("case", [(EC.shape_case, k) for k in EC.SHAPES] + [(EC.rigid_case, k) for k in EC.RIGID],
                         ids=lambda p: p[1])
def test_hard_edge_inputs_are_usable(case):
    """The badly conditioned cases (collapsed corner, 1e6 offset, pure cancellation) have no absolute
    bound -- the GPU suite holds the fused kernel against the ORACLE's error there -- but the oracle's
    error must be finite and no Gauss point may sit on the yield surface."""
    c = case[0](case[1])
    hp, margin, els = EC.hp_update(c)
    EC.assert_clear_of_yield_surface(margin)
    E = EC.errors(EC.oracle_update(c), hp, els)
    print(case[1], {k: float(f"{v:.3g}") for k, v in E.items()})
    assert all(np.isfinite(v) for v in E.values())


def test_scaled_inputs_scale_the_reference_exactly():
    c = EC.scaling_case()
    hp, _, _ = EC.hp_update(c)
    for k in (400, -400):
        hs, _, _ = EC.hp_update(EC.scaled(c, k))
        for name in EC.NAMES:
            assert np.array_equal(hs[name], hp[name] * (np.ldexp(1.0, k) if EC.SCALED_BY[name] else 1.0)), (k, name)


@pytest.mark.parametrize("case", EC.knife_cases(), ids=lambda p: p[0])
def test_knife_edge_deletions_of_the_oracle(case):
    """The deletion counts the GPU suite expects are the oracle's."""
    _, table, szz, eq8, n_del = case
    m = EC.knife_model(table)
    o = O.Oracle(m)
    o.s["integ_stress"][:, 2] = szz
    o.s["integ_eq_plastic_strain"][:] = np.tile(eq8, m.nElement)
    o.run(1, 1)
    assert len(o.deletions) == n_del
    assert not o.s["disp"].any()
