"""The oracle's contact (oracle/hakai_oracle_contact.c) against an independent literal Python
restatement (tests/contact_ref.py), on CPU: surface extraction, pair lists, the surface update after
deletions and the contact force bit for bit (Float128 ~ exact rational sum rounded once).
The reference itself cannot run here (no Julia) and ships no contact fixtures: parity of this path
to HAKAI is pinned only by these restatements ("parity unpinned" against the Julia run)."""
import numpy as np
import pytest

from hakai import mesh
import oracle as O
from contact_ref import ContactRef


def _counts_ref(ref):
    return [dict(i_instance=c["i"] + 1, j_instance=c["j"] + 1, n_nodes_i=len(c["nodes_i"]), n_triangles=len(c["tri_e"]),
                 n_nodes_j=len(c["nodes_j"])) for c in ref.ct]


def _ref_force(ref, o):
    return ref.force(o.s["position"].reshape(-1, 3), o.s["velo"], o.diag_M, o.s["element_flag"])


@pytest.mark.parametrize("flag", [1, 2])
def test_pairs_and_sizes(flag):
    m = mesh.two_body_model(plate=(5, 4, 2), impactor=(3, 2, 2), contact_flag=flag, perturb=0.05, seed=2)
    o = O.Oracle(m)
    ref = ContactRef(m)
    assert o.contact_pairs() == _counts_ref(ref)
    assert O.lib().hko_contact_min_size(o.ct) == ref.min_size
    assert O.lib().hko_contact_max_size(o.ct) == ref.max_size
    want = [(1, 2), (2, 1)] if flag == 1 else [(1, 1), (1, 2), (2, 1), (2, 2)]
    assert [(p["i_instance"], p["j_instance"]) for p in o.contact_pairs()] == want


def test_single_instance_gets_self_pair():
    """one instance with *Contact -> a self pair (1,1)."""
    m = mesh.bar_model(2, 2, 3, mesh.steel_ductile(), 0.0)
    m.contact_flag = 1
    o = O.Oracle(m)
    assert [(p["i_instance"], p["j_instance"]) for p in o.contact_pairs()] == [(1, 1)]
    assert o.contact_pairs() == _counts_ref(ContactRef(m))


@pytest.mark.parametrize("myu", [None, 0.0])
def test_contact_force_matches_restatement(myu):
    m = mesh.two_body_model(plate=(6, 6, 2), impactor=(3, 3, 2), v=-1e5, perturb=0.03, seed=4, myu=myu)
    o = O.Oracle(m)
    ref = ContactRef(m)
    total = 0
    for t in range(1, 40):
        o.run(t, 1)
        f, n = o.contact_force()
        fr, nr = _ref_force(ref, o)
        assert n == nr
        assert np.array_equal(f, fr), f"step {t}: max diff {np.max(np.abs(f - fr))}"
        total += n
    assert total > 20, "the impactor must be in contact for several steps"


def test_surface_update_after_deletion():
    """Deleted impactor elements expose neighbour faces: node/triangle lists and forces follow."""
    m = mesh.two_body_model(plate=(6, 6, 1), impactor=(2, 2, 3), v=-3e5, d_time=2e-8, n_steps=400)
    o = O.Oracle(m)
    ref = ContactRef(m)
    seen = 0
    checked = 0
    for t in range(1, 400):
        o.run(t, 1)
        for (_, e) in o.deletions[seen:]:
            ref.element_deleted(int(e))
        seen = len(o.deletions)
        if seen and t % 10 == 0:
            assert o.contact_pairs() == _counts_ref(ref)
            f, n = o.contact_force()
            fr, nr = _ref_force(ref, o)
            assert n == nr and np.array_equal(f, fr)
            checked += n
    assert seen >= 4, "elements must be deleted during contact"
    assert checked > 0


def test_contact_pair_surfaces():
    """*Contact Pair: plate top layer vs impactor bottom layer (v2/readInpFile_j.jl:517-564,
    :1063-1102; surface filter v2/HAKAI_j.jl:2087-2112)."""
    m = mesh.two_body_model(plate=(6, 6, 2), impactor=(3, 3, 2), v=-1e5, perturb=0.03, seed=4, surfaces=True)
    full = O.Oracle(mesh.two_body_model(plate=(6, 6, 2), impactor=(3, 3, 2), perturb=0.03, seed=4))
    o = O.Oracle(m)
    ref = ContactRef(m)
    assert o.contact_pairs() == _counts_ref(ref)
    # the surfaces are subsets of the exterior
    assert all(p["n_triangles"] < q["n_triangles"] for p, q in zip(o.contact_pairs(), full.contact_pairs()))
    total = 0
    for t in range(1, 30):
        o.run(t, 1)
        f, n = o.contact_force()
        fr, nr = _ref_force(ref, o)
        assert n == nr and np.array_equal(f, fr)
        total += n
    assert total > 10


CHARPY = "HAKAI-v0.0.1/input/Charpy-test-v0.0.1.inp"   # below the ref_decks fixture (tests/golden/decks)


def test_reference_charpy_contact_pairs(ref_decks):
    """The reference's *Contact Pair deck: 4 instances, 3 pairs with element surfaces. Oracle pairs,
    surface sizes and forces along the run equal the literal restatement."""
    import hakai
    m = hakai.read_inp(f"{ref_decks}/{CHARPY}")
    assert [(a[0], b[0]) for a, b in m.contact_pairs] == [(2, 1), (2, 3), (2, 4)]
    o = O.Oracle(m)
    ref = ContactRef(m)
    assert o.contact_pairs() == _counts_ref(ref)
    for t in range(1, 200, 40):
        o.run(t, 40)
        f, n = o.contact_force()
        fr, nr = _ref_force(ref, o)
        assert n == nr and np.array_equal(f, fr)


@pytest.mark.parametrize("case", ["deletion", "self", "pair_surfaces", "charpy_deck"])
def test_indexed_oracle_equals_literal(case):
    """The oracle's indexed contact mode (sorted face keys, membership tables, cell index; the
    checker for BASELINE C4 at 4 M hex) reproduces the literal restatement bit for bit: pair lists,
    surface updates after deletions, contact events and the whole trajectory."""
    if case == "deletion":
        m, n = mesh.two_body_model(plate=(6, 6, 1), impactor=(2, 2, 3), v=-3e5, d_time=2e-8, n_steps=400), 400
    elif case == "self":
        m, n = mesh.two_body_model(plate=(6, 6, 2), impactor=(3, 3, 3), v=-1e5, perturb=0.02, seed=1,
                                   contact_flag=2), 300
    elif case == "pair_surfaces":
        m, n = mesh.two_body_model(plate=(6, 6, 2), impactor=(3, 3, 2), v=-1e5, perturb=0.02, seed=1,
                                   surfaces=True), 300
    else:
        import os
        from deck_fixtures import model_from_arrays
        z = np.load(os.path.join(os.path.dirname(__file__), "golden", "deck_Charpy_test.npz"))
        m, n = model_from_arrays(z, "Charpy_test"), 1500
    a, b = O.Oracle(m), O.Oracle(m, contact_indexed=True)
    assert a.contact_pairs() == b.contact_pairs()
    a.run(1, n)
    b.run(1, n)
    assert a.deletions == b.deletions
    for k in ("disp", "disp_pre", "integ_stress", "element_flag"):
        assert np.array_equal(a.s[k], b.s[k]), k
    assert a.contact_pairs() == b.contact_pairs()
    fa, na = a.contact_force()
    fb, nb = b.contact_force()
    assert na == nb and np.array_equal(fa, fb)
    if case == "deletion":
        assert len(a.deletions) >= 4
