"""History output on N ranks (in-process groups, hakai_comm_init_local): every rank records the sums
over the nodes it owns, hakai_history_combine adds the ranks' records in rank order.

The states of a group are bit-identical to one context's, so solver B of test_gpu_history.run_b --
one context, no history, one step at a time -- supplies the global arrays, and a rank's record is
checked against the restatement (history_ref) of B's arrays restricted to the rank's owned nodes
(history_ranks.ref_sets), with test_gpu_history.check_records' unchanged bounds: 48 u sum|term| for
the plain fields, its cumulative form for the works. A shared node counted twice, or by nobody, is
off by a whole term. The combined record adds R - 1 roundings per value, each at most u times a
partial sum that sum|term| bounds: (48 + R - 1) u sum|term| against the global restatement.
"""
import functools
import os

import numpy as np
import pytest

import hakai
from hakai import _abi, dist, mesh
from hakai.solver import Solver, history_combine, history_group, read_history_csv
from history_ranks import build_group, close_group, enable, numpy_combine, rank_ref, ref_sets, step
from history_ref import HistoryRef, U, balance, prescribed_mask
from test_gpu_history import check_records, run_b, same_records
from util import bitwise_equal, fast_deletion_bar, small_bar

pytestmark = pytest.mark.gpu


def rank_disp_equal(rk, st_rank, st_global):
    return np.array_equal(st_rank.disp.reshape(-1, 3), st_global.disp.reshape(-1, 3)[rk.l2g - 1])


# ---- 1, 2. small_bar: per-rank records, combined record -------------------------------------------------
@functools.lru_cache(maxsize=None)
def small_bar_case(world, exact):
    m = small_bar()
    nN = m.nNode
    k_if = dist.partition_ranges(6, world)[0][1]  # the layer ranks 0 and 1 share
    gsets = [np.arange(1, nN + 1), mesh.plane_nodes(3, 2, 0), mesh.plane_nodes(3, 2, 6), np.array([17]),
             np.array([nN]), np.zeros(0, np.int64), mesh.plane_nodes(3, 2, k_if)]
    tune = {"elem_exact": exact}
    ranks = build_group(m, world, 515000 + 10 * world + exact, slab=(3, 2), tune=tune)
    lsets = [dist.local_sets(gsets, rk.l2g) for rk in ranks]
    enable(ranks, lsets)
    step(ranks, 1, 60)
    hs = [rk.sv.history() for rk in ranks]
    comb = history_group([rk.sv for rk in ranks])
    finals = [rk.sv.download() for rk in ranks]
    refs = ref_sets(ranks, lsets)
    close_group(ranks)
    recs, mags, seed, fb, _ = run_b(m, 60, refs, tune)
    return dict(ranks=ranks, hs=hs, comb=comb, finals=finals, recs=recs, mags=mags, seed=seed, fb=fb,
                S=len(gsets) + 1)


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_per_rank_records_match_restatement(world, exact):
    c = small_bar_case(world, exact)
    for r, (rk, h) in enumerate(zip(c["ranks"], c["hs"])):
        assert np.array_equal(h["steps"], np.arange(60))
        check_records(h, *rank_ref(c["recs"], c["mags"], c["seed"], r, c["S"]))
        assert rank_disp_equal(rk, c["finals"][r], c["fb"])        # history perturbs nothing
        assert np.all(h["values"][:, 6, :] == 0.0)                 # the empty set
        assert bitwise_equal(h["values"][:, 0, :], h["values"][:, 1, :])  # set 0 = the set of all nodes
    # the shared layer (set 7) is rank 0's: rank 1 holds its nodes and counts none of them
    assert np.any(c["hs"][0]["U"][:, 7, 2] != 0.0) and np.all(c["hs"][1]["values"][:, 7, :] == 0.0)
    assert np.any(c["hs"][0]["F_int"][:, 2, 2] != 0.0)             # the clamped plane's reaction, rank 0 only
    assert all(np.all(h["values"][:, 2, :] == 0.0) for h in c["hs"][1:])


@pytest.mark.parametrize("exact", [0, 1])
@pytest.mark.parametrize("world", [2, 3])
def test_combined_record(world, exact):
    c = small_bar_case(world, exact)
    v, k = numpy_combine(c["hs"])
    assert np.array_equal(c["comb"]["steps"], np.arange(60))
    assert bitwise_equal(c["comb"]["values"], v) and bitwise_equal(c["comb"]["ke_seed"], k)
    got, ref, mag = c["comb"]["values"][:, 0, :], c["recs"][:, 0, :], c["mags"][:, 0, :]
    for f in (0, 1, 2, 6, 7, 8, 13, 14, 15):  # F_int, P, U of set 0 against the global restatement
        assert np.all(np.abs(got[:, f] - ref[:, f]) <= (48 + world - 1) * U * mag[:, f]), f
    assert np.any(got[:, 13:16] != 0.0)


# ---- 3. reduction edges on ranks ------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(3, 3, 128), (3, 3, 257)])
def test_reduction_edges_on_ranks(shape):
    """Two ranks of 1040 nodes each (five chunks, one group), then of 2080 and 2064 (two groups).
    The upper rank's first 16 local nodes are the layer it shares with rank 0: not owned. Both
    launch forms, with and without owner-computed assembly: the same bits."""
    m = small_bar(*shape)
    got = []
    for form, own in ((0, 0), (1, 0), (0, 1), (1, 1)):
        tune = {"elem_pipe_min": 0, "elem_pipe_blocks": 6, "own_assembly": own, "history_one_block": form}
        ranks = build_group(m, 2, 525000 + 100 * shape[2] + 2 * form + own, slab=(3, 3), tune=tune)
        lsets = []
        for rk in ranks:
            nl = rk.loc.nNode
            one_wave = np.arange(66, 72)  # lanes of one wave only
            per_chunk = np.array([min(c * 256 + (37 * c) % 256 + 1, nl) for c in range((nl + 255) // 256)])
            # rank 1: nodes of the shared layer only (not owned: zeros); rank 0: its side of that layer
            edge = np.arange(1, 6) if rk.rank == 1 else np.arange(nl - 15, nl + 1)
            lsets.append([one_wave, per_chunk, edge])
        assert not ranks[1].own[:16].any() and ranks[1].own[16:].all() and ranks[0].own.all()
        enable(ranks, lsets)
        step(ranks, 1, 3)
        got.append([rk.sv.history() for rk in ranks])
        own_steps = [rk.sv.stat("own_steps") for rk in ranks]
        assert all(n == (3 if own else 0) for n in own_steps), own_steps
        refs = ref_sets(ranks, lsets)
        close_group(ranks)
    recs, mags, seed, _, _ = run_b(m, 3, refs)
    for hs in got:
        for r, h in enumerate(hs):
            check_records(h, *rank_ref(recs, mags, seed, r, 4))
            same_records(h, got[0][r])
    assert np.all(got[0][1]["values"][:, 3, :] == 0.0) and np.any(got[0][0]["values"][:, 3, :] != 0.0)
    assert np.any(got[0][1]["F_int"][:, 0, :] != 0.0)


# ---- 4. one rank with a communicator ----------------------------------------------------------------------
def test_one_rank_with_a_communicator_equals_no_communicator():
    m = small_bar()
    sets = [mesh.plane_nodes(3, 2, 0), mesh.plane_nodes(3, 2, 6), np.array([17])]
    hs = []
    for comm in (False, True):
        with Solver(m) as sv:
            if comm:
                sv.comm_init_local(0, 1, 535001)
                sv.set_interface(np.zeros(0, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32))
            sv.history_enable(sets)
            sv.step(1, 40)
            hs.append(sv.history())
    assert np.array_equal(hs[0]["steps"], np.arange(40))
    same_records(hs[0], hs[1])
    same_records(history_combine([hs[1]]), hs[1])  # one part: the identity


# ---- 5. contact, x-slab numbering ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def contact_model():
    return mesh.two_body_model(plate=(8, 8, 2), impactor=(4, 4, 3), v=-3e5, d_time=2e-8, n_steps=400, x_slabs=True)


@pytest.mark.parametrize("world", [2, 4])
def test_contact_x_slabs(world):
    """Range partitions of the x-slab numbering: every rank holds part of both bodies and the shared
    nodes are scattered through its local numbering."""
    m = contact_model()
    n1, n = 9 * 9 * 3, 40
    gsets = [np.arange(1, n1 + 1), np.arange(n1 + 1, m.nNode + 1), mesh.plane_nodes(8, 8, 0)]
    ranks = build_group(m, world, 545000 + world, contact=True)
    shared = np.flatnonzero(~ranks[1].own)
    assert len(shared) > 1 and np.any(np.diff(shared) > 1)  # not one leading block of local ids
    lsets = [dist.local_sets(gsets, rk.l2g) for rk in ranks]
    enable(ranks, lsets)
    step(ranks, 1, n)
    hs = [rk.sv.history() for rk in ranks]
    comb = history_group([rk.sv for rk in ranks])
    refs = ref_sets(ranks, lsets) + gsets  # the global body sets last
    close_group(ranks)
    recs, mags, seed, _, _ = run_b(m, n, refs)
    for r, h in enumerate(hs):
        check_records(h, *rank_ref(recs, mags, seed, r, 4))  # F_ext and W_ext among the fields
    late = comb["steps"] >= 30  # the 0.1 mm gap closes near step 17
    assert np.all(comb["F_ext"][:5] == 0.0) and np.all(comb["W_ext"][:5] == 0.0)
    assert np.all(comb["W_ext"][late][:, 0] != 0.0) and np.all(comb["W_ext"][late][:, 2] != 0.0)
    for s in (1, 2):
        assert np.any(comb["F_ext"][late][:, s, :] != 0.0)
    g = 1 + world * 4  # rows of the global body sets in the reference
    tot, parts = comb["F_ext"][:, 0, :], comb["F_ext"][:, 1, :] + comb["F_ext"][:, 2, :]
    bound = 48 * U * (mags[:, 0, 3:6] + mags[:, g, 3:6] + mags[:, g + 1, 3:6]) + \
        U * (np.abs(comb["F_ext"][:, 1, :]) + np.abs(comb["F_ext"][:, 2, :]))
    assert np.all(np.abs(tot - parts) <= bound)


# ---- 6. deletion, amplitude BC, balance ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def deletion_bar_b():
    m = fast_deletion_bar()
    with Solver(m) as sv:  # B: one context, no history
        sv.step(1, 3000)
        return sv.download(), sv.deleted()


@pytest.mark.parametrize("world", [2, 3])
def test_deletion_bar_balance_on_ranks(world):
    m = fast_deletion_bar()
    fb, db = deletion_bar_b()
    ranks = build_group(m, world, 555000 + world, slab=(2, 2))
    enable(ranks, [[] for _ in ranks], stride=50, capacity=64)
    step(ranks, 1, 3000)
    comb = history_group([rk.sv for rk in ranks])
    dels = np.array(sorted(tuple(x) for rk in ranks for x in rk.sv.deleted()))
    for rk in ranks:
        assert rk.sv.history_count() == (60, 60)
        assert rank_disp_equal(rk, rk.sv.download(), fb)
    close_group(ranks)
    assert len(db) == 4 and np.array_equal(dels, db)
    assert np.array_equal(comb["steps"], np.arange(0, 3000, 50))
    res = [balance(v[0], comb["ke_seed"][0]) for v in comb["values"]]
    worst = max(abs(r) for r, _ in res) / max(big for _, big in res)
    print(f"deletion bar on {world} ranks: worst balance residual of the combined records {worst:.3e} of the "
          "largest energy term")
    assert worst <= 64 * 1.3e-14  # the bound test_deletion_bar_balance takes from the CPU oracle for this model
    assert comb["W_bc"][-1, 0] != 0.0 and comb["W_int"][-1, 0] > 0.0


# ---- 7. exchange overflow and retry -------------------------------------------------------------------------
def overflow_model():
    return mesh.two_body_model(plate=(16, 16, 8), impactor=(4, 4, 4), v=-3e5, d_time=2e-8, n_steps=300)


def overflow_run(key, tune, chunk):
    m = overflow_model()
    n1 = 17 * 17 * 9
    gsets = [np.arange(1, n1 + 1), np.arange(n1 + 1, m.nNode + 1)]
    ranks = build_group(m, 2, key, tune=tune, contact=True)
    enable(ranks, [dist.local_sets(gsets, rk.l2g) for rk in ranks], capacity=512)
    for t in range(1, m.n_steps + 1, chunk):
        step(ranks, t, min(chunk, m.n_steps + 1 - t))
    hs = [rk.sv.history() for rk in ranks]
    retries = min(rk.sv.stat("exchange_retries") for rk in ranks)
    close_group(ranks)
    return hs, retries


@functools.lru_cache(maxsize=None)
def overflow_default():
    return overflow_run(565000, None, 300)


@pytest.mark.parametrize("caps", [1, 3])
def test_exchange_overflow_retry_leaves_one_record_per_step(caps):
    """The model and tunings of test_contact_group_exchange_capacities_grow: steps that overflow an
    exchange block are poisoned on every rank and run again. Nothing of a poisoned attempt survives
    in the records: they equal the undisturbed run's bit for bit, one per step."""
    base, _ = overflow_default()
    tune = {"contact_exchange_deletions": caps, "contact_exchange_bins": caps, "contact_exchange_events": caps}
    hs, retries = overflow_run(565010 + caps, tune, 300)
    assert retries >= 1
    for h, h0 in zip(hs, base):
        assert np.array_equal(h["steps"], np.arange(300))
        same_records(h, h0)
    assert np.any(base[0]["W_ext"][-1] != 0.0) or np.any(base[1]["W_ext"][-1] != 0.0)


def test_deletion_exchange_overflow_retry_in_one_call():
    """contact_exchange_deletions = 1, the whole run in one call: the even-step parity case of
    test_contact_group_deletion_exchange_overflow_retry_bitexact."""
    base, _ = overflow_default()
    hs, retries = overflow_run(565020, {"contact_exchange_deletions": 1}, 300)
    assert retries >= 1
    for h, h0 in zip(hs, base):
        assert np.array_equal(h["steps"], np.arange(300))
        same_records(h, h0)


# ---- 8. restart on ranks ---------------------------------------------------------------------------------
def test_restart_on_ranks():
    """Every rank's state downloaded and uploaded back after 20 steps (collective): the count returns
    to 0, KE_seed comes from the uploaded displacements, and the first step takes Q from the uploaded
    buffer at interface nodes too (no interface fix runs in it). A rank's downloaded Q is its local
    sum; an upload wants the assembled one, which B (bit-identical states) supplies."""
    m = small_bar()
    gsets = [mesh.plane_nodes(3, 2, 0), mesh.plane_nodes(3, 2, 3), mesh.plane_nodes(3, 2, 6)]
    with Solver(m) as b:
        b.step(1, 20)
        sb = b.download()
        b.upload(sb)
        ranks = build_group(m, 2, 575001, slab=(3, 2))
        lsets = [dist.local_sets(gsets, rk.l2g) for rk in ranks]
        enable(ranks, lsets)
        step(ranks, 1, 20)
        assert all(rk.sv.history_count() == (20, 20) for rk in ranks)
        for rk in ranks:
            st = rk.sv.download()
            assert rank_disp_equal(rk, st, sb)
            st.Q = np.ascontiguousarray(sb.Q.reshape(-1, 3)[rk.l2g - 1].ravel())
            rk.sv.upload(st)
        assert all(rk.sv.history_count() == (0, 0) for rk in ranks)
        step(ranks, 21, 10)
        hs = [rk.sv.history() for rk in ranks]
        close_group(ranks)
        # B from the same state, as run_b steps it
        ref = HistoryRef(b.diag_M, prescribed_mask(m), ref_sets(ranks, lsets), m.dt)
        st = b.download(disp=True, disp_pre=True, Q=True)
        seed = ref.seed(st.disp, st.disp_pre)
        recs, mags = [], []
        for t in range(21, 31):
            b.step(t, 1)
            nx = b.download(disp=True, disp_pre=True, Q=True)
            v, g = ref.step(nx.disp, st.disp, st.Q)
            recs.append(v)
            mags.append(g)
            st = nx
    recs, mags = np.array(recs), np.array(mags)
    for r, h in enumerate(hs):
        assert np.array_equal(h["steps"], np.arange(20, 30))
        check_records(h, *rank_ref(recs, mags, seed, r, 4), k0=20)  # ke_seed within 48 u sum|term| too
        assert np.all(h["ke_seed"][0] > 0)


# ---- 9. refusals -------------------------------------------------------------------------------------------
def test_refusals_on_ranks():
    m = small_bar()
    loc, diag, iface = dist.slab_partition(m, 0, 2, 3, 2)
    with Solver(loc, diag_M=diag) as sv:
        sv.comm_init_local(0, 2, 585001)
        with pytest.raises(hakai.HakaiError) as ei:  # ownership comes from the interface
            sv.history_enable([])
        assert ei.value.code == _abi.HAKAI_ERR_STATE
        sv.set_interface(*iface)
        sv.history_enable([np.array([1, 2])], stride=2, capacity=8)
        with pytest.raises(hakai.HakaiError) as ei:
            sv.set_interface(*iface)
        assert ei.value.code == _abi.HAKAI_ERR_STATE
        with pytest.raises(hakai.HakaiError) as ei:
            sv.history_enable([np.array([loc.nNode + 1])])  # local ids
        assert ei.value.code == _abi.HAKAI_ERR_ARG
        assert sv.history_count() == (0, 0)
        sv.history_disable()
        sv.set_interface(*iface)
    a = dict(steps=np.array([0, 2]), values=np.ones((2, 1, 16)), ke_seed=np.ones(1))
    b = dict(steps=np.array([0, 3]), values=np.ones((2, 1, 16)), ke_seed=np.ones(1))
    with pytest.raises(hakai.HakaiError) as ei:
        history_combine([a, b])
    assert ei.value.code == _abi.HAKAI_ERR_STATE


# ---- 10. driver ----------------------------------------------------------------------------------------------
def test_multi_driver_writes_history_csv(tmp_path, monkeypatch):
    from hakai.run import hakai_multi
    from inp_writer import write_inp
    m0 = mesh.two_body_model(plate=(5, 5, 2), impactor=(3, 3, 2), v=-1e5, n_steps=300)
    deck = write_inp(str(tmp_path / "impact.inp"), m0)
    monkeypatch.delenv("HAKAI_HISTORY", raising=False)
    hakai_multi(deck, str(tmp_path / "plain"), local_ranks=2, verbose=False)
    assert not os.path.exists(tmp_path / "plain" / "history.csv")
    monkeypatch.setenv("HAKAI_HISTORY", "5")
    hakai_multi(deck, str(tmp_path / "hist"), local_ranks=2, verbose=False)
    hakai.hakai(deck, str(tmp_path / "one"), verbose=False)
    monkeypatch.delenv("HAKAI_HISTORY")
    files = sorted(os.listdir(tmp_path / "plain"))
    assert len(files) == 101 and sorted(os.listdir(tmp_path / "hist")) == files + ["history.csv"]
    for f in files:
        assert (tmp_path / "plain" / f).read_bytes() == (tmp_path / "hist" / f).read_bytes(), f
    csv, one = (read_history_csv(str(tmp_path / d / "history.csv")) for d in ("hist", "one"))
    assert csv["sets"] == one["sets"] == ["all", "inst1", "inst2", "bc1"]
    assert np.array_equal(csv["steps"], one["steps"]) and len(csv["steps"]) == 60
    assert np.array_equal(csv["time"], one["time"])
    # a hand-built group of the same partition, the driver's element arithmetic
    m = hakai.read_inp(deck)
    names, gsets, dropped = m.history_sets
    assert names == csv["sets"] and not dropped
    ranks = build_group(m, 2, 595001, tune={"elem_exact": 1}, contact=True)
    enable(ranks, [dist.local_sets(gsets, rk.l2g) for rk in ranks], stride=5, capacity=m.n_steps // 5 + 1)
    step(ranks, 1, m.n_steps)
    h = history_group([rk.sv for rk in ranks])
    close_group(ranks)
    assert np.array_equal(csv["steps"], h["steps"]) and bitwise_equal(csv["values"], h["values"])
    assert np.any(h["F_ext"] != 0.0) and h["W_ext"][-1, 0] != 0.0  # the bodies met during the run
