"""History output on N ranks, the host side on the CPU: the mapping of global node sets to a rank's
local ids with the ownership rule (hakai.dist.local_sets, owned_nodes), the deck's history sets as
both drivers take them (Model.history_sets), and the driver's gather of the ranks' records over
gloo (hakai.run.gather_history), world 2 and 3."""
import os
import socket

import numpy as np
import pytest
import torch.distributed as tdist
import torch.multiprocessing as mp

import hakai
from hakai import dist, mesh
from hakai.run import gather_history
from hakai.solver import history_combine
from util import bitwise_equal, fast_deletion_bar, small_bar


def _partitions(kind, world):
    """[(local model, iface, local_node_global)] of a small mesh."""
    if kind == "slab":
        glob = small_bar(3, 2, 9)
        out = []
        for r in range(world):
            loc, _, iface = dist.slab_partition(glob, r, world, 3, 2)
            out.append((loc, iface, dist.slab_node_global(loc)))
        return glob, out
    glob = mesh.two_body_model(plate=(8, 8, 2), impactor=(4, 4, 3), x_slabs=True)
    gdiag, _ = glob.lumped_mass()
    out = []
    for r in range(world):
        loc, _, iface, l2g, _ = dist.range_partition(glob, r, world, gdiag)
        out.append((loc, iface, l2g))
    return glob, out


@pytest.mark.parametrize("kind,world", [("slab", 1), ("slab", 2), ("slab", 4), ("range", 2), ("range", 4)])
def test_owned_local_sets_partition_the_global_sets(kind, world):
    glob, parts = _partitions(kind, world)
    nN = glob.nNode
    rng = np.random.default_rng(7)
    gsets = [np.arange(1, nN + 1), rng.permutation(nN)[:nN // 3] + 1, np.array([1, nN]), np.zeros(0, np.int64)]
    gsets += [l2g[iface[0]] for _, iface, l2g in parts[:1]]  # rank 0's shared nodes: on two ranks each
    counted = [np.zeros(nN, np.int64) for _ in gsets]
    held = [np.zeros(nN, np.int64) for _ in gsets]
    for r, (loc, iface, l2g) in enumerate(parts):
        own = dist.owned_nodes(loc.nNode, iface, r)
        lsets = dist.local_sets(gsets, l2g)
        assert len(lsets) == len(gsets)
        for i, (ls, gs) in enumerate(zip(lsets, gsets)):
            assert ls.dtype == np.int64 and np.all(ls >= 1) and np.all(ls <= loc.nNode)
            assert len(np.unique(ls)) == len(ls)
            back = l2g[ls - 1]
            assert np.all(np.isin(back, gs))                      # nothing outside the global set
            assert np.array_equal(back, gs[np.isin(gs, l2g)])      # every node the rank holds, in set order
            held[i][back - 1] += 1
            counted[i][l2g[ls[own[ls - 1]] - 1] - 1] += 1
    for i, gs in enumerate(gsets):
        want = np.zeros(nN, np.int64)
        want[gs - 1] = 1
        assert np.array_equal(counted[i], want)   # owned by exactly one rank: the owned parts partition the set
        assert np.all(held[i][gs - 1] >= 1) and np.all(held[i] <= 2)
    if world > 1:
        assert np.all(held[4][gsets[4] - 1] == 2)  # a shared node stays in the set on both ranks


def test_owner_is_the_lower_rank():
    _, parts = _partitions("slab", 3)
    for r, (loc, iface, l2g) in enumerate(parts):
        own = dist.owned_nodes(loc.nNode, iface, r)
        ln, lo, hi = iface
        assert not own[ln[hi == r]].any() and own[ln[lo == r]].all()
        assert own.sum() == loc.nNode - np.count_nonzero(hi == r)


def test_deck_history_sets_follow_the_one_gpu_driver(tmp_path):
    """"all", one set per instance, one per *Boundary group, read with the deck (hakai_inp_history_sets,
    the definition hakai_run_inp uses)."""
    from inp_writer import write_inp
    m0 = mesh.two_body_model(plate=(5, 5, 2), impactor=(3, 3, 2), v=-1e5, n_steps=300)
    m = hakai.read_inp(write_inp(str(tmp_path / "impact.inp"), m0))
    names, sets, dropped = m.history_sets
    assert names == ["all", "inst1", "inst2", "bc1"] and dropped == []
    n1 = 6 * 6 * 3
    assert np.array_equal(sets[0], np.arange(1, n1 + 1)) and np.array_equal(sets[1], np.arange(n1 + 1, m.nNode + 1))
    bc_nodes = np.unique((np.concatenate([d for d, _ in m.bc[0].entries]) - 1) // 3 + 1)
    assert np.array_equal(sets[2], bc_nodes)
    assert fast_deletion_bar().history_sets is None  # a model built in code has no deck


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _records(rank, n=23, S=4):
    rng = np.random.default_rng(40 + rank)
    return dict(steps=np.arange(n, dtype=np.int64) * 5, values=rng.standard_normal((n, S, 16)) * 10.0 ** rank,
                ke_seed=rng.standard_normal(S))


def _worker(rank, world, port, ret):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    tdist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for n in (23, 0):  # a run with records, and one too short for any
            parts = gather_history(tdist, None, rank, world, _records(rank, n))
            if rank == 0:
                ok = len(parts) == world
                for r, p in enumerate(parts):
                    want = _records(r, n)
                    ok &= all(p[k].dtype == want[k].dtype and bitwise_equal(p[k], want[k]) for k in want)
                h = history_combine(parts)
                v = parts[0]["values"]
                for p in parts[1:]:
                    v = v + p["values"]
                ret[n] = bool(ok and bitwise_equal(h["values"], v))
            else:
                assert parts is None
    finally:
        tdist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_gather_history_over_gloo(world):
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, _free_port(), ret), nprocs=world, join=True)
    assert ret.get(23) and ret.get(0)
