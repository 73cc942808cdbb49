"""Helpers of the N-rank history tests (test_gpu_history_ranks.py): in-process groups with history
on, and the per-rank restatement.

The states of an N-rank group are bit-identical to one context's, so one context without history
(solver B of test_gpu_history.run_b) supplies the per-step global arrays for every rank's check: a
rank's record is the restatement (history_ref) of B's arrays with every set restricted to the nodes
the rank owns, set 0 included. HistoryRef always puts "every node" in front, so the reference sets
of one run are laid out as

    [every node] + for each rank: [the rank's owned nodes] + [each of its sets, owned part]

all in global 1-based ids, and rank r's rows of the result are ref_rows(r, S).
"""
import numpy as np

from hakai import dist
from hakai.solver import Solver, step_group


class Rank:
    """One rank of a group: its solver, local model, interface, local->global node map (1-based) and
    the mask of the local nodes it owns."""

    def __init__(self, sv, loc, iface, l2g, rank):
        self.sv, self.loc, self.iface, self.l2g, self.rank = sv, loc, iface, np.asarray(l2g, np.int64), rank
        self.own = dist.owned_nodes(loc.nNode, iface, rank)


def build_group(glob, world, key, slab=None, tune=None, contact=False):
    """An in-process group of `world` ranks: z-slabs of a structured bar (slab=(nx, ny),
    dist.slab_partition) or contiguous element ranges (dist.range_partition), with the multi-GPU
    contact of `glob` if asked. Tunings go to every rank."""
    gdiag, _ = glob.lumped_mass()
    ranks = []
    for r in range(world):
        if slab:
            loc, diag, iface = dist.slab_partition(glob, r, world, *slab)
            l2g, off = dist.slab_node_global(loc), None
        else:
            loc, diag, iface, l2g, off = dist.range_partition(glob, r, world, gdiag)
        sv = Solver(loc, diag_M=diag)
        sv.set_element_offset(loc.global_element_offset)
        sv.comm_init_local(r, world, key)
        sv.set_interface(*iface)
        if contact:
            sv.set_contact_global(glob, l2g, off, gdiag)
        for k, v in (tune or {}).items():
            sv.set_tuning(k, v)
        ranks.append(Rank(sv, loc, iface, l2g, r))
    return ranks


def close_group(ranks):
    for rk in ranks:
        rk.sv.close()


def enable(ranks, local_sets, stride=1, capacity=1 << 12):
    """history_enable on every rank; local_sets[r] = rank r's sets in local 1-based ids."""
    for rk, sets in zip(ranks, local_sets):
        rk.sv.history_enable(sets, stride=stride, capacity=capacity)


def step(ranks, t_first, n_steps):
    step_group([rk.sv for rk in ranks], t_first, n_steps)


def ref_sets(ranks, local_sets):
    """The reference sets of the module docstring (without the leading "every node", which
    HistoryRef adds): global 1-based ids, every rank's sets restricted to the nodes it owns."""
    out = []
    for rk, sets in zip(ranks, local_sets):
        out.append(rk.l2g[rk.own])
        for s in sets:
            s = np.asarray(s, np.int64).ravel() - 1
            out.append(rk.l2g[s[rk.own[s]]])
    return out


def ref_rows(r, S):
    """Rows of rank r (its S sets, set 0 included) in a reference built from ref_sets."""
    return 1 + r * S + np.arange(S)


def rank_ref(recs, mags, seed, r, S):
    """Rank r's slice of a reference run: (records, magnitudes, (ke_seed, its magnitude))."""
    i = ref_rows(r, S)
    return recs[:, i], mags[:, i], (seed[0][i], seed[1][i])


def numpy_combine(parts):
    """((p_0 + p_1) + p_2) + ... of the ranks' history() dicts, in NumPy: (values, ke_seed)."""
    v, k = parts[0]["values"].copy(), parts[0]["ke_seed"].copy()
    for p in parts[1:]:
        v, k = v + p["values"], k + p["ke_seed"]
    return v, k
