"""HAKAI(fname) on several GPUs: the reference's driver surface (v2/HAKAI_j.jl:81-978, called by
main() with ARGS[1], :3729-3735) with the mesh split over ranks.

    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 \
        -m hakai.run deck.inp out_dir            # one process per GPU, RCCL over xGMI

Every rank reads the deck, computes the global lumped mass (v2/HAKAI_j.jl:183-218) and takes a
contiguous global element range (hakai.dist.range_partition); contact decks pass the global
contact model to every rank, which keeps its own share of it (hakai_set_contact_global). Each step is bit-identical to the
single-GPU run. At the output cadence (floor(time_num/100) steps, :471-480, :932-942) the ranks send
their state to rank 0, which uploads it into an output context holding the whole mesh, takes the
node averages there (cal_node_stress_strain, :3408-3486) and writes out_dir/file%03d.vtk (:3517-3717)
-- the same files, byte for byte, as the one-GPU driver (hakai.hakai / bin/hakai).

Env HAKAI_HISTORY=<stride> also writes out_dir/history.csv, with the one-GPU driver's sets, names
and capacity rule (hakai_inp_history_sets): every rank records the sums over the nodes it owns, the
records travel to rank 0 once at the end of the run, and rank 0 adds them in rank order
(hakai_history_combine). The VTK files are the same bytes with and without.

Env HAKAI_DT_CHECK=1 also writes out_dir/stable_dt.csv, the one-GPU driver's stable-step records
(hakai_stable_dt at state 0 and at every output, the deck's mass_scaling and the stepped d_time):
every rank evaluates its own elements, the records travel to rank 0 once at the end
(gather_stable_dt), and rank 0 combines them (hakai_stable_dt_combine). Unset, nothing changes.

`local_ranks=N` runs the same partition as an in-process group on one device (tests).
"""
from __future__ import annotations

import ctypes
import math
import os
import sys
from dataclasses import replace

import numpy as np

from . import dist as _dist
from ._abi import HISTORY_MAX_SETS, check, lib, ptr
from .model import read_inp
from .solver import (STABLE_DT_KEYS, Solver, State, comm_unique_id, history_combine, stable_dt_combine, step_group,
                     write_history_csv, write_stable_dt_csv)

I64 = ctypes.c_int64


OUT_KEYS = ("disp", "velo", "integ_stress", "integ_strain", "integ_eq_plastic_strain", "integ_triax_stress",
            "element_flag")


def _gather_state(sv: Solver) -> dict:
    st = sv.download(disp=True, velo=True, integ_stress=True, integ_strain=True, integ_eq_plastic_strain=True,
                     integ_triax_stress=True, element_flag=True)
    return {k: getattr(st, k) for k in OUT_KEYS}


def _out_shapes(n_nodes: int, n_elem: int) -> dict:
    """Shapes and dtypes of a rank's output arrays (as Solver.download returns them)."""
    return {"disp": ((3 * n_nodes,), np.float64), "velo": ((3 * n_nodes,), np.float64),
            "integ_stress": ((8 * n_elem, 6), np.float64), "integ_strain": ((8 * n_elem, 6), np.float64),
            "integ_eq_plastic_strain": ((8 * n_elem,), np.float64),
            "integ_triax_stress": ((8 * n_elem,), np.float64), "element_flag": ((n_elem,), np.int64)}


def gather_parts(tdist, group, rank: int, world: int, part: dict, metas: list, device=None):
    """Rank 0 collects every rank's output arrays for one output step: raw point-to-point transfers
    into preallocated buffers, no pickling (gather_object pickled ~1.8 GB per rank per
    output at C5). device=None: host tensors over `group` (gloo); a CUDA device: the arrays travel
    as device tensors over the NCCL (RCCL, xGMI) group. metas[r] = (l2g, e0, n_elem) of rank r
    (exchanged once at setup). Returns [(meta, arrays)] on rank 0, None elsewhere."""
    import torch
    if rank != 0:
        for k in OUT_KEYS:
            t = torch.from_numpy(np.ascontiguousarray(part[k]))
            tdist.send(t if device is None else t.to(device), 0, group=group)
        return None
    out = [(metas[0][:2], part)]
    for r in range(1, world):
        l2g, e0, ne = metas[r]
        arrs = {}
        for k, (shape, dt) in _out_shapes(len(l2g), ne).items():
            if device is None:
                buf = np.empty(shape, dt)
                tdist.recv(torch.from_numpy(buf), r, group=group)
            else:
                t = torch.empty(shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=device)
                tdist.recv(t, r, group=group)
                buf = t.cpu().numpy()
            arrs[k] = buf
        out.append(((l2g, e0), arrs))
    return out


def gather_history(tdist, group, rank: int, world: int, part: dict, device=None):
    """Rank 0 collects every rank's history records (Solver.history() dicts) once, at the end of the
    run: the record count, then steps, values and ke_seed as raw tensors (host tensors over gloo,
    device tensors over the NCCL group, as gather_parts). Returns the dicts in rank order on rank 0,
    None elsewhere."""
    import torch
    keys = ("steps", "values", "ke_seed")

    def send(a):
        t = torch.from_numpy(np.ascontiguousarray(a))
        tdist.send(t if device is None else t.to(device), 0, group=group)

    def recv(r, shape, dt):
        if device is None:
            buf = np.empty(shape, dt)
            tdist.recv(torch.from_numpy(buf), r, group=group)
            return buf
        t = torch.empty(shape, dtype=torch.float64 if dt == np.float64 else torch.int64, device=device)
        tdist.recv(t, r, group=group)
        return t.cpu().numpy()

    if rank != 0:
        send(np.array([len(part["steps"])], np.int64))
        for k in keys:
            send(part[k])
        return None
    out = [{k: part[k] for k in keys}]
    S = part["values"].shape[1]
    for r in range(1, world):
        n = int(recv(r, (1,), np.int64)[0])
        out.append(dict(steps=recv(r, (n,), np.int64), values=recv(r, (n, S, 16), np.float64),
                        ke_seed=recv(r, (S,), np.float64)))
    return out


def _stable_pack(recs: list) -> np.ndarray:
    """Solver.stable_dt() dicts as an (n, 7) int64 array, the doubles as their bits."""
    a = np.zeros((len(recs), len(STABLE_DT_KEYS)), np.int64)
    for i, r in enumerate(recs):
        for j, k in enumerate(STABLE_DT_KEYS):
            a[i, j] = np.float64(r[k]).view(np.int64) if k.startswith("dt_") else int(r[k])
    return a


def _stable_unpack(a: np.ndarray) -> list:
    return [{k: float(np.int64(row[j]).view(np.float64)) if k.startswith("dt_") else int(row[j])
             for j, k in enumerate(STABLE_DT_KEYS)} for row in a]


def gather_stable_dt(tdist, group, rank: int, world: int, recs: list, device=None):
    """Rank 0 collects every rank's stable-step records (a list of Solver.stable_dt() dicts, the same
    number on every rank) once, at the end of the run, as one raw int64 tensor per rank (host
    tensors over gloo, device tensors over the NCCL group, as gather_history). Returns the lists in
    rank order on rank 0, None elsewhere."""
    import torch
    mine = _stable_pack(recs)
    if rank != 0:
        t = torch.from_numpy(mine)
        tdist.send(t if device is None else t.to(device), 0, group=group)
        return None
    out = [recs]
    for r in range(1, world):
        if device is None:
            buf = np.empty(mine.shape, np.int64)
            tdist.recv(torch.from_numpy(buf), r, group=group)
        else:
            t = torch.empty(mine.shape, dtype=torch.int64, device=device)
            tdist.recv(t, r, group=group)
            buf = t.cpu().numpy()
        out.append(_stable_unpack(buf))
    return out


class _Output:
    """Rank 0's output context: the whole mesh, no contact, state uploaded at each output."""

    def __init__(self, glob, gdiag, device, out_dir):
        self.glob = glob
        self.sv = Solver(replace(glob, contact_flag=0, contact_pairs=None), device=device, diag_M=gdiag)
        self.out_dir = out_dir
        os.makedirs(out_dir, exist_ok=True)
        # files are formatted and written on the writer's threads while the ranks step on
        self.writer = None
        w = ctypes.c_void_p()
        check(lib().hakai_vtk_writer_create(ctypes.byref(w), out_dir.encode(), glob.nNode, ptr(glob.coordmat),
                                            glob.nElement, ptr(glob.elementmat, I64), 0))
        self.writer = w

    def write(self, idx, parts):
        g = self.glob
        nN, nE = g.nNode, g.nElement
        disp, velo = np.zeros(3 * nN), np.zeros(3 * nN)
        st = State.empty(nN, nE)
        st.Qe = None
        st.disp_pre = st.velo = st.Q = st.integ_yield_stress = None
        for (l2g, e0), a in parts:
            n = l2g - 1
            disp.reshape(-1, 3)[n] = a["disp"].reshape(-1, 3)  # shared nodes: identical on both ranks
            velo.reshape(-1, 3)[n] = a["velo"].reshape(-1, 3)
            ne = a["element_flag"].shape[0]
            st.integ_stress[8 * e0:8 * (e0 + ne)] = a["integ_stress"]
            st.integ_strain[8 * e0:8 * (e0 + ne)] = a["integ_strain"]
            st.integ_eq_plastic_strain[8 * e0:8 * (e0 + ne)] = a["integ_eq_plastic_strain"]
            st.integ_triax_stress[8 * e0:8 * (e0 + ne)] = a["integ_triax_stress"]
            st.element_flag[e0:e0 + ne] = a["element_flag"]
        st.disp = disp
        self.sv.upload(st)
        avg = self.sv.node_stress_strain()
        check(lib().hakai_vtk_writer_submit(self.writer, idx, ptr(st.element_flag, I64), ptr(disp), ptr(velo),
                                            ptr(avg["node_stress"]), ptr(avg["node_strain"]),
                                            ptr(avg["node_eq_plastic_strain"]), ptr(avg["node_mises_stress"]),
                                            ptr(avg["node_triax_stress"])))

    def close(self):
        if self.writer:
            try:
                check(lib().hakai_vtk_writer_wait(self.writer))
            finally:
                lib().hakai_vtk_writer_destroy(self.writer)
                self.writer = None
        self.sv.close()


def _setup_rank(glob, gdiag, rank, world, device, comm):
    loc, diag, iface, l2g, off = _dist.range_partition(glob, rank, world, gdiag)
    sv = Solver(loc, device=device, diag_M=diag)
    # the driver's element arithmetic is the reference's, operation for operation (as hakai_run_inp)
    sv.set_tuning("elem_exact", 0 if os.environ.get("HAKAI_ELEM_EXACT") == "0" else 1)
    sv.set_element_offset(loc.global_element_offset)
    comm(sv)
    sv.set_interface(*iface)
    if glob.contact_flag >= 1:
        sv.set_contact_global(glob, l2g, off, gdiag)
    return sv, (l2g, int(off[rank]))


def hakai_multi(fname: str, out_dir: str = "temp", local_ranks: int = 0, device: int = 0, verbose: bool = True):
    """HAKAI(fname) over torch.distributed's world (one process per GPU, already initialised with the
    nccl backend), or over `local_ranks` contexts of one process on `device`."""
    if os.environ.get("HAKAI_ELEM_HISTORY"):
        raise ValueError("HAKAI_ELEM_HISTORY is set: the N-GPU driver does not write elem_history.csv yet (the ranks' "
                         "records exist, Solver.elem_history / elem_history_group) -- run the deck on one GPU "
                         "(hakai.hakai / the hakai CLI) or unset the variable")
    glob = read_inp(fname)
    if glob.loads is not None and not glob.loads.empty:
        raise ValueError(f"{fname}: the deck has external loads (*Cload / *Dload / *Dsload); the N-GPU driver does "
                         "not apply loads yet -- run it on one GPU (hakai.hakai / the hakai CLI)")
    if glob.walls is not None and not glob.walls.empty:
        raise ValueError(f"{fname}: the deck has rigid walls (*Rigid Wall); the N-GPU driver does not apply walls "
                         "yet -- run it on one GPU (hakai.hakai / the hakai CLI)")
    if glob.variable_mass_scaling is not None:
        raise ValueError(f"{fname}: the deck has *Variable Mass Scaling; the N-GPU driver does not scale mass yet "
                         "(a shared node needs the neighbour rank's elements) -- run it on one GPU (hakai.hakai / "
                         "the hakai CLI)")
    gdiag, _ = glob.lumped_mass()
    dt = glob.dt
    time_num = glob.end_time / dt
    n_steps = int(math.floor(time_num)) if time_num >= 1 else 0
    d_out = int(math.floor(time_num / 100))
    if local_ranks:
        world, rank, tdist = local_ranks, 0, None
        key = abs(hash((fname, os.getpid()))) % (1 << 40)
        svs, meta = [], []
        for r in range(world):
            sv, mt = _setup_rank(glob, gdiag, r, world, device, lambda s, r=r: s.comm_init_local(r, world, key))
            svs.append(sv)
            meta.append(mt)
    else:
        import torch
        import torch.distributed as tdist
        world, rank = tdist.get_world_size(), tdist.get_rank()
        device = torch.cuda.current_device()
        obj = [comm_unique_id() if rank == 0 else None]
        tdist.broadcast_object_list(obj, src=0)
        sv, mt = _setup_rank(glob, gdiag, rank, world, device, lambda s: s.comm_init(rank, world, obj[0]))
        svs, meta = [sv], [mt]
        # output transfers: raw arrays as device tensors over the world's NCCL (RCCL) group, or host
        # tensors if the world runs gloo; the partition metadata once
        out_group = None
        out_dev = torch.device("cuda", device) if tdist.get_backend() == "nccl" else None
        metas = [None] * world if rank == 0 else None
        tdist.gather_object((mt[0], mt[1], sv.model.nElement), metas, dst=0)
    if verbose and rank == 0:
        print(f"readInpFile:{fname}\nnNode:{glob.nNode}\nnElement:{glob.nElement}\ncontact_flag:{glob.contact_flag}")
        print(f"mass_scaling:{glob.mass_scaling:g}\ntime_num:{time_num:g}\nranks:{world}")
    # HAKAI_HISTORY=<stride>: the one-GPU driver's history output (hakai_run_inp) -- its sets, its
    # names and its capacity rule; every rank records the nodes it owns, rank 0 combines at the end
    hist_stride = int(os.environ.get("HAKAI_HISTORY") or 0)
    hist_names = None
    if hist_stride > 0:
        hist_names, gsets, dropped = glob.history_sets
        if verbose and rank == 0:
            for d in dropped:
                print(f"history: set {d} left out (at most {HISTORY_MAX_SETS} sets)", file=sys.stderr)
        for sv, (l2g, _) in zip(svs, meta):
            sv.history_enable(_dist.local_sets(gsets, l2g), stride=hist_stride, capacity=n_steps // hist_stride + 1)
    out = _Output(glob, gdiag, device, out_dir) if rank == 0 else None
    # HAKAI_DT_CHECK=1: the one-GPU driver's stable-step records (hakai_run_inp) -- at state 0 and at
    # every output each rank evaluates its own elements (global ids: the element offset is set), the
    # records travel to rank 0 once at the end, which combines them and writes out_dir/stable_dt.csv
    dt_check = os.environ.get("HAKAI_DT_CHECK") == "1"
    dt_steps, dt_recs = [], [[] for _ in svs]

    def output(idx):
        if dt_check:
            dt_steps.append(idx * d_out)
            for sv, recs in zip(svs, dt_recs):
                recs.append(sv.stable_dt(dt, glob.mass_scaling))
        parts = [(mt, _gather_state(sv)) for sv, mt in zip(svs, meta)]
        if tdist is not None:
            parts = gather_parts(tdist, out_group, rank, world, parts[0][1], metas, out_dev)
        if out is not None:
            out.write(idx, parts)

    try:
        output(0)
        i_out, t0, reported = 1, 1, 0
        while t0 <= n_steps:
            t1 = n_steps if d_out <= 0 else min(n_steps, ((t0 + d_out - 1) // d_out) * d_out)
            if local_ranks:
                step_group(svs, t0, t1 - t0 + 1, dt)
            else:
                svs[0].step(t0, t1 - t0 + 1, dt)
            if verbose:
                nd = sum(len(sv.deleted()) for sv in svs)
                if tdist is not None:
                    box = [None] * world
                    tdist.all_gather_object(box, nd)
                    nd = sum(box)
                if rank == 0:
                    for q in range(reported, nd):
                        print(f"Element deleted:{glob.nElement - q - 1}/{glob.nElement}")
                    print(f"\r{t1 * dt:.4e} / {glob.end_time:.4e}     ", end="", flush=True)
                reported = nd
            if d_out > 0 and t1 % d_out == 0:
                output(i_out)
                i_out += 1
            t0 = t1 + 1
        for sv in svs:
            sv.sync()
        if hist_stride > 0:  # the ranks' records travel to rank 0 once
            parts = [sv.history() for sv in svs]
            if tdist is not None:
                parts = gather_history(tdist, out_group, rank, world, parts[0], out_dev)
            if rank == 0:
                h = history_combine(parts)
                write_history_csv(os.path.join(out_dir, "history.csv"), hist_names, h["steps"], h["values"], dt)
        if dt_check:
            parts = dt_recs
            if tdist is not None:
                parts = gather_stable_dt(tdist, out_group, rank, world, dt_recs[0], out_dev)
            if rank == 0:
                recs = [stable_dt_combine(list(p)) for p in zip(*parts)]
                write_stable_dt_csv(os.path.join(out_dir, "stable_dt.csv"), dt_steps, recs, dt)
                if verbose:
                    for key, el in (("dt_est", "element_est"), ("dt_safe", "element_safe")):
                        first = next(((s, r) for s, r in zip(dt_steps, recs) if dt > r[key]), None)
                        if first:
                            print(f"stable_dt: step {first[0]}: d_time {dt:.6e} > {key} {first[1][key]:.6e} "
                                  f"(element {first[1][el]})", file=sys.stderr)
        if verbose and rank == 0:
            print()
    finally:
        for sv in svs:
            sv.close()
        if out is not None:
            out.close()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        print("usage: python -m torch.distributed.run --nproc-per-node N -m hakai.run deck.inp [out_dir]")
        return 2
    import torch
    import torch.distributed as tdist
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    device = _dist.rank_device(local_rank, int(os.environ.get("LOCAL_WORLD_SIZE", os.environ.get("WORLD_SIZE", "1"))))
    torch.cuda.set_device(device)
    tdist.init_process_group("nccl", device_id=torch.device("cuda", device))
    try:
        hakai_multi(argv[0], argv[1] if len(argv) > 1 else "temp", verbose=True)
    finally:
        tdist.destroy_process_group()
    return 0


if __name__ == "__main__":
    sys.exit(main())
