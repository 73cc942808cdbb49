"""Host-side mirror of HAKAI's solver interface over the MI355X C ABI.

* ``Solver``             -- the persistent device context: hakai()'s state (v2/HAKAI_j.jl:81-480)
                            and its time loop (:487-951) as ``step(t_first, n)``.
* ``cal_stress_hexa``    -- same name, arguments and in-place semantics as the reference
                            (v2/HAKAI_j.jl:1033), executed by the gfx950 element kernel.
* ``cal_triax_stress``   -- v2/HAKAI_j.jl:982.
* ``hakai``              -- HAKAI(fname): .inp -> out_dir/file%03d.vtk (v2/HAKAI_j.jl:81).
Every call goes to libhakai_hip.so; there is no Python or CPU compute path.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass

import numpy as np

from ._abi import MassScaleT, StableDtT, StateT, check, lib, ptr
from .model import Loads, Model, Walls

I64 = ctypes.c_int64


@dataclass
class State:
    """Reference-layout state arrays (v2/HAKAI_j.jl:225-230, :430-456)."""
    disp: np.ndarray
    disp_pre: np.ndarray
    velo: np.ndarray
    Q: np.ndarray
    integ_stress: np.ndarray            # (8nE, 6)  == Julia 6 x 8nE
    integ_strain: np.ndarray
    integ_yield_stress: np.ndarray      # (8nE,)
    integ_eq_plastic_strain: np.ndarray
    integ_triax_stress: np.ndarray
    element_flag: np.ndarray            # (nE,) int64
    Qe: np.ndarray | None = None        # (nE, 24) element internal forces of the last step

    @staticmethod
    def empty(nN: int, nE: int) -> "State":
        f = lambda *s: np.zeros(s)  # noqa: E731
        return State(f(3 * nN), f(3 * nN), f(3 * nN), f(3 * nN), f(8 * nE, 6), f(8 * nE, 6), f(8 * nE),
                     f(8 * nE), f(8 * nE), np.ones(nE, np.int64), f(nE, 24))

    def c(self) -> StateT:
        s = StateT()
        for name, _ in StateT._fields_:
            a = getattr(self, name)
            if a is not None:
                setattr(s, name, ptr(a, ctypes.c_int64 if a.dtype == np.int64 else ctypes.c_double))
        return s


class Solver:
    """Persistent device context holding one (rank-local) model."""

    def __init__(self, model: Model, device: int = 0, diag_M: np.ndarray | None = None):
        self.L = lib()
        self.model = model
        self.ctx = ctypes.c_void_p()
        check(self.L.hakai_create(ctypes.byref(self.ctx), device))
        if diag_M is None:
            diag_M, _ = model.lumped_mass()
        self.diag_M = np.ascontiguousarray(diag_M, dtype=np.float64)
        mats, keep = model.c_materials()
        check(self.L.hakai_upload_model(self.ctx, model.nNode, ptr(model.coordmat), model.nElement,
                                        ptr(model.elementmat, I64), ptr(model.element_material, I64),
                                        len(model.materials), mats, ptr(self.diag_M)))
        del keep
        bc, keep = model.c_bc()
        check(self.L.hakai_set_bc(self.ctx, ctypes.byref(bc)))
        del keep
        if getattr(model, "contact_flag", 0) >= 1:
            inst = model.element_instance
            inst = np.ones(model.nElement, np.int64) if inst is None else np.ascontiguousarray(inst, np.int64)
            ncp, cpi, cpo, cpe = model.c_contact_pairs()
            check(self.L.hakai_set_contact_cp(self.ctx, int(model.contact_flag), ptr(inst, I64), ncp,
                                              ptr(cpi, ctypes.c_int32), ptr(cpo, I64), ptr(cpe, I64)))
            if getattr(model, "contact_params", None) is not None:
                check(self.L.hakai_set_contact_params(self.ctx, *[float(x) for x in model.contact_params]))
        if getattr(model, "loads", None) is not None and not model.loads.empty:
            self.set_loads(model.loads)
        if getattr(model, "walls", None) is not None and not model.walls.empty:
            self.set_walls(model.walls)
        self.reset()

    # -- lifecycle ---------------------------------------------------------------------------
    def close(self):
        if self.ctx:
            self.L.hakai_destroy(self.ctx)
            self.ctx = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- state ---------------------------------------------------------------------------------
    def reset(self):
        """Fresh state with the model's initial velocity (v2/HAKAI_j.jl:225-239, :430-465)."""
        m = self.model
        check(self.L.hakai_reset_state(self.ctx, len(m.ic_dofs), ptr(m.ic_dofs, I64), ptr(m.ic_values), m.dt))

    def upload(self, st: State):
        s = st.c()
        check(self.L.hakai_upload_state(self.ctx, ctypes.byref(s)))

    def download(self, st: State | None = None, **only) -> State:
        """Copy the device state back in the reference layout. only=dict(name=True) limits arrays."""
        m = self.model
        if st is None:
            st = State.empty(m.nNode, m.nElement)
        s = st.c()
        if only:
            for name, _ in StateT._fields_:
                if not only.get(name, False):
                    setattr(s, name, None)
        check(self.L.hakai_download_state(self.ctx, ctypes.byref(s)))
        return st

    # -- time loop -------------------------------------------------------------------------------
    def step(self, t_first: float, n_steps: int, d_time: float | None = None):
        check(self.L.hakai_step(self.ctx, float(t_first), int(n_steps),
                                float(self.model.dt if d_time is None else d_time)))

    def sync(self):
        check(self.L.hakai_sync(self.ctx))

    def deleted(self, cap: int = 1 << 16) -> np.ndarray:
        """(step, element 1-based) pairs of the deletions so far, in (step, element) order."""
        n = I64(0)
        log = np.zeros(2 * cap, np.int64)
        check(self.L.hakai_deleted(self.ctx, ctypes.byref(n), ptr(log, I64), cap))
        k = min(n.value, cap)
        return log[:2 * k].reshape(k, 2)

    def negative_jacobians(self) -> int:
        n = I64(0)
        check(self.L.hakai_negative_jacobians(self.ctx, ctypes.byref(n)))
        return n.value

    def node_stress_strain(self):
        nN = self.model.nNode
        ns, nn = np.zeros((nN, 6)), np.zeros((nN, 6))
        ne, nm, nt = np.zeros(nN), np.zeros(nN), np.zeros(nN)
        check(self.L.hakai_node_stress_strain(self.ctx, ptr(ns), ptr(nn), ptr(ne), ptr(nm), ptr(nt)))
        return dict(node_stress=ns, node_strain=nn, node_eq_plastic_strain=ne, node_mises_stress=nm,
                    node_triax_stress=nt)

    # -- contact ----------------------------------------------------------------------------------
    def contact_stats(self) -> dict:
        """Counters of the last contact step (hakai_contact_stats)."""
        st = np.zeros(12, np.int64)
        check(self.L.hakai_contact_stats(self.ctx, ptr(st, I64), 12))
        keys = ("events", "max_events", "candidate_triangles", "touched_nodes", "live_triangles", "live_nodes_i",
                "live_nodes_j", "binned_contact_nodes", "exchange_bytes_per_rank", "hash_buckets",
                "tested_triangles", "exchange_record_bytes_per_rank")
        return {k: int(v) for k, v in zip(keys, st)}

    def contact_info(self):
        """Pairs [(i_instance, j_instance, n_nodes_i, n_triangles, n_nodes_j)], (min, max) element size."""
        n = ctypes.c_int32(0)
        info = np.zeros(5 * 4096, np.int64)
        sizes = np.zeros(2)
        check(self.L.hakai_contact_info(self.ctx, ctypes.byref(n), ptr(info, I64), 4096, ptr(sizes)))
        return [tuple(int(x) for x in info[5 * p:5 * p + 5]) for p in range(n.value)], tuple(sizes)

    def contact_force(self, t: float, d_time: float | None = None) -> np.ndarray:
        """cal_contact_force at the current device state (external_force of step t), 3nN."""
        f = np.zeros(3 * self.model.nNode)
        check(self.L.hakai_contact_force(self.ctx, float(t), float(self.model.dt if d_time is None else d_time),
                                         ptr(f)))
        return f

    # -- external loads -----------------------------------------------------------------------------
    def set_loads(self, loads: Loads):
        """Replace the external loads (hakai_set_loads): concentrated forces, gravity, follower face
        pressure, each with an optional amplitude table. Captured step graphs are dropped and an
        enabled history restarts. A refused call leaves the previous loads in force."""
        s, keep = loads.c()
        check(self.L.hakai_set_loads(self.ctx, ctypes.byref(s)))
        del keep

    def clear_loads(self):
        check(self.L.hakai_clear_loads(self.ctx))

    def load_force(self, t: float, d_time: float | None = None) -> np.ndarray:
        """The load force of step t at the current device state, without contact (3nN; no step)."""
        f = np.zeros(3 * self.model.nNode)
        check(self.L.hakai_load_force(self.ctx, float(t), float(self.model.dt if d_time is None else d_time), ptr(f)))
        return f

    # -- rigid walls ----------------------------------------------------------------------------------
    def set_walls(self, walls: Walls):
        """Replace the rigid walls (hakai_set_walls): moving planes with penalty, damping and Coulomb
        friction. Captured step graphs are dropped and an enabled history restarts; the loads stay
        in force. A refused call leaves the previous walls in force."""
        s, keep = walls.c()
        check(self.L.hakai_set_walls(self.ctx, ctypes.byref(s)))
        del keep

    def clear_walls(self):
        check(self.L.hakai_clear_walls(self.ctx))

    def wall_force(self, t: float, d_time: float | None = None) -> np.ndarray:
        """The wall force of step t at the current device state, without contact and loads (3nN; no step)."""
        f = np.zeros(3 * self.model.nNode)
        check(self.L.hakai_wall_force(self.ctx, float(t), float(self.model.dt if d_time is None else d_time), ptr(f)))
        return f

    # -- profiling (HIP events on the context's own stream) ------------------------------------
    def profile(self, on: bool = True, kernels=None):
        """Time kernels with HIP events on the context's stream (all, or the HAKAI_K_* ids given)."""
        if kernels is None:
            check(self.L.hakai_profile_enable(self.ctx, int(on)))
        else:
            check(self.L.hakai_profile_mask(self.ctx, sum(1 << k for k in kernels) if on else 0))

    def profile_read(self, kernel: int) -> tuple[float, int]:
        ms, n = ctypes.c_double(0), I64(0)
        check(self.L.hakai_profile_read(self.ctx, kernel, ctypes.byref(ms), ctypes.byref(n)))
        return ms.value, n.value

    def set_tuning(self, key: str, value: int):
        check(self.L.hakai_set_tuning(self.ctx, key.encode(), int(value)))

    def stat(self, key: str) -> int:
        """Step-loop counter (hakai_stat): graph_steps, own_steps, own_rows, own_entries, own_superbatch, own_slots,
        conn_patterns (0: the element kernel reads the plain connectivity array), conn_bytes, device_buffers (device
        arrays the library holds now, over every context of the process)."""
        n = I64(0)
        check(self.L.hakai_stat(self.ctx, key.encode(), ctypes.byref(n)))
        return n.value

    def graph_steps(self) -> int:
        """Steps run from captured hipGraphs so far (hakai_graph_steps)."""
        n = I64(0)
        check(self.L.hakai_graph_steps(self.ctx, ctypes.byref(n)))
        return n.value

    # -- history output --------------------------------------------------------------------------
    @staticmethod
    def _record_sets(sets):
        """(n, off, ids): a list of 1-based id arrays in the form the C entry points take."""
        sets = [np.ascontiguousarray(s, np.int64).ravel() for s in sets]
        off = np.zeros(len(sets) + 1, np.int64)
        off[1:] = np.cumsum([len(s) for s in sets])
        ids = np.ascontiguousarray(np.concatenate(sets) if sets else np.zeros(0), np.int64)
        return len(sets), off, ids

    def _records(self, count, read, shape, first, n, *more):
        """The held records, or records [first, first+n) counted from the (re)start, through a
        count-and-read pair: steps (n,), values (n, *shape). `more` are read's further arguments."""
        nw, nh = count()
        if first is None:
            first = nw - nh
        if n is None:
            n = nw - first
        steps = np.zeros(max(n, 0), np.int64)
        values = np.zeros((max(n, 0), *shape))
        check(read(self.ctx, int(first), int(n), ptr(steps, I64), ptr(values), *more))
        return steps, values

    def history_enable(self, sets=(), stride: int = 1, capacity: int = 1 << 16):
        """Per-step sums over node sets (hakai_history_enable): `sets` is a list of 1-based node id
        arrays (at most 15; set 0, every node, is always there). A record is kept every `stride`
        states, the newest `capacity` of them. On a rank (after set_interface) the ids are the
        rank's local ones (dist.local_sets), stride and capacity the same on every rank, and the
        records are the rank's partial sums over the nodes it owns (history_group combines them)."""
        n, off, nodes = self._record_sets(sets)
        check(self.L.hakai_history_enable(self.ctx, n, ptr(off, I64), ptr(nodes, I64), int(stride), int(capacity)))
        self._history_sets = n + 1

    def history_disable(self):
        check(self.L.hakai_history_disable(self.ctx))

    def history_count(self) -> tuple[int, int]:
        """(records written since the last (re)start, how many of the newest are still held)."""
        nw, nh = I64(0), I64(0)
        check(self.L.hakai_history_count(self.ctx, ctypes.byref(nw), ctypes.byref(nh)))
        return nw.value, nh.value

    def history(self, first: int | None = None, n: int | None = None) -> dict:
        """The held records (or records [first, first+n) counted from the (re)start): ``steps`` (n,),
        ``values`` (n, sets, 16), ``ke_seed`` (sets,) and one array per field of
        ``_abi.HISTORY_FIELDS`` -- (n, sets, 3) for F_int, F_ext, P, U; (n, sets) for KE, W_int,
        W_ext, W_bc."""
        ke = np.zeros(self._history_sets)
        steps, values = self._records(self.history_count, self.L.hakai_history_read, (self._history_sets, 16), first,
                                      n, ptr(ke))
        return _history_dict(steps, values, ke)

    # -- element-set history ------------------------------------------------------------------------
    def elem_history_enable(self, sets=(), stride: int = 1, capacity: int = 1 << 16):
        """Element-set records (hakai_elem_history_enable): `sets` is a list of 1-based element id
        arrays (at most 15; set 0, every element, is always there). The record of state k is kept
        when k % stride == 0, the newest `capacity` of them. On a rank the ids are the rank's local
        ones and the records its partials (elem_history_group combines them)."""
        n, off, elems = self._record_sets(sets)
        check(self.L.hakai_elem_history_enable(self.ctx, n, ptr(off, I64), ptr(elems, I64), int(stride),
                                               int(capacity)))
        self._elem_history_sets = n + 1

    def elem_history_disable(self):
        check(self.L.hakai_elem_history_disable(self.ctx))

    def elem_history_count(self) -> tuple[int, int]:
        """(records written since the last (re)start, how many of the newest are still held)."""
        nw, nh = I64(0), I64(0)
        check(self.L.hakai_elem_history_count(self.ctx, ctypes.byref(nw), ctypes.byref(nh)))
        return nw.value, nh.value

    def elem_history(self, first: int | None = None, n: int | None = None) -> dict:
        """The held records (or records [first, first+n) counted from the (re)start): ``steps`` (n,),
        ``values`` (n, sets, 24) and one array per field of ``_abi.ELEM_HISTORY_FIELDS`` --
        (n, sets, 6) for S and E, (n, sets) for the rest."""
        return _elem_history_dict(*self._records(self.elem_history_count, self.L.hakai_elem_history_read,
                                                 (self._elem_history_sets, 24), first, n))

    def elem_history_probe(self, sets=(), per_elem: bool = False) -> dict:
        """The record of the current state (hakai_elem_history_probe), with sets of its own: a dict by
        field name, (sets, 6) for S and E, (sets,) for the rest, ``values`` (sets, 24); with per_elem
        also ``per_elem`` (nElement, 20): V, V0, S[6], E[6], EQ, SE, PD, eqps_max, q_max, V / V0."""
        n, off, elems = self._record_sets(sets)
        values = np.zeros((n + 1, 24))
        pe = np.zeros((self.model.nElement, 20)) if per_elem else None
        check(self.L.hakai_elem_history_probe(self.ctx, n, ptr(off, I64), ptr(elems, I64), ptr(values), ptr(pe)))
        out = {k: v[0] for k, v in _elem_history_dict(np.zeros(1, np.int64), values[None]).items() if k != "steps"}
        if per_elem:
            out["per_elem"] = pe
        return out

    # -- stable time step -------------------------------------------------------------------------
    def stable_dt(self, d_time: float | None = None, mass_scaling: float | None = None,
                  per_element: bool = False) -> dict:
        """The stable-step diagnostic at the current state (hakai_stable_dt): ``dt_est`` (the
        conventional L / c, not a bound), ``dt_safe`` (a guaranteed lower bound of the elastic critical
        step; contact's penalty stiffness is outside it), the 1-based elements that attain them
        (``element_est``, ``element_safe``; 0: no active element) and ``n_active``, ``n_est_below``,
        ``n_safe_below`` counted against d_time. Defaults: the model's stepped ``dt`` and its
        ``mass_scaling``. per_element adds ``dt_est_elem`` and ``dt_safe_elem`` (nElement; +inf where
        the element is deleted)."""
        m = self.model
        r = StableDtT()
        nE = m.nElement
        est = np.zeros(nE) if per_element else None
        safe = np.zeros(nE) if per_element else None
        check(self.L.hakai_stable_dt(self.ctx, float(m.mass_scaling if mass_scaling is None else mass_scaling),
                                     float(m.dt if d_time is None else d_time), ctypes.byref(r), ptr(est), ptr(safe)))
        out = _stable_dict(r)
        if per_element:
            out.update(dt_est_elem=est, dt_safe_elem=safe)
        return out

    # -- selective mass scaling ----------------------------------------------------------------------
    def mass_scale(self, dt_target: float | None = None, safety: float = 0.9, max_factor: float = float("inf"),
                   mass_scaling: float | None = None) -> dict:
        """Add mass to the elements whose guaranteed stable step ``dt_safe`` is below ``dt_target`` at
        the current state, as much as brings it there (hakai_mass_scale); no other element changes.
        Defaults: the model's stepped ``dt`` and its ``mass_scaling``. Returns the fields of
        hakai_mass_scale_t: ``n_active``, ``n_scaled``, ``n_changed``, ``n_capped``, ``n_unfixable``,
        ``max_factor_reached`` with ``element_factor``, ``mass_added``, and the minimum ``dt_safe``
        after the call with ``element_safe``. Mass only grows; the same call again changes nothing."""
        m = self.model
        r = MassScaleT()
        check(self.L.hakai_mass_scale(self.ctx, float(m.mass_scaling if mass_scaling is None else mass_scaling),
                                      float(m.dt if dt_target is None else dt_target), float(safety),
                                      float(max_factor), ctypes.byref(r)))
        return {name: getattr(r, name) for name, _ in MassScaleT._fields_}

    def mass_scale_state(self) -> dict:
        """``elem_added`` (nElement: the mass added to each of the element's 8 nodes) and ``diag_M``
        (3 nNode: the mass the steps read) of the context (hakai_mass_scale_get)."""
        added, diag = np.zeros(self.model.nElement), np.zeros(3 * self.model.nNode)
        check(self.L.hakai_mass_scale_get(self.ctx, ptr(added), ptr(diag)))
        return dict(elem_added=added, diag_M=diag)

    def clear_mass_scale(self):
        """Back to the uploaded mass, bit for bit (hakai_clear_mass_scale)."""
        check(self.L.hakai_clear_mass_scale(self.ctx))

    # -- multi-GPU ---------------------------------------------------------------------------------
    def comm_init(self, rank: int, nranks: int, uid: bytes):
        buf = (ctypes.c_uint8 * 128).from_buffer_copy(uid)
        check(self.L.hakai_comm_init(self.ctx, rank, nranks, buf))

    def comm_init_local(self, rank: int, nranks: int, group_key: int):
        """Join an in-process group (same device); step the group with ``step_group``."""
        check(self.L.hakai_comm_init_local(self.ctx, rank, nranks, int(group_key)))

    def set_element_offset(self, offset: int):
        check(self.L.hakai_set_element_offset(self.ctx, int(offset)))

    def set_contact_global(self, glob: Model, local_node_global: np.ndarray, rank_elem_off: np.ndarray,
                           glob_diag_M: np.ndarray | None = None):
        """Multi-GPU contact (hakai_set_contact_global): this rank sets up the contact model of the
        global mesh `glob` (its contact_flag, instances, *Contact Pair surfaces and constants) and
        searches the entries of its own elements and nodes.
        Call after comm_init[_local], set_element_offset and set_interface."""
        if glob_diag_M is None:
            glob_diag_M, _ = glob.lumped_mass()
        diag = np.ascontiguousarray(glob_diag_M, np.float64)
        inst = glob.element_instance
        inst = np.ones(glob.nElement, np.int64) if inst is None else np.ascontiguousarray(inst, np.int64)
        ncp, cpi, cpo, cpe = glob.c_contact_pairs()
        l2g = np.ascontiguousarray(local_node_global, np.int64)
        off = np.ascontiguousarray(rank_elem_off, np.int64)
        check(self.L.hakai_set_contact_global(self.ctx, int(glob.contact_flag), glob.nNode, ptr(glob.coordmat),
                                              glob.nElement, ptr(glob.elementmat, I64),
                                              ptr(glob.element_material, I64), ptr(inst, I64), ptr(diag),
                                              ptr(l2g, I64), ptr(off, I64), ncp, ptr(cpi, ctypes.c_int32),
                                              ptr(cpo, I64), ptr(cpe, I64)))
        if glob.contact_flag >= 1 and getattr(glob, "contact_params", None) is not None:
            check(self.L.hakai_set_contact_params(self.ctx, *[float(x) for x in glob.contact_params]))

    def set_interface(self, local_node: np.ndarray, rank_lo: np.ndarray, rank_hi: np.ndarray):
        ln = np.ascontiguousarray(local_node, np.int64)
        lo = np.ascontiguousarray(rank_lo, np.int32)
        hi = np.ascontiguousarray(rank_hi, np.int32)
        check(self.L.hakai_set_interface(self.ctx, len(ln), ptr(ln, I64), ptr(lo, ctypes.c_int32),
                                         ptr(hi, ctypes.c_int32)))


def _history_dict(steps, values, ke) -> dict:
    from ._abi import HISTORY_FIELDS
    out = dict(steps=steps, values=values, ke_seed=ke)
    for name, lo, w in HISTORY_FIELDS:
        out[name] = values[:, :, lo:lo + w] if w > 1 else values[:, :, lo]
    return out


def history_combine(parts: list[dict]) -> dict:
    """The ranks' partial records (Solver.history() dicts, in rank order) as the record of the whole
    model (hakai_history_combine): ((p_0 + p_1) + p_2) + ... per value, the same dict as
    Solver.history()."""
    shapes = {(p["steps"].shape, p["values"].shape) for p in parts}
    if len(shapes) != 1:
        raise ValueError(f"history_combine: the ranks hold different record counts or sets: {sorted(shapes)}")
    steps = np.ascontiguousarray(np.stack([p["steps"] for p in parts]), np.int64)
    values = np.ascontiguousarray(np.stack([p["values"] for p in parts]), np.float64)
    ke = np.ascontiguousarray(np.stack([p["ke_seed"] for p in parts]), np.float64)
    R, n, S = values.shape[0], values.shape[1], values.shape[2]
    so, vo, ko = np.zeros(n, np.int64), np.zeros((n, S, 16)), np.zeros(S)
    check(lib().hakai_history_combine(R, S, n, ptr(steps, I64), ptr(values), ptr(ke), ptr(so, I64), ptr(vo),
                                      ptr(ko)))
    return _history_dict(so, vo, ko)


def history_group(solvers: list[Solver], first: int | None = None, n: int | None = None) -> dict:
    """The record of the whole model from a group of ranks (solvers[r] = rank r): every rank's
    history(first, n), combined in rank order. The same dict as Solver.history()."""
    return history_combine([sv.history(first, n) for sv in solvers])


def _elem_history_dict(steps, values) -> dict:
    from ._abi import ELEM_HISTORY_FIELDS
    out = dict(steps=steps, values=values)
    for name, lo, w in ELEM_HISTORY_FIELDS:
        out[name] = values[:, :, lo:lo + w] if w > 1 else values[:, :, lo]
    return out


def elem_history_combine(parts: list[dict]) -> dict:
    """The ranks' partial records (Solver.elem_history() dicts, in rank order) as the record of the
    whole model (hakai_elem_history_combine): sums added in rank order, extremes with the lower id
    among equals. The same dict as Solver.elem_history()."""
    shapes = {(p["steps"].shape, p["values"].shape) for p in parts}
    if len(shapes) != 1:
        raise ValueError(f"elem_history_combine: the ranks hold different record counts or sets: {sorted(shapes)}")
    steps = np.ascontiguousarray(np.stack([p["steps"] for p in parts]), np.int64)
    values = np.ascontiguousarray(np.stack([p["values"] for p in parts]), np.float64)
    R, n, S = values.shape[0], values.shape[1], values.shape[2]
    so, vo = np.zeros(n, np.int64), np.zeros((n, S, 24))
    check(lib().hakai_elem_history_combine(R, S, n, ptr(steps, I64), ptr(values), ptr(so, I64), ptr(vo)))
    return _elem_history_dict(so, vo)


def elem_history_group(solvers: list[Solver], first: int | None = None, n: int | None = None) -> dict:
    """The record of the whole model from a group of ranks (solvers[r] = rank r): every rank's
    elem_history(first, n), combined in rank order."""
    return elem_history_combine([sv.elem_history(first, n) for sv in solvers])


STABLE_DT_KEYS = tuple(name for name, _ in StableDtT._fields_)


def _stable_dict(r: StableDtT) -> dict:
    return {k: getattr(r, k) for k in STABLE_DT_KEYS}


def _stable_struct(d: dict, r: StableDtT | None = None) -> StableDtT:
    r = StableDtT() if r is None else r
    for (k, t) in StableDtT._fields_:
        setattr(r, k, float(d[k]) if t is ctypes.c_double else int(d[k]))
    return r


def stable_dt_combine(parts: list[dict]) -> dict:
    """The ranks' Solver.stable_dt() dicts as the whole model's (hakai_stable_dt_combine): the minimum
    over the ranks, an equal value to the lowest element id, counts summed."""
    arr = (StableDtT * len(parts))()
    for i, p in enumerate(parts):
        _stable_struct(p, arr[i])
    out = StableDtT()
    check(lib().hakai_stable_dt_combine(len(parts), arr, ctypes.byref(out)))
    return _stable_dict(out)


def stable_dt_group(solvers: list[Solver], d_time: float | None = None, mass_scaling: float | None = None) -> dict:
    """The diagnostic of the whole model from a group of ranks (element offsets set): every rank's
    stable_dt on its own elements, combined. Element ids are global."""
    return stable_dt_combine([sv.stable_dt(d_time, mass_scaling) for sv in solvers])


def write_stable_dt_csv(path: str, steps, records: list[dict], d_time: float):
    """Stable-step records (Solver.stable_dt() dicts, one per entry of steps) as CSV
    (hakai_stable_dt_write_csv)."""
    steps = np.ascontiguousarray(steps, np.int64)
    assert len(steps) == len(records), (len(steps), len(records))
    arr = (StableDtT * max(len(records), 1))()
    for i, p in enumerate(records):
        _stable_struct(p, arr[i])
    check(lib().hakai_stable_dt_write_csv(str(path).encode(), len(records), ptr(steps, I64), arr, float(d_time)))


def read_stable_dt_csv(path: str) -> dict:
    """A stable_dt.csv back as dict(steps, time, d_time, records): the same doubles."""
    with open(path) as fh:
        head = fh.readline().strip().split(",")
        rows = [ln.strip().split(",") for ln in fh if ln.strip()]
    assert head == ["step", "time", "d_time", *STABLE_DT_KEYS], head
    conv = [float if t is ctypes.c_double else int for _, t in StableDtT._fields_]
    return dict(steps=np.array([int(r[0]) for r in rows], np.int64), time=np.array([float(r[1]) for r in rows]),
                d_time=np.array([float(r[2]) for r in rows]),
                records=[{k: f(x) for k, f, x in zip(STABLE_DT_KEYS, conv, r[3:])} for r in rows])


def step_group(solvers: list[Solver], t_first: float, n_steps: int, d_time: float | None = None):
    """Advance an in-process group (hakai_comm_init_local, solvers[r] = rank r) in lockstep
    (hakai_step_group): per step every rank's contact search, then every rank's exchange and update."""
    if not solvers:
        return
    arr = (ctypes.c_void_p * len(solvers))(*[sv.ctx for sv in solvers])
    dt = solvers[0].model.dt if d_time is None else d_time
    check(lib().hakai_step_group(arr, len(solvers), float(t_first), int(n_steps), float(dt)))


def comm_unique_id() -> bytes:
    buf = (ctypes.c_uint8 * 128)()
    check(lib().hakai_comm_unique_id(buf))
    return bytes(buf)


# ---- literal mirrors of the reference functions ---------------------------------------------------
def cal_stress_hexa(Qe, integ_stress, integ_strain, integ_yield_stress, integ_eq_plastic_strain, position,
                    d_disp, elementmat, element_flag, integ_num, Pusai_mat, MATERIAL, element_material,
                    elementMinSize, elementVolume, device: int = 0):
    """cal_stress_hexa (v2/HAKAI_j.jl:1033-1036), arrays in the reference's layout, mutated in place:
    Qe (nE,24) accumulates; integ_* (8nE,6)/(8nE,); position (nN,3); d_disp (3nN,);
    elementmat (nE,8) 1-based; MATERIAL a list of model.Material. Pusai_mat and elementMinSize are
    accepted for signature parity and not needed (the kernel builds Pusai in registers)."""
    from .model import Model
    tmp = Model(position, elementmat, element_material, MATERIAL)
    mats, keep = tmp.c_materials()
    nN, nE = position.shape[0], elementmat.shape[0]
    check(lib().hakai_stress_hexa(device, nN, nE, ptr(Qe), ptr(integ_stress), ptr(integ_strain),
                                  ptr(integ_yield_stress), ptr(integ_eq_plastic_strain),
                                  ptr(np.ascontiguousarray(position, np.float64)),
                                  ptr(np.ascontiguousarray(d_disp, np.float64)),
                                  ptr(tmp.elementmat, I64), ptr(np.ascontiguousarray(element_flag, np.int64), I64),
                                  int(integ_num), len(MATERIAL), mats, ptr(tmp.element_material, I64),
                                  ptr(elementVolume)))
    del keep


def cal_triax_stress(integ_stress, integ_triax_stress, device: int = 0):
    """cal_triax_stress (v2/HAKAI_j.jl:982), in place."""
    st = np.ascontiguousarray(integ_stress, np.float64)
    check(lib().hakai_triax_stress(device, st.shape[0], ptr(st), ptr(integ_triax_stress)))


def _write_records_csv(write, F: int, path: str, set_names, steps, values, d_time: float):
    steps = np.ascontiguousarray(steps, np.int64)
    values = np.ascontiguousarray(values, np.float64)
    names = (ctypes.c_char_p * len(set_names))(*[str(s).encode() for s in set_names])
    assert values.shape == (len(steps), len(set_names), F), values.shape
    check(write(str(path).encode(), len(set_names), names, len(steps), ptr(steps, I64), ptr(values), float(d_time)))


def _read_records_csv(path: str, F: int, field0: str) -> dict:
    with open(path) as fh:
        head = fh.readline().strip().split(",")
        rows = [ln.strip().split(",") for ln in fh if ln.strip()]
    sets = [h[:-len("_" + field0)] for h in head[2::F]]
    steps = np.array([int(r[0]) for r in rows], np.int64)
    time = np.array([float(r[1]) for r in rows])
    values = np.array([[float(x) for x in r[2:]] for r in rows]).reshape(len(rows), len(sets), F)
    return dict(sets=sets, steps=steps, time=time, values=values)


def write_history_csv(path: str, set_names, steps, values, d_time: float):
    """History records as CSV (hakai_history_write_csv): values (n, sets, 16), set 0's name first."""
    _write_records_csv(lib().hakai_history_write_csv, 16, path, set_names, steps, values, d_time)


def read_history_csv(path: str) -> dict:
    """A history.csv back as dict(sets, steps, time, values (n, sets, 16)): the same doubles."""
    return _read_records_csv(path, 16, "F_int_x")


def write_elem_history_csv(path: str, set_names, steps, values, d_time: float):
    """Element-set records as CSV (hakai_elem_history_write_csv): values (n, sets, 24), set 0's name first."""
    _write_records_csv(lib().hakai_elem_history_write_csv, 24, path, set_names, steps, values, d_time)


def read_elem_history_csv(path: str) -> dict:
    """An elem_history.csv back as dict(sets, steps, time, values (n, sets, 24)): the same doubles."""
    return _read_records_csv(path, 24, "N_active")


MASS_SCALE_CSV = ("step", "dt_target", "n_active", "n_scaled", "n_changed", "n_capped", "n_unfixable", "mass_added",
                  "max_factor_reached", "element_factor", "dt_safe", "element_safe")


def read_mass_scale_csv(path: str) -> list[dict]:
    """A driver's mass_scale.csv back as one dict per application: the same doubles (step and dt_target,
    then Solver.mass_scale()'s fields)."""
    with open(path) as fh:
        head = fh.readline().strip().split(",")
        assert tuple(head) == MASS_SCALE_CSV, head
        flt = ("dt_target", "mass_added", "max_factor_reached", "dt_safe")
        return [{k: (float(v) if k in flt else int(v)) for k, v in zip(head, ln.strip().split(","))}
                for ln in fh if ln.strip()]


def hakai(fname: str, out_dir: str = "temp", device: int = 0, verbose: bool = True):
    """HAKAI(fname) (v2/HAKAI_j.jl:81): run the deck on the GPU and write out_dir/file%03d.vtk.
    Env HAKAI_HISTORY=<stride> also writes out_dir/history.csv, env HAKAI_DT_CHECK=1 also
    out_dir/stable_dt.csv; a deck with *Variable Mass Scaling (Model.variable_mass_scaling) gets its
    mass scaled after the reset (repeat=output: at every output state too) and out_dir/mass_scale.csv
    (hakai_run_inp)."""
    check(lib().hakai_run_inp(str(fname).encode(), str(out_dir).encode(), device, int(verbose)))
