"""HAKAI model container in the reference's own layout (ModelType, v2/readInpFile_j.jl:129-150).

All index arrays are int64 and 1-based, exactly like the Julia arrays:
  coordmat (nNode, 3) C-order  == Julia 3 x nNode column-major
  elementmat (nElement, 8)     == Julia 8 x nElement column-major
Boundary conditions keep the BCType structure (groups of (dof list, value) with an optional
amplitude); the initial velocity is flattened to (dofs, values) in IC order.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field

import numpy as np

from . import _abi
from ._abi import BCT, LoadsT, MaterialT, WallsT, check, lib, ptr


@dataclass
class Material:
    """MaterialType (v2/readInpFile_j.jl:84-96): density, elastic, *Plastic table, DUCTILE table."""
    name: str
    density: float
    young: float
    poisson: float
    plastic: np.ndarray = field(default_factory=lambda: np.zeros((0, 2)))   # (yield stress, eq. plastic strain)
    ductile: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))   # (fracture strain, triax, rate)


@dataclass
class BCGroup:
    """One *Boundary block (BCType, v2/readInpFile_j.jl:98-104)."""
    entries: list  # [(dofs int64 1-based, value float)]
    amp_time: np.ndarray | None = None
    amp_value: np.ndarray | None = None


@dataclass
class Loads:
    """External loads (hakai_loads_t, include/hakai_hip.h): global 1-based ids. ``amps`` is a list of
    (time, value) tables of at least two rows; a load's ``*_amp`` is an index into it, -1 the constant 1.
    ``grav_accel`` is (n_grav, 3), magnitude times direction; ``press_face`` is 1..6 (S1..S6)."""
    amps: list = field(default_factory=list)
    cload_dof: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    cload_value: np.ndarray = field(default_factory=lambda: np.zeros(0))
    cload_amp: np.ndarray | None = None
    grav_accel: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    grav_amp: np.ndarray | None = None
    press_elem: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    press_face: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int32))
    press_value: np.ndarray = field(default_factory=lambda: np.zeros(0))
    press_amp: np.ndarray | None = None

    def __post_init__(self):
        self.amps = [(np.ascontiguousarray(t, np.float64).ravel(), np.ascontiguousarray(v, np.float64).ravel())
                     for t, v in self.amps]
        self.cload_dof = np.ascontiguousarray(self.cload_dof, np.int64).ravel()
        self.cload_value = np.ascontiguousarray(self.cload_value, np.float64).ravel()
        self.grav_accel = np.ascontiguousarray(self.grav_accel, np.float64).reshape(-1, 3)
        self.press_elem = np.ascontiguousarray(self.press_elem, np.int64).ravel()
        self.press_face = np.ascontiguousarray(self.press_face, np.int32).ravel()
        self.press_value = np.ascontiguousarray(self.press_value, np.float64).ravel()
        for name, n in (("cload_amp", len(self.cload_dof)), ("grav_amp", len(self.grav_accel)),
                        ("press_amp", len(self.press_elem))):
            a = getattr(self, name)
            a = np.full(n, -1, np.int32) if a is None else np.ascontiguousarray(a, np.int32).ravel()
            setattr(self, name, a)

    @property
    def empty(self) -> bool:
        return len(self.cload_dof) == 0 and len(self.grav_accel) == 0 and len(self.press_elem) == 0

    def c(self):
        """(LoadsT, holder): keep the holder alive while the C side uses the struct."""
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        amp_n = np.array([len(t) for t, _ in self.amps], np.int32)
        amp_off = np.zeros(len(self.amps), np.int64)
        if len(self.amps) > 1:
            amp_off[1:] = np.cumsum(amp_n[:-1])
        pad = [np.zeros(1)]  # (a pointer even where a list is empty)
        at = np.ascontiguousarray(np.concatenate([t for t, _ in self.amps] + pad))
        av = np.ascontiguousarray(np.concatenate([v for _, v in self.amps] + pad))
        s = LoadsT()
        s.n_amp, s.amp_n, s.amp_off, s.amp_time, s.amp_value = len(self.amps), ptr(amp_n, i32), ptr(amp_off, i64), \
            ptr(at), ptr(av)
        s.n_cload, s.cload_dof, s.cload_value, s.cload_amp = len(self.cload_dof), ptr(self.cload_dof, i64), \
            ptr(self.cload_value), ptr(self.cload_amp, i32)
        s.n_grav, s.grav_accel, s.grav_amp = len(self.grav_accel), ptr(self.grav_accel), ptr(self.grav_amp, i32)
        s.n_press, s.press_elem, s.press_face, s.press_value, s.press_amp = len(self.press_elem), \
            ptr(self.press_elem, i64), ptr(self.press_face, i32), ptr(self.press_value), ptr(self.press_amp, i32)
        return s, (amp_n, amp_off, at, av, self)


@dataclass
class Walls:
    """Rigid walls (hakai_walls_t, include/hakai_hip.h): up to 32 moving planes with penalty, damping
    and Coulomb friction. ``origin``, ``normal``, ``motion`` are (n_wall, 3); ``normal`` is any non-zero
    vector pointing into the half-space the nodes may occupy (the library normalises it). ``amps`` is
    a list of (time, value) tables of at least two rows and ``amp`` an index into it per wall, -1 the
    constant 1: the wall is displaced by motion * amp(time). ``nodes`` is one array of global 1-based
    ids per wall; an empty one (or None) means every node. Defaults as the deck keyword's: stiffness
    0, scale 0.5, damping 0, friction 0, no motion."""
    origin: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    normal: np.ndarray = field(default_factory=lambda: np.zeros((0, 3)))
    motion: np.ndarray | None = None
    amp: np.ndarray | None = None
    stiffness: np.ndarray | None = None
    scale: np.ndarray | None = None
    damping: np.ndarray | None = None
    friction: np.ndarray | None = None
    nodes: list | None = None
    amps: list = field(default_factory=list)

    def __post_init__(self):
        self.amps = [(np.ascontiguousarray(t, np.float64).ravel(), np.ascontiguousarray(v, np.float64).ravel())
                     for t, v in self.amps]
        self.origin = np.ascontiguousarray(self.origin, np.float64).reshape(-1, 3)
        self.normal = np.ascontiguousarray(self.normal, np.float64).reshape(-1, 3)
        n = len(self.origin)
        self.motion = np.zeros((n, 3)) if self.motion is None else \
            np.ascontiguousarray(self.motion, np.float64).reshape(-1, 3)
        self.amp = np.full(n, -1, np.int32) if self.amp is None else np.ascontiguousarray(self.amp, np.int32).ravel()
        for name, default in (("stiffness", 0.0), ("scale", 0.5), ("damping", 0.0), ("friction", 0.0)):
            a = getattr(self, name)
            a = np.full(n, default) if a is None else np.ascontiguousarray(a, np.float64).ravel()
            setattr(self, name, a)
        nodes = [None] * n if self.nodes is None else list(self.nodes)
        self.nodes = [np.zeros(0, np.int64) if x is None else np.ascontiguousarray(x, np.int64).ravel() for x in nodes]
        for name in ("normal", "motion", "amp", "stiffness", "scale", "damping", "friction", "nodes"):
            if len(getattr(self, name)) != n:
                raise ValueError(f"Walls.{name}: {len(getattr(self, name))} entries for {n} walls")

    @property
    def n_wall(self) -> int:
        return len(self.origin)

    @property
    def empty(self) -> bool:
        return self.n_wall == 0

    def c(self):
        """(WallsT, holder): keep the holder alive while the C side uses the struct."""
        i32, i64 = ctypes.c_int32, ctypes.c_int64
        amp_n = np.array([len(t) for t, _ in self.amps], np.int32)
        amp_off = np.zeros(len(self.amps), np.int64)
        if len(self.amps) > 1:
            amp_off[1:] = np.cumsum(amp_n[:-1])
        pad = [np.zeros(1)]  # (a pointer even where a list is empty)
        at = np.ascontiguousarray(np.concatenate([t for t, _ in self.amps] + pad))
        av = np.ascontiguousarray(np.concatenate([v for _, v in self.amps] + pad))
        node_off = np.concatenate([[0], np.cumsum([len(x) for x in self.nodes])]).astype(np.int64)
        nodes = np.ascontiguousarray(np.concatenate(self.nodes + [np.zeros(1, np.int64)]))
        arrs = [np.ascontiguousarray(np.concatenate([a.ravel(), np.zeros(1, a.dtype)]))
                for a in (self.origin, self.normal, self.motion, self.amp, self.stiffness, self.scale, self.damping,
                          self.friction)]
        s = WallsT()
        s.n_amp, s.amp_n, s.amp_off, s.amp_time, s.amp_value = len(self.amps), ptr(amp_n, i32), ptr(amp_off, i64), \
            ptr(at), ptr(av)
        s.n_wall = self.n_wall
        s.origin, s.normal, s.motion, s.amp = ptr(arrs[0]), ptr(arrs[1]), ptr(arrs[2]), ptr(arrs[3], i32)
        s.stiffness, s.scale, s.damping, s.friction = ptr(arrs[4]), ptr(arrs[5]), ptr(arrs[6]), ptr(arrs[7])
        s.node_off, s.nodes = ptr(node_off, i64), ptr(nodes, i64)
        return s, (amp_n, amp_off, at, av, node_off, nodes, arrs, self)


@dataclass
class Model:
    coordmat: np.ndarray
    elementmat: np.ndarray
    element_material: np.ndarray
    materials: list
    bc: list = field(default_factory=list)
    ic_dofs: np.ndarray = field(default_factory=lambda: np.zeros(0, np.int64))
    ic_values: np.ndarray = field(default_factory=lambda: np.zeros(0))
    d_time: float = 1e-7          # *Dynamic, Explicit increment (before mass scaling)
    end_time: float = 1e-4
    mass_scaling: float = 1.0
    contact_flag: int = 0
    element_instance: np.ndarray | None = None
    name: str = "model"
    # cal_contact_force constants (myu, kc_o, kc_s, Cr_o, Cr_s); None = the reference's
    # hard-coded (0.25, 1, 1, 0, 0) (v2/HAKAI_j.jl:2255-2259)
    contact_params: tuple | None = None
    # *Contact Pair surfaces: [((instance, elements), (instance, elements)), ...] with 1-based
    # instances and instance-local 1-based element ids; None = all-exterior contact
    contact_pairs: list | None = None
    # read_inp: the drivers' history sets of the deck (hakai_inp_history_sets) -- (names with "all"
    # first, [global 1-based node ids per kept set], names left out); None for a model built in code
    history_sets: tuple | None = None
    # read_inp: the drivers' element-set history sets (hakai_inp_elem_history_sets) -- (names with "all"
    # first, [global 1-based element ids per kept set], names left out); None for a model built in code
    elem_history_sets: tuple | None = None
    # external loads (*Cload, *Dload, *Dsload of a deck; Solver applies them); None = no loads
    loads: Loads | None = None
    # rigid walls (*Rigid Wall of a deck; Solver applies them); None = no wall
    walls: Walls | None = None
    # *Variable Mass Scaling of a deck: dict(dt=target or None for the stepped dt, safety=, max_factor=,
    # repeat=True for repeat=output); None = the deck has none. The one-GPU drivers (hakai.hakai, the
    # hakai CLI) apply it; a Solver does not on its own -- call Solver.mass_scale(**...) where wanted
    variable_mass_scaling: dict | None = None

    def c_contact_pairs(self):
        """(n_cp, cp_instance int32[2n], cp_elem_off int64[2n+1], cp_elems int64[]) for the C ABI."""
        cps = self.contact_pairs or []
        inst = np.array([s[0] for cp in cps for s in cp], np.int32)
        lists = [np.asarray(s[1], np.int64) for cp in cps for s in cp]
        off = np.concatenate([[0], np.cumsum([len(x) for x in lists])]).astype(np.int64)
        els = np.concatenate(lists).astype(np.int64) if lists else np.zeros(0, np.int64)
        return len(cps), np.ascontiguousarray(inst), np.ascontiguousarray(off), np.ascontiguousarray(els)

    def __post_init__(self):
        self.coordmat = np.ascontiguousarray(self.coordmat, dtype=np.float64)
        self.elementmat = np.ascontiguousarray(self.elementmat, dtype=np.int64)
        self.element_material = np.ascontiguousarray(self.element_material, dtype=np.int64)
        self.ic_dofs = np.ascontiguousarray(self.ic_dofs, dtype=np.int64)
        self.ic_values = np.ascontiguousarray(self.ic_values, dtype=np.float64)

    @property
    def nNode(self) -> int:
        return self.coordmat.shape[0]

    @property
    def nElement(self) -> int:
        return self.elementmat.shape[0]

    @property
    def dt(self) -> float:
        """Step after mass scaling (v2/HAKAI_j.jl:114)."""
        return self.d_time * np.sqrt(self.mass_scaling)

    @property
    def time_num(self) -> float:
        return self.end_time / self.dt

    @property
    def n_steps(self) -> int:
        """Iterations of `for t = 1:time_num` (Float64 range)."""
        tn = self.time_num
        return int(np.floor(tn)) if tn >= 1 else 0

    # ---- ctypes views (keep the returned holder alive while the C side uses it) ----
    def c_materials(self):
        keep = []
        arr = (MaterialT * len(self.materials))()
        for i, m in enumerate(self.materials):
            pl = np.ascontiguousarray(m.plastic, dtype=np.float64).reshape(-1, 2)
            du = np.ascontiguousarray(m.ductile, dtype=np.float64).reshape(-1, 3)
            keep += [pl, du]
            arr[i].density, arr[i].young, arr[i].poisson = m.density, m.young, m.poisson
            arr[i].n_plastic, arr[i].plastic = pl.shape[0], ptr(pl)
            arr[i].n_ductile, arr[i].ductile = du.shape[0], ptr(du)
        return arr, keep

    def bc_arrays(self):
        amp_n, amp_off, amp_t, amp_v, entry_off, entry_val, dof_off, dofs = [], [], [], [], [], [], [], []
        for g in self.bc:
            amp_off.append(len(amp_t))
            if g.amp_time is None:
                amp_n.append(0)
            else:
                amp_n.append(len(g.amp_time))
                amp_t += list(np.asarray(g.amp_time, dtype=np.float64))
                amp_v += list(np.asarray(g.amp_value, dtype=np.float64))
            entry_off.append(len(entry_val))
            for d, v in g.entries:
                dof_off.append(len(dofs))
                entry_val.append(float(v))
                dofs += list(np.asarray(d, dtype=np.int64))
        entry_off.append(len(entry_val))
        dof_off.append(len(dofs))
        return dict(amp_n=np.array(amp_n, np.int32), amp_off=np.array(amp_off, np.int64),
                    amp_time=np.array(amp_t + [0.0], np.float64), amp_value=np.array(amp_v + [0.0], np.float64),
                    entry_off=np.array(entry_off, np.int64), entry_value=np.array(entry_val + [0.0], np.float64),
                    dof_off=np.array(dof_off, np.int64), dofs=np.array(dofs + [0], np.int64))

    def c_bc(self):
        a = self.bc_arrays()
        s = BCT()
        s.n_groups = len(self.bc)
        s.amp_n = ptr(a["amp_n"], ctypes.c_int32)
        s.amp_off = ptr(a["amp_off"], ctypes.c_int64)
        s.amp_time = ptr(a["amp_time"])
        s.amp_value = ptr(a["amp_value"])
        s.entry_off = ptr(a["entry_off"], ctypes.c_int64)
        s.entry_value = ptr(a["entry_value"])
        s.dof_off = ptr(a["dof_off"], ctypes.c_int64)
        s.dofs = ptr(a["dofs"], ctypes.c_int64)
        return s, a

    def lumped_mass(self) -> tuple[np.ndarray, np.ndarray]:
        """diag_M (3nN, per dof) and elementVolume via the library's host code (v2/HAKAI_j.jl:183-218)."""
        mats, keep = self.c_materials()
        diag = np.zeros(3 * self.nNode)
        vol = np.zeros(self.nElement)
        check(lib().hakai_lumped_mass(self.nNode, ptr(self.coordmat), self.nElement,
                                      ptr(self.elementmat, ctypes.c_int64), ptr(self.element_material, ctypes.c_int64),
                                      len(self.materials), mats, self.mass_scaling, ptr(diag), ptr(vol)))
        del keep
        return diag, vol


def _arr(p, n, dtype):
    if n == 0:
        return np.zeros(0, dtype=dtype)
    return np.ctypeslib.as_array(p, shape=(n,)).astype(dtype, copy=True)


def read_inp(path: str) -> Model:
    """readInpFile (v2/readInpFile_j.jl:152) through the library's C++ reader."""
    L = lib()
    out = ctypes.POINTER(_abi.InpModelT)()
    check(L.hakai_inp_read(str(path).encode(), ctypes.byref(out)))
    try:
        m = out.contents
        nN, nE = m.nNode, m.nElement
        coord = _arr(m.coordmat, 3 * nN, np.float64).reshape(nN, 3)
        elem = _arr(m.elementmat, 8 * nE, np.int64).reshape(nE, 8)
        emat = _arr(m.element_material, nE, np.int64)
        einst = _arr(m.element_instance, nE, np.int64)
        mats = []
        for i in range(m.nMat):
            mt = m.materials[i]
            pl = _arr(mt.plastic, 2 * mt.n_plastic, np.float64).reshape(-1, 2)
            du = _arr(mt.ductile, 3 * mt.n_ductile, np.float64).reshape(-1, 3)
            mats.append(Material(f"mat{i + 1}", mt.density, mt.young, mt.poisson, pl, du))
        bc = []
        b = m.bc
        G = b.n_groups
        if G:
            entry_off = _arr(b.entry_off, G + 1, np.int64)
            n_ent = int(entry_off[-1])
            dof_off = _arr(b.dof_off, n_ent + 1, np.int64)
            dofs = _arr(b.dofs, int(dof_off[-1]), np.int64)
            vals = _arr(b.entry_value, n_ent, np.float64)
            amp_n = _arr(b.amp_n, G, np.int32)
            amp_off = _arr(b.amp_off, G, np.int64)
            n_amp = int(max([amp_off[g] + amp_n[g] for g in range(G)] + [0]))
            at = _arr(b.amp_time, n_amp, np.float64)
            av = _arr(b.amp_value, n_amp, np.float64)
            for g in range(G):
                ents = [(dofs[dof_off[j]:dof_off[j + 1]].copy(), float(vals[j]))
                        for j in range(entry_off[g], entry_off[g + 1])]
                if amp_n[g] > 0:
                    sl = slice(amp_off[g], amp_off[g] + amp_n[g])
                    bc.append(BCGroup(ents, at[sl].copy(), av[sl].copy()))
                else:
                    bc.append(BCGroup(ents))
        ic_d = _arr(m.ic_dofs, m.n_ic_dofs, np.int64)
        ic_v = _arr(m.ic_values, m.n_ic_dofs, np.float64)
        cps = None
        if m.n_cp > 0:
            inst = _arr(m.cp_instance, 2 * m.n_cp, np.int64)
            off = _arr(m.cp_elem_off, 2 * m.n_cp + 1, np.int64)
            els = _arr(m.cp_elems, int(off[-1]), np.int64)
            cps = [tuple((int(inst[2 * k + s]), els[off[2 * k + s]:off[2 * k + s + 1]].copy()) for s in range(2))
                   for k in range(m.n_cp)]
        # the sets HAKAI_HISTORY records, from the one definition both drivers use
        ns, nd = ctypes.c_int32(0), ctypes.c_int32(0)
        hoff = np.zeros(_abi.HISTORY_MAX_SETS + 1, np.int64)
        check(L.hakai_inp_history_sets(out, ctypes.byref(ns), ptr(hoff, ctypes.c_int64), None, 0, None, 0,
                                       ctypes.byref(nd)))
        hnodes = np.zeros(max(int(hoff[ns.value]), 1), np.int64)
        cap = 32 * (ns.value + nd.value + 2)
        text = ctypes.create_string_buffer(cap)
        check(L.hakai_inp_history_sets(out, ctypes.byref(ns), ptr(hoff, ctypes.c_int64), ptr(hnodes, ctypes.c_int64),
                                       len(hnodes), text, cap, ctypes.byref(nd)))
        hnames = text.value.decode().split("\n")[:-1]
        hsets = [hnodes[hoff[s]:hoff[s + 1]].copy() for s in range(ns.value)]
        # the sets HAKAI_ELEM_HISTORY records
        es, ed = ctypes.c_int32(0), ctypes.c_int32(0)
        eoff = np.zeros(_abi.ELEM_HISTORY_MAX_SETS + 1, np.int64)
        check(L.hakai_inp_elem_history_sets(out, ctypes.byref(es), ptr(eoff, ctypes.c_int64), None, 0, None, 0,
                                            ctypes.byref(ed)))
        eelems = np.zeros(max(int(eoff[es.value]), 1), np.int64)
        check(L.hakai_inp_elem_history_sets(out, ctypes.byref(es), ptr(eoff, ctypes.c_int64), ptr(eelems, ctypes.c_int64),
                                            len(eelems), None, 0, ctypes.byref(ed)))
        ecap = 1 << 16
        etext = ctypes.create_string_buffer(ecap)
        check(L.hakai_inp_elem_history_sets(out, ctypes.byref(es), ptr(eoff, ctypes.c_int64), None, 0, etext, ecap,
                                            ctypes.byref(ed)))
        enames = etext.value.decode().split("\n")[:-1]
        esets = [eelems[eoff[s]:eoff[s + 1]].copy() for s in range(es.value)]
        ld, loads = m.loads, None
        if ld.n_cload or ld.n_grav or ld.n_press:
            lo = _arr(ld.amp_off, ld.n_amp, np.int64)
            ln = _arr(ld.amp_n, ld.n_amp, np.int32)
            n_amp = int(max([lo[a] + ln[a] for a in range(ld.n_amp)] + [0]))
            lt, lv = _arr(ld.amp_time, n_amp, np.float64), _arr(ld.amp_value, n_amp, np.float64)
            loads = Loads([(lt[lo[a]:lo[a] + ln[a]].copy(), lv[lo[a]:lo[a] + ln[a]].copy()) for a in range(ld.n_amp)],
                          _arr(ld.cload_dof, ld.n_cload, np.int64), _arr(ld.cload_value, ld.n_cload, np.float64),
                          _arr(ld.cload_amp, ld.n_cload, np.int32),
                          _arr(ld.grav_accel, 3 * ld.n_grav, np.float64).reshape(-1, 3),
                          _arr(ld.grav_amp, ld.n_grav, np.int32), _arr(ld.press_elem, ld.n_press, np.int64),
                          _arr(ld.press_face, ld.n_press, np.int32), _arr(ld.press_value, ld.n_press, np.float64),
                          _arr(ld.press_amp, ld.n_press, np.int32))
        wl, walls = m.walls, None
        if wl.n_wall:
            nw = wl.n_wall
            wo = _arr(wl.amp_off, wl.n_amp, np.int64)
            wn = _arr(wl.amp_n, wl.n_amp, np.int32)
            n_amp = int(max([wo[a] + wn[a] for a in range(wl.n_amp)] + [0]))
            wt, wv = _arr(wl.amp_time, n_amp, np.float64), _arr(wl.amp_value, n_amp, np.float64)
            noff = _arr(wl.node_off, nw + 1, np.int64)
            wnodes = _arr(wl.nodes, int(noff[-1]), np.int64)
            walls = Walls(_arr(wl.origin, 3 * nw, np.float64), _arr(wl.normal, 3 * nw, np.float64),
                          _arr(wl.motion, 3 * nw, np.float64), _arr(wl.amp, nw, np.int32),
                          _arr(wl.stiffness, nw, np.float64), _arr(wl.scale, nw, np.float64),
                          _arr(wl.damping, nw, np.float64), _arr(wl.friction, nw, np.float64),
                          [wnodes[noff[w]:noff[w + 1]].copy() for w in range(nw)],
                          [(wt[wo[a]:wo[a] + wn[a]].copy(), wv[wo[a]:wo[a] + wn[a]].copy()) for a in range(wl.n_amp)])
        vms = None
        if m.vms_set:
            vms = dict(dt=float(m.vms_dt) if m.vms_dt > 0 else None, safety=float(m.vms_safety),
                       max_factor=float(m.vms_max_factor), repeat=bool(m.vms_repeat))
        return Model(coord, elem, emat, mats, bc, ic_d, ic_v, m.d_time, m.end_time, m.mass_scaling,
                     m.contact_flag, einst, name=str(path), contact_pairs=cps,
                     history_sets=(hnames[:ns.value + 1], hsets, hnames[ns.value + 1:]),
                     elem_history_sets=(enames[:es.value + 1], esets, enames[es.value + 1:]), loads=loads, walls=walls,
                     variable_mass_scaling=vms)
    finally:
        L.hakai_inp_free(out)
