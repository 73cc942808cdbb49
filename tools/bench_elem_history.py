#!/usr/bin/env python3
"""Cost of the element-set history: wall time per step with the feature off, at stride 1 and at
stride 100, the time of one probe, and both launch forms around the one-block threshold.

    python tools/bench_elem_history.py c3            # one context, C3 (2 M hex)
    python tools/bench_elem_history.py tensile5e     # the Tensile5e deck's mesh (launch-bound)
    python tools/bench_elem_history.py forms         # probe time of both launch forms at 128 .. 4096 elements

Settling steps before each timed run, as tools/bench_history.py; prints one JSON line (median and
every round). The driver's sets of a deck are not known here: c3 and tensile5e record set 0 and
three sets (the lower half, the upper half and every second element)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hakai-fem_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
from bench_history import timed  # noqa: E402


def probe_ms(sv, sets, n=20):
    sv.elem_history_probe(sets)
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        sv.elem_history_probe(sets)
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("c3", "tensile5e", "forms"))
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle", type=int, default=30)
    a = ap.parse_args()
    from hakai import mesh
    from hakai.solver import Solver
    out = {"mode": a.mode, "lib": os.environ.get("HAKAI_LIB", "this tree"), "steps": a.steps, "rounds": a.rounds,
           "settle": a.settle}
    if a.mode == "forms":
        out["probe_ms"] = {}
        for nz in (2, 4, 8, 16, 32, 64):            # 8 x 8 x nz: 128 .. 4096 elements
            m = mesh.bar_model(8, 8, nz, mesh.steel_ductile(), lambda z, L: 5e4 * z / L, d_time=1e-8, n_steps=10)
            row = {}
            for form in (1, 0):
                with Solver(m) as sv:
                    sv.set_tuning("elem_history_one_block", form)
                    sv.step(1, 4)
                    row["one_block" if form else "two_launches"] = probe_ms(sv, [])
            out["probe_ms"][m.nElement] = row
        print(json.dumps(out), flush=True)
        return
    m = mesh.config_c3() if a.mode == "c3" else mesh.tensile5e_model()
    nE = m.nElement
    sets = [np.arange(1, nE // 2 + 1), np.arange(nE // 2 + 1, nE + 1), np.arange(1, nE + 1, 2)]
    out["elements"] = nE
    with Solver(m) as sv:
        t, out["off"] = timed(sv.step, sv.sync, 1, a.settle, a.rounds, a.steps)
        for stride in (1, 100):
            sv.elem_history_enable(sets, stride=stride, capacity=64)
            t, out[f"stride{stride}"] = timed(sv.step, sv.sync, t, a.settle, a.rounds, a.steps)
        sv.elem_history_disable()
        t, out["off_again"] = timed(sv.step, sv.sync, t, a.settle, a.rounds, a.steps)
        out["probe"] = probe_ms(sv, sets)
        out["graph_steps"] = sv.graph_steps()
    out["record_ms"] = out["stride1"]["median_ms"] - out["off"]["median_ms"]
    out["stride100_ms_per_step"] = out["stride100"]["median_ms"] - out["off"]["median_ms"]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
