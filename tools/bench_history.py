#!/usr/bin/env python3
"""Cost of history output: wall time per step with history off and at stride 1.

    python tools/bench_history.py c3                 # one context, C3 (2 M hex)
    python tools/bench_history.py ranks              # 2-rank in-process group, a C3-size slab per rank
    HAKAI_LIB=<another build> python tools/bench_history.py c3     # A/B against another library

`ranks` drains one rank's phase before the next rank's (tuning group_serial 1, as
tools/bench_contact.py --ranks), so the ranks do not share the one GPU while they are timed: the
group's time per step is the sum of the ranks'. Settling steps before each timed run; prints one JSON
line (median and every round)."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hakai-fem_amd"))


def timed(step, sync, t, settle, rounds, steps):
    step(t, settle)
    sync()
    t += settle
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        step(t, steps)
        sync()
        ms.append((time.perf_counter() - t0) / steps * 1e3)
        t += steps
    return t, {"median_ms": statistics.median(ms), "min_ms": min(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("c3", "ranks"))
    ap.add_argument("--layers", type=int, default=5000, help="z layers per context (C3: 5000)")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle", type=int, default=30)
    a = ap.parse_args()
    from hakai import dist, mesh
    from hakai.solver import Solver, step_group
    out = {"mode": a.mode, "lib": os.environ.get("HAKAI_LIB", "this tree"), "steps": a.steps, "rounds": a.rounds,
           "settle": a.settle}
    if a.mode == "c3":
        m = mesh.config_c3(max(1, 5000 // a.layers))
        svs = [Solver(m)]
        out["nodes"] = [m.nNode]

        def step(t, n):
            svs[0].step(t, n)
    else:
        svs = []
        for r in range(2):
            loc, diag, iface = dist.bar_slab(20, 20, 2 * a.layers, r, 2, mesh.steel_ductile(),
                                             lambda z, L: 5e4 * z / L)
            sv = Solver(loc, diag_M=diag)
            sv.set_element_offset(loc.global_element_offset)
            sv.comm_init_local(r, 2, 4343)
            sv.set_interface(*iface)
            sv.set_tuning("group_serial", 1)
            svs.append(sv)
        out["nodes"] = [sv.model.nNode for sv in svs]

        def step(t, n):
            step_group(svs, t, n)

    def sync():
        for sv in svs:
            sv.sync()

    t, out["off"] = timed(step, sync, 1, a.settle, a.rounds, a.steps)
    for sv in svs:
        sv.history_enable([], stride=1, capacity=64)
    t, out["stride1"] = timed(step, sync, t, a.settle, a.rounds, a.steps)
    out["history_ms_per_step"] = out["stride1"]["median_ms"] - out["off"]["median_ms"]
    for sv in svs:
        sv.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
