#!/usr/bin/env python3
"""Cost of the stable-time-step diagnostic (hakai_stable_dt) next to one step of the same context.

    python tools/bench_stable_dt.py c3                 # C3 (2 M hex)
    python tools/bench_stable_dt.py tensile5e          # the 5-element deck
    python tools/bench_stable_dt.py c3 --out profiles/stable_dt_cost.json   # merge the result into a file

After settling steps it times, in one process and on one context: `rounds` x `steps` steps (wall
time per step), then `calls` calls of stable_dt() and `calls` with the per-element arrays requested.
The call is synchronous -- two launches, the 56-byte result copy (plus 16 B per element when the
arrays are asked for) and the stream sync -- so its wall time on a drained stream is what a driver
pays per record; the first call, which allocates the scratch, is timed apart. Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hakai-fem_amd"))


def wall_ms(fn, n):
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ms.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=("c3", "tensile5e"))
    ap.add_argument("--layers", type=int, default=5000, help="z layers of the C3 bar (5000: 2 M hex)")
    ap.add_argument("--steps", type=int, default=0, help="steps per timed round (0: 200 for c3, 4000 for tensile5e)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--settle", type=int, default=0, help="settling steps (0: 30 for c3, 200 for tensile5e)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--out", default=None, help="JSON file to merge the result into, under the mode's name")
    a = ap.parse_args()
    from hakai import mesh
    from hakai.solver import Solver
    c3 = a.mode == "c3"
    m = mesh.config_c3(max(1, 5000 // a.layers)) if c3 else mesh.tensile5e_model()
    steps = a.steps or (200 if c3 else 4000)
    settle = a.settle or (30 if c3 else 200)
    out = {"mode": a.mode, "elements": m.nElement, "nodes": m.nNode, "steps": steps, "rounds": a.rounds,
           "settle": settle, "calls": a.calls}
    with Solver(m) as sv:
        sv.step(1, settle)
        sv.sync()
        t = 1 + settle
        ms = []
        for _ in range(a.rounds):
            t0 = time.perf_counter()
            sv.step(t, steps)
            sv.sync()
            ms.append((time.perf_counter() - t0) / steps * 1e3)
            t += steps
        out["step"] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "all_ms": ms}
        out["first_call_ms"] = wall_ms(sv.stable_dt, 1)["min_ms"]
        out["call"] = wall_ms(sv.stable_dt, a.calls)
        out["first_call_per_element_ms"] = wall_ms(lambda: sv.stable_dt(per_element=True), 1)["min_ms"]
        out["call_per_element"] = wall_ms(lambda: sv.stable_dt(per_element=True), a.calls)
        out["result"] = sv.stable_dt()
        out["d_time"] = m.dt
    out["call_over_step"] = out["call"]["median_ms"] / out["step"]["median_ms"]
    print(json.dumps(out), flush=True)
    if a.out:
        doc = {}
        if os.path.exists(a.out):
            with open(a.out) as fh:
                doc = json.load(fh)
        doc[a.mode] = out
        with open(a.out, "w") as fh:
            json.dump(doc, fh, indent=1)
            fh.write("\n")


if __name__ == "__main__":
    main()
