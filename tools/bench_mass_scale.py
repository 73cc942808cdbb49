#!/usr/bin/env python3
"""Cost of selective mass scaling (hakai_mass_scale) next to hakai_stable_dt on the same context.

    python tools/bench_mass_scale.py c3                                        # C3 (2 M hex)
    python tools/bench_mass_scale.py c3 --out profiles/mass_scale_cost.json    # merge the result into a file

After settling steps it times, in one process and on one context, on a drained stream: `calls` calls
of stable_dt() (two launches, the result copy, the sync), then `calls` calls of mass_scale() with a
target that scales about `fraction` of the elements -- three launches (need, finish, gather), the
80-byte result copy and the sync; the first call, which allocates the scratch, copies the uploaded
mass and changes it, is timed apart, the later calls change nothing but do all the work. Prints one
JSON line with both and the gather's bytes."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

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
    ap.add_argument("--settle", type=int, default=0, help="settling steps (0: 30 for c3, 200 for tensile5e)")
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--fraction", type=float, default=0.1, help="share of the elements the target scales")
    ap.add_argument("--out", default=None, help="JSON file to merge the result into, under the mode's name")
    a = ap.parse_args()
    from hakai import mesh
    from hakai.solver import Solver
    c3 = a.mode == "c3"
    m = mesh.config_c3(max(1, 5000 // a.layers)) if c3 else mesh.tensile5e_model()
    settle = a.settle or (30 if c3 else 200)
    out = {"mode": a.mode, "elements": m.nElement, "nodes": m.nNode, "settle": settle, "calls": a.calls}
    with Solver(m) as sv:
        sv.step(1, settle)
        sv.sync()
        out["stable_dt_first_call_ms"] = wall_ms(sv.stable_dt, 1)["min_ms"]
        out["stable_dt"] = wall_ms(sv.stable_dt, a.calls)
        safe = sv.stable_dt(per_element=True)["dt_safe_elem"]
        target = 0.9 * float(np.quantile(safe[np.isfinite(safe)], a.fraction))
        out["dt_target"] = target
        first = {}
        t0 = time.perf_counter()
        first = sv.mass_scale(dt_target=target)
        out["mass_scale_first_call_ms"] = (time.perf_counter() - t0) * 1e3
        out["first_result"] = first
        out["mass_scale"] = wall_ms(lambda: sv.mass_scale(dt_target=target), a.calls)
        out["stable_dt_scaled"] = wall_ms(sv.stable_dt, a.calls)
        again = sv.mass_scale(dt_target=target)
        assert again["n_changed"] == 0 and again["mass_added"] == first["mass_added"]
    # k_mass_gather: per node the uploaded mass, the new mass, two CSR bounds; per incidence its row and the
    # element's added mass (8 B each way for added in k_mass_need on top of k_stable_dt's reads)
    out["gather_bytes"] = m.nNode * (8 + 8 + 4) + 8 * m.nElement * (4 + 8)
    out["mass_scale_over_stable_dt"] = out["mass_scale"]["median_ms"] / out["stable_dt"]["median_ms"]
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
