"""Cost of the external loads (hakai_set_loads) on the GPU: C3 (2 M hex, fused element mode) step
time with gravity + pressure on one end face, with gravity alone and without loads; Tensile5e
microseconds per step with one concentrated load against none. Settling steps first, the variants
alternated in one process, 48 untimed steps after every change (the step graphs are captured again);
host clock around a synchronised block of steps. One JSON line per timed block, to stdout and to the
file given as the first argument (profiles/loads_cost.json holds a run).

    python tools/bench_loads.py [out.jsonl]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hakai-fem_amd"))
import numpy as np
from hakai import mesh
from hakai.model import Loads
from hakai.solver import Solver

out = open(sys.argv[1] if len(sys.argv) > 1 else os.devnull, "w")

def emit(**kw):
    s = json.dumps(kw)
    print(s, flush=True)
    out.write(s + "\n"); out.flush()

def timed(sv, t0, n):
    sv.sync()
    a = time.perf_counter()
    sv.step(t0, n)
    sv.sync()
    return time.perf_counter() - a

def alternate(name, sv, variants, settle, n, reps, t=1):
    sv.step(t, settle); t += settle
    for r in range(reps):
        for vname, apply in variants:
            apply(sv)
            sv.step(t, 48); t += 48          # graphs captured again after the change, caches settled
            e = timed(sv, t, n); t += n
            emit(case=name, variant=vname, rep=r, steps=n, ms_per_step=e / n * 1e3, graph_steps=sv.graph_steps())

# (a) C3, 2 M hex, fused element mode (the benchmark's)
m = mesh.config_c3(v_end=5e5)
nx, ny, nz = 20, 20, 5000
top = np.arange((nz - 1) * nx * ny, nz * nx * ny) + 1
ld = Loads(grav_accel=[[0.0, 0.0, -9.81e3]], press_elem=top, press_face=np.full(len(top), 2), press_value=np.full(len(top), -50.0))
with Solver(m) as sv:
    alternate("C3", sv, [("none", lambda s: s.clear_loads()), ("gravity+end_pressure", lambda s: s.set_loads(ld)),
                         ("gravity", lambda s: s.set_loads(Loads(grav_accel=[[0.0, 0.0, -9.81e3]])))], 100, 300, 4)
del m
# (c) Tensile5e, launch-bound
m = mesh.tensile5e_model()
one = Loads(cload_dof=[3 * m.nNode], cload_value=[10.0])
with Solver(m) as sv:
    alternate("Tensile5e", sv, [("none", lambda s: s.clear_loads()), ("one_cload", lambda s: s.set_loads(one))], 200, 2000, 5)
