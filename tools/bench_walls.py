"""Cost of the rigid walls (hakai_set_walls) on the GPU: C3 (2 M hex, fused element mode) step time
without loads or walls, with gravity, with gravity plus one floor on all nodes, and with gravity plus
a floor on a 400-node list (the mask stream); Tensile5e microseconds per step in graph mode with one
wall against none. Settling steps first, the variants alternated in one process, 48 untimed steps
after every change (the step graphs are captured again); host clock around a synchronised block of
steps. One JSON line per timed block, to stdout and to the file given as the first argument
(profiles/walls_cost.json holds a run).

    python tools/bench_walls.py [out.jsonl]"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hakai-fem_amd"))
import numpy as np
from hakai import mesh
from hakai.model import Loads, Walls
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

# (a) C3, 2 M hex, fused element mode (the benchmark's); the floor lies in the clamped plane z = 0,
# so the perturbed nodes below it touch it and the others only evaluate the gap
m = mesh.config_c3(v_end=5e5)
grav = Loads(grav_accel=[[0.0, 0.0, -9.81e3]])
floor = dict(origin=[[0.0, 0.0, 0.0]], normal=[[0.0, 0.0, 1.0]], damping=[0.1], friction=[0.3])
some = mesh.plane_nodes(20, 20, 0)[:400]

def both(walls):
    def apply(s):
        s.set_loads(grav)
        s.set_walls(walls)
    return apply

def neither(s):
    s.clear_loads()
    s.clear_walls()

def gravity(s):
    s.clear_walls()
    s.set_loads(grav)

with Solver(m) as sv:
    alternate("C3", sv, [("none", neither), ("gravity", gravity), ("gravity+floor_all_nodes", both(Walls(**floor))),
                         ("gravity+floor_400_nodes", both(Walls(nodes=[some], **floor)))], 100, 300, 4)
del m
# (b) Tensile5e, launch-bound, graph mode
m = mesh.tensile5e_model()
lo = m.coordmat.min(axis=0)
wall = Walls(origin=[lo], normal=[[0.0, 0.0, 1.0]], friction=[0.2])
with Solver(m) as sv:
    alternate("Tensile5e", sv, [("none", lambda s: s.clear_walls()), ("one_wall", lambda s: s.set_walls(wall))], 200, 2000, 5)
