"""Rigid-wall cases shared by the CPU, reader and GPU tests -- TEST INFRASTRUCTURE ONLY.

TABLES are the amplitude tables of the load tests (two-point, multi-point, stepped, non-monotonic,
late start) in units of seconds; rigid_wall writes the deck keyword; corner_walls, many_walls and
random_state build the probe cases of tests/test_gpu_walls.py."""
import numpy as np

from hakai.model import Walls

TABLES = {"two_point": ([0.0, 1e-5], [0.0, 1.0]),
          "multi_point": ([0.0, 1e-6, 3e-6, 1e-5], [0.0, 1.0, 0.25, 2.0]),
          "stepped": ([0.0, 2e-6, 2e-6, 1e-5], [0.0, 0.0, 1.0, 1.0]),
          "non_monotonic": ([0.0, 4e-6, 2e-6, 1e-5], [1.0, -1.0, 3.0, 0.5]),
          "late_start": ([2e-6, 4e-6, 8e-6], [0.5, 1.5, -0.5])}


def rigid_wall(name, origin, normal, motion=None, **params):
    """The *Rigid Wall block of a deck: params are nset, amplitude, stiffness, scale, damping, friction."""
    head = f"*Rigid Wall, name={name}" + "".join(
        f", {k}={v if isinstance(v, str) else repr(float(v))}" for k, v in params.items())
    vals = list(origin) + list(normal) + (list(motion) if motion is not None else [])
    return head + "\n" + ", ".join(repr(float(v)) for v in vals) + "\n"


def random_state(m, seed, depth=0.02, speed=5.0, dt=1e-7):
    """disp, disp_pre (3nN): displacements of the order of `depth` and velocities of the order of `speed`."""
    rng = np.random.default_rng(seed)
    disp = rng.normal(0, depth, 3 * m.nNode)
    return disp, disp - rng.normal(0, speed, 3 * m.nNode) * dt


def centre(m):
    return m.coordmat.mean(axis=0)


def one_wall(m, **kw):
    """A plane through the mesh's centre: a random state puts about half the nodes through it."""
    args = dict(origin=[centre(m)], normal=[[0.3, -0.2, 1.0]], stiffness=[2e5], scale=[0.25], damping=[0.2],
                friction=[0.3])
    args.update(kw)
    return Walls(**args)


def corner_walls(m, **kw):
    """Three mutually oblique walls meeting in a corner at the centre: a node in the corner sums three
    contributions, in index order."""
    c = centre(m)
    args = dict(origin=[c, c, c], normal=[[1, 0.2, 0.1], [0.1, 1, 0.3], [0.2, 0.1, 1]], stiffness=[1e5, 2e5, 3e5],
                scale=[0.5, 0.25, 0.125], damping=[0.1, 0.2, 0.3], friction=[0.3, 0.2, 0.1])
    args.update(kw)
    return Walls(**args)


def many_walls(m, seed, amps=None):
    """32 walls: random planes near the centre, every third one on all nodes, the others on random node
    lists (so all 32 mask bits and the all-nodes path occur in one model)."""
    rng = np.random.default_rng(seed)
    c = centre(m)
    nodes = [np.zeros(0, np.int64) if w % 3 == 0 else rng.choice(m.nNode, max(1, m.nNode // 3), replace=False) + 1
             for w in range(32)]
    nodes[31] = np.arange(1, m.nNode + 1)                # the highest bit on every node, through a list
    amps = amps or []
    return Walls(origin=c + rng.normal(0, 0.01, (32, 3)), normal=rng.normal(0, 1, (32, 3)),
                 motion=rng.normal(0, 0.05, (32, 3)), amp=rng.integers(-1, len(amps), 32),
                 stiffness=rng.uniform(0, 1e5, 32), scale=rng.uniform(0, 0.5, 32), damping=rng.uniform(0, 0.3, 32),
                 friction=rng.uniform(0, 0.5, 32), nodes=nodes, amps=amps)
