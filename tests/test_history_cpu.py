"""History output on the CPU: the energy balance of the record definition (history_ref) on the
oracle's trajectories, and the CSV round trip.

The balance KE - KE_seed + W_int - W_ext - W_bc of set 0 is an algebraic identity of the central
difference update: on the oracle, stepped one step at a time with exactly rounded sums, only the
rounding of the terms themselves is left. Bounds: 64 x the residual measured for each model when
the feature was specified (worst over the steps, relative to the largest energy term of the run)."""
import os

import numpy as np
import pytest

import oracle as O
from hakai import mesh
from history_ref import NF, HistoryRef, balance, prescribed_mask
from util import fast_deletion_bar, small_bar

# model, steps, the residual measured at specification
CASES = {
    "small_bar": (small_bar, 400, 7.9e-15),
    "two_body": (mesh.two_body_model, 200, 8.6e-15),
    "deletion_bar": (fast_deletion_bar, 3000, 1.3e-14),
}


def oracle_balance(m, n_steps, sets=()):
    """Steps the oracle one step at a time; returns (records (n, sets, 16), ke_seed, worst balance
    residual of set 0 relative to the run's largest energy term, deletions)."""
    o = O.Oracle(m)
    ref = HistoryRef(o.diag_M, prescribed_mask(m), sets, m.dt)
    ke_seed, _ = ref.seed(o.s["disp"], o.s["disp_pre"])
    recs, res, scale = [], [], 0.0
    for t in range(1, n_steps + 1):
        disp, Q = o.s["disp"].copy(), o.s["Q"].copy()
        o.run(t, 1)
        val, _ = ref.step(o.s["disp"], disp, Q, o.s["external_force"])
        recs.append(val)
        r, big = balance(val[0], ke_seed[0])
        res.append(abs(r))
        scale = max(scale, big)
    return np.array(recs), ke_seed, max(res) / scale, o.deletions


@pytest.fixture(scope="module")
def runs():
    return {k: oracle_balance(f(), n) for k, (f, n, _) in CASES.items()}


@pytest.mark.parametrize("name", list(CASES))
def test_energy_balance_is_rounding_level(runs, name):
    recs, ke_seed, worst, _ = runs[name]
    print(f"{name}: worst balance residual {worst:.3e} of the largest energy term")
    assert worst <= 64 * CASES[name][2]
    assert np.max(np.abs(recs[:, 0, 9])) > 0  # something moved


def test_contact_and_constraint_work_are_exercised(runs):
    assert runs["two_body"][0][-1, 0, 11] != 0.0            # W_ext: the bodies touched
    assert np.any(runs["two_body"][0][:, 0, 3:6] != 0.0)
    assert runs["small_bar"][0][-1, 0, 11] == 0.0            # no contact, no external work
    assert runs["deletion_bar"][0][-1, 0, 12] != 0.0         # W_bc: the amplitude BC pulls
    assert len(runs["deletion_bar"][3]) == 4                 # deletions


def test_sets_add_up():
    """Two disjoint sets that cover the mesh sum to set 0 (exactly rounded sums: to rounding)."""
    m = small_bar()
    half = m.nNode // 2
    recs, _, _, _ = oracle_balance(m, 20, sets=[np.arange(1, half + 1), np.arange(half + 1, m.nNode + 1)])
    tot, parts = recs[:, 0, :], recs[:, 1, :] + recs[:, 2, :]
    scale = np.abs(recs[:, 1, :]) + np.abs(recs[:, 2, :])  # (the halves' internal forces cancel in the total)
    # each value is one rounding of an exact sum; a work adds one more per step (20 steps)
    assert np.all(np.abs(tot - parts) <= (4 + 20) * 2.0 ** -53 * np.maximum.accumulate(scale, axis=0))
    assert np.any(scale[:, :3] > 0) and np.any(scale[:, 9] > 0)


def test_csv_round_trip(tmp_path):
    """A CSV written from synthetic records parses back to the same doubles."""
    from hakai.solver import read_history_csv, write_history_csv
    rng = np.random.default_rng(7)
    n, S = 9, 3
    values = rng.normal(size=(n, S, NF)) * 10.0 ** rng.integers(-300, 300, size=(n, S, NF))
    values[0, 0, 0], values[1, 1, 1], values[2, 2, 2] = 0.0, -0.0, 5e-324
    steps = np.arange(n, dtype=np.int64) * 7
    path = os.path.join(tmp_path, "history.csv")
    write_history_csv(path, ["all", "inst1", "bc1"], steps, values, 1.25e-7)
    got = read_history_csv(path)
    assert got["sets"] == ["all", "inst1", "bc1"]
    assert np.array_equal(got["steps"], steps)
    assert np.array_equal(got["values"].view(np.uint64), values.view(np.uint64))
    assert np.array_equal(got["time"], steps * 1.25e-7)
    head = open(path).readline().strip().split(",")
    assert head[:3] == ["step", "time", "all_F_int_x"] and head[-1] == "bc1_U_z" and len(head) == 2 + S * NF
