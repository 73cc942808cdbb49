"""hakai_history_combine on the CPU (a host helper, no GPU): the ranks' partial history records added
in rank order, ((p_0 + p_1) + p_2) + ..., one rounding per addition -- against the same sum in NumPy,
bit for bit; one part is the identity; differing step lists and null pointers are refused and leave
the outputs untouched. Then the stand-alone program that drives the helper and the CSV writer at
their edges (tools/history_host_check.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import hakai
from hakai import _abi
from hakai._abi import ptr
from hakai.solver import history_combine
from util import bitwise_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "history_host_check")
I64 = ctypes.c_int64


def random_parts(rng, R, n, S):
    """Records whose order of addition matters: magnitudes over 2^-60 .. 2^60, mixed signs, some
    exact cancellations between ranks."""
    parts = []
    for r in range(R):
        v = rng.standard_normal((n, S, 16)) * np.exp2(rng.integers(-60, 61, (n, S, 16)))
        k = rng.standard_normal(S) * np.exp2(rng.integers(-60, 61, S))
        if r > 0 and n > 0:
            v[:, :, ::5] = -parts[0]["values"][:, :, ::5]  # cancels rank 0's value, then the rest adds up
        parts.append(dict(steps=np.arange(n, dtype=np.int64) * 7, values=v, ke_seed=k))
    return parts


@pytest.mark.parametrize("R,n,S", [(2, 40, 3), (3, 17, 16), (5, 1, 1), (8, 9, 4), (2, 0, 2)])
def test_combine_is_the_rank_order_sum(R, n, S):
    parts = random_parts(np.random.default_rng(100 * R + S), R, n, S)
    h = history_combine(parts)
    v, k = parts[0]["values"].copy(), parts[0]["ke_seed"].copy()
    for p in parts[1:]:
        v, k = v + p["values"], k + p["ke_seed"]
    assert np.array_equal(h["steps"], parts[0]["steps"])
    assert bitwise_equal(h["values"], v) and bitwise_equal(h["ke_seed"], k)
    assert h["F_int"].shape == (n, S, 3) and h["KE"].shape == (n, S)
    if R > 2 and n > 0:  # the order matters for these values: another order gives other bits somewhere
        w = parts[-1]["values"].copy()
        for p in parts[-2::-1]:
            w = w + p["values"]
        assert not bitwise_equal(w, v)


def test_one_part_is_the_identity():
    (p,) = random_parts(np.random.default_rng(5), 1, 12, 6)
    p["values"][3, 2, 1] = -0.0
    h = history_combine([p])
    assert np.array_equal(h["steps"], p["steps"])
    assert bitwise_equal(h["values"], p["values"]) and bitwise_equal(h["ke_seed"], p["ke_seed"])


def test_refusals_leave_the_outputs_untouched():
    L = hakai.lib()
    R, n, S = 2, 3, 2
    steps = np.tile(np.arange(n, dtype=np.int64), (R, 1))
    values = np.ones((R, n, S, 16))
    ke = np.ones((R, S))
    so, vo, ko = np.full(n, -7, np.int64), np.full((n, S, 16), -7.0), np.full(S, -7.0)

    def call(R=R, S=S, n=n, steps=steps, values=values, ke=ke, so=so, vo=vo, ko=ko):
        return L.hakai_history_combine(R, S, n, ptr(steps, I64), ptr(values), ptr(ke), ptr(so, I64), ptr(vo), ptr(ko))

    bad = steps.copy()
    bad[1, 2] = 5
    assert call(steps=bad) == _abi.HAKAI_ERR_STATE
    assert b"rank 1" in L.hakai_last_error()
    for kw in (dict(steps=None), dict(values=None), dict(ke=None), dict(so=None), dict(vo=None), dict(ko=None),
               dict(R=0), dict(S=0), dict(S=17), dict(n=-1)):
        assert call(**kw) == _abi.HAKAI_ERR_ARG, kw
    assert np.all(so == -7) and np.all(vo == -7.0) and np.all(ko == -7.0)
    with pytest.raises(ValueError):  # the Python wrapper: ranks with different record counts
        history_combine([dict(steps=steps[0], values=values[0], ke_seed=ke[0]),
                         dict(steps=steps[0, :2], values=values[0, :2], ke_seed=ke[0])])
    assert call() == 0 and np.all(vo == 2.0) and np.all(ko == 2.0) and np.array_equal(so, steps[0])


def test_host_program_at_the_edges(tmp_path):
    """Zero records, one rank, 16 sets, every refusal, the CSV read back: tools/history_host_check."""
    if not os.path.exists(EXE):
        pytest.skip("tools/_build/history_host_check not built (__graft_entry__.build())")
    r = subprocess.run([EXE, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "history_host_check: OK" in r.stdout, (r.stdout[-2000:], r.stderr[-2000:])
    assert os.listdir(tmp_path) == []
