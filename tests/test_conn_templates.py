"""Connectivity templates, planned and decoded on the CPU (tools/conn_plan_check.cpp).

The planner (csrc/hakai_conn_plan.hpp) stores, per element, the base node conn[e][0] and the id of the
element's pattern of eight offsets conn[e][k] - conn[e][0], packed into one 32-bit record, plus the table
of distinct patterns; the element kernel then reads 4 B per element instead of 32. The check program
builds the padded connectivity as hakai_upload_model hands it over, plans it and decodes every (element,
lane) as the kernel does: the result must be the input, entry for entry, with the pattern counts the
mesh implies. Above the cap of 256 patterns there is no compressed form. The GPU side is
tests/test_gpu_conn_templates.py.
"""
import functools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "conn_plan_check")


@functools.lru_cache(maxsize=None)
def _plan(args):
    assert os.path.exists(EXE), "tools/_build/conn_plan_check not built (__graft_entry__.build())"
    out = subprocess.run([EXE] + args.split(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"], r
    return r


def _round_trip(r, patterns):
    assert r["compressed"] == 1 and r["mismatch"] == 0, r
    assert r["patterns"] == patterns, r
    assert r["bytes"] == 4 * r["nEp"] + 32 * patterns and r["plain_bytes"] == 32 * r["nEp"], r


def test_small_bar_less_than_one_batch():
    """3x2x4: 24 elements and 8 padding elements in the one batch -- the lattice pattern and the
    padding's pattern of zeros."""
    r = _plan("bar 3 2 4")
    assert (r["nE"], r["nEp"]) == (24, 32)
    _round_trip(r, 2)


def test_33_elements_two_batches():
    """nE = 33: the second batch holds one element and 31 padding elements."""
    r = _plan("bar 1 1 33")
    assert (r["nE"], r["nEp"]) == (33, 64)
    _round_trip(r, 2)


def test_two_regions_border_inside_a_batch():
    """3x3x5 (45 elements) then 4x2x3: different y and z strides, and the second region starts in the
    middle of the second batch."""
    r = _plan("bar 3 3 5 4 2 3")
    assert (r["nE"], r["nEp"]) == (69, 96)
    _round_trip(r, 3)


@pytest.mark.parametrize("seed", [7, 8])
def test_permuted_node_order_negative_offsets(seed):
    """Each region's local node order permuted: the base is no longer the element's smallest node, so
    some offsets are negative."""
    _round_trip(_plan(f"bar 3 3 5 4 2 3 --perm {seed}"), 3)


def test_cap_and_one_more():
    """Exactly 256 distinct patterns compress; 257 report the plain form, with the plain bytes."""
    _round_trip(_plan("distinct 256"), 256)
    r = _plan("distinct 257")
    assert r["compressed"] == 0 and r["patterns"] == 0 and r["bytes"] == r["plain_bytes"], r
    _round_trip(_plan("distinct 8 --cap 8"), 8)
    assert _plan("distinct 9 --cap 8")["compressed"] == 0


def test_shuffled_connectivity_is_plain():
    r = _plan("bar 6 5 20 --shuffle 3")
    assert r["compressed"] == 0 and r["bytes"] == 32 * r["nEp"], r


def test_c3_one_pattern_eight_megabytes():
    """The bench workload: 2 M elements, whole batches, one pattern -- 8.0 MB per launch against 64.0."""
    r = _plan("bar 20 20 5000")
    assert r["nEp"] == 2_000_000 and 1 <= r["patterns"] <= 2, r
    _round_trip(r, r["patterns"])
    assert r["bytes"] == 8_000_000 + 32 * r["patterns"] and r["plain_bytes"] == 64_000_000, r
