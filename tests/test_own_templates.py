"""Template form of the owner-assembly entry lists, replayed on the CPU (tools/own_plan_check.cpp).

On a lattice mesh super-batches that meet the section's layer pattern at the same phase hold the
same entries up to a constant added to their node and row targets. The template form
(csrc/hakai_own_plan.hpp) stores each distinct relative pass once, gives every super-batch a 16-byte
header with its bases, and computes the LDS slot as node mod P instead of storing the allocator's.
The replay executes it as the kernel does -- header, relative target, derived slot -- next to the
plain form, and both must equal the reference's serial sum bit for bit. Meshes without a valid P
keep the plain form. The GPU side is tests/test_gpu_own_templates.py.
"""
import functools
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "own_plan_check")

C3 = "20 20 5000 --G 512"  # the bench workload's plan


@functools.lru_cache(maxsize=None)
def _plan(args):
    assert os.path.exists(EXE), "tools/_build/own_plan_check not built (__graft_entry__.build())"
    out = subprocess.run([EXE] + args.split(), capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return json.loads(out.stdout.strip().splitlines()[-1])


def _replayed(r):
    assert r["ok"] and r["planned"], r
    assert r["mismatch"] == 0 and r["double_fin"] == 0, r


@pytest.mark.parametrize("args", ["20 20 300", C3, "3 3 200 --G 8", "5 1 1 --G 1", "20 20 300 --exact 1"])
def test_template_form_replay_bitexact(args):
    r = _plan(args)
    _replayed(r)
    assert r["template_form"] == 1, r
    assert 1 <= r["templates"] <= r["passes"], r
    assert r["entries_stored"] <= r["entries"], r
    assert r["slots"] <= r["template_slots"] <= r["slot_cap"], r  # P holds at least the sums open at once


@pytest.mark.parametrize("args", ["3 3 200 --G 8 --shuffle 11", "100 100 40 --G 32"])
def test_no_slot_rule_keeps_plain_form(args):
    """Shuffled numbering and row bands of a wide section admit no node mod P: plain form, replayed
    as before."""
    r = _plan(args)
    _replayed(r)
    assert r["template_form"] == 0 and r["templates"] == 0, r
    assert r["entries_stored"] == r["entries"], r


def test_c3_plan_stores_a_tenth_at_most():
    """The C3 plan repeats with the 25 phases of a 20x20 section against 64-element super-batches,
    plus the head and tail passes of each block run: 99 distinct passes, 17 341 stored entries
    against 5 606 008 listed (0.31 %)."""
    r = _plan(C3)
    print(r)
    assert r["template_form"] == 1
    assert r["entries_stored"] <= 0.10 * r["entries"], r


def test_selftest_one_lane_apart_is_another_template():
    """The tool's selftest: headers at their field extremes, node mod P by conditional subtraction,
    and a template store in which two passes that differ in one lane id do not share a template."""
    assert os.path.exists(EXE), "tools/_build/own_plan_check not built (__graft_entry__.build())"
    out = subprocess.run([EXE, "--selftest"], capture_output=True, text=True, timeout=30)
    assert out.returncode == 0, out.stdout + out.stderr
    r = json.loads(out.stdout.strip().splitlines()[-1])
    assert r["ok"] and r["bad"] == 0 and r["selftest"] > 0, r
