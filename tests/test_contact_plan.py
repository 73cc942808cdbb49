"""The contact-model plan against the oracle's own lists, on the CPU (tools/contact_plan_check.cpp, no GPU).

The planner (csrc/hakai_contact_plan.cpp contact_plan) enumerates once every contact node and
triangle that can ever appear, with the elements whose deletion adds it. The tool builds small
lattice cases, each at the smallest shape where one of the reference's surface rules can go wrong,
and walks deletion sequences: at every point the plan's live entries (the device's live() rule) must
equal the oracle's nodes_i / nodes_j as sets and its triangles as a multiset, in the oracle's literal
mode and its indexed mode. It also checks pair order, element sizes bit for bit, the initial counts,
the element -> entry CSRs, tiles and regions, box-duplicate segments, the per-rank plans of
contiguous element ranges against the one-rank plan (the ownership rule), and the argument errors'
messages. The GPU contact tests then check that the kernels execute these plans.
"""
import json
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tools", "_build", "contact_plan_check")

CASES = [
    "one_element",              # single self pair; the instance's very last face is never exterior
    "block_self",               # adders, nodes exposed by several deletions, no j-side additions of a self pair
    "two_blocks",               # two directed pairs; j-side additions only across instances; 2 and 3 ranks
    "three_blocks",             # pair enumeration order, flag 1 and 2; more duplicates than the alias table holds
    "doubled_element",          # runs of 2 and 3 equal face keys
    "contact_pair_lists",       # *Contact Pair lists: only the list length is compared
    "negative_orientation",     # winding follows the sign test
    "interior_rank_and_tiles",  # a rank without a surface element; a region of two tiles
    "argument_errors",          # four bad inputs: the message, and no plan
]
KINDS = ["pairs", "sizes", "counts", "nodes_i", "nodes_j", "tri", "csr", "tiles", "dup", "own", "errors"]


def _run(*args):
    if not os.path.exists(EXE):
        pytest.skip("tools/_build/contact_plan_check not built (__graft_entry__.build())")
    out = subprocess.run([EXE, *args], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    return out.stdout.strip().splitlines()


@pytest.mark.parametrize("case", CASES)
def test_contact_plan_matches_oracle(case):
    r = json.loads(_run("--case", case)[-1])
    assert r["ok"] and r["cases"] == 1 and r["plans"] > 0 and r["checks"] > 0, r
    for k in KINDS:
        assert r[k] == 0, (k, r)


def test_contact_plan_no_case_left_out():
    """The tool's own list is the list above, and a plain run goes through all of it."""
    assert _run("--list") == CASES
    r = json.loads(_run()[-1])
    assert r["ok"] and r["cases"] == len(CASES), r
    for k in KINDS:
        assert r[k] == 0, (k, r)
