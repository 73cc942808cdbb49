#!/usr/bin/env python3
"""Per-kernel comparison of gfx950 device assembly: did a change of the sources change a kernel?

    python tools/kernel_asm_diff.py --old OLD... --new NEW... [--old-flags FLAGS] [--new-flags FLAGS]
                                    [--only REGEX] [--json OUT] [--lines N]

Each OLD / NEW is a device assembly file (.s), a HIP source (compiled to device assembly with the
flags its own tree's Makefile gives its object, `make print-flags`, or with --old-flags / --new-flags
for sources no Makefile knows; no GPU needed) or a source tree (every hakai-fem_amd/csrc/*.hip in
it, and csrc/hakai_comm.cpp, whose interface kernels hipcc compiles too). The kernels of each side are collected over all its files and matched by base name (`k_...`;
a template instantiation keeps its mangled arguments), so a kernel may move between files or
namespaces. Before comparing, mangled symbols are reduced to the base name, basic-block and other
local labels are renumbered in order of appearance, and comments, blank lines and assembler
directives are dropped. It compares text and knows nothing about particular instructions.

Prints per kernel the instruction count of each side and `same`, or the first differing lines.
Exit status 1 if a kernel differs or exists on one side only."""
import argparse
import difflib
import glob
import json
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kernel_resources  # noqa: E402  (flags(): the Makefile's flags per object)

SYM = re.compile(r"_Z[A-Za-z0-9_$.]+")
LOCAL = re.compile(r"\.L[A-Za-z_$]+[0-9_]+")


def base_name(sym):
    """Kernel name of an Itanium-mangled function symbol without its namespaces:
    `_ZN12_GLOBAL__N_18k_ct_binENS_6StepInE...` -> `k_ct_bin`; a template instantiation keeps
    the mangled rest (`k_element_pipe<ILb1E...>`); anything else is returned as it is."""
    if not sym.startswith("_Z"):
        return sym
    s, names = sym[2:], []
    nested = s.startswith("N")
    if nested:
        s = s[1:]
    while True:
        m = re.match(r"(\d+)", s)
        if not m:
            break
        n = int(m.group(1))
        names.append(s[m.end():m.end() + n])
        s = s[m.end() + n:]
        if not nested:
            break
    if not names:
        return sym
    return names[-1] + (f"<{s}>" if s.startswith("I") else "")


def normalise(lines):
    """Instruction and label lines of one kernel body, symbols and local labels made comparable."""
    out, labels = [], {}

    def lab(m):
        return labels.setdefault(m.group(0), f".L{len(labels)}")

    for ln in lines:
        ln = re.split(r";|//", ln, 1)[0].strip()
        if not ln:
            continue
        if ln.startswith(".") and not re.match(r"\.L[\w$]+:", ln):
            continue  # assembler directive
        ln = SYM.sub(lambda m: base_name(m.group(0)), ln)
        ln = LOCAL.sub(lab, ln)
        out.append(re.sub(r"\s+", " ", ln))
    return out


def kernels(text):
    """{base name: normalised body} of the `k_...` functions of one assembly text."""
    out, cur, body = {}, None, []
    for ln in text.splitlines():
        m = re.match(r"([A-Za-z_$][\w$.]*):", ln)
        if m and cur is None and re.match(r"k_", base_name(m.group(1))):
            cur, body = base_name(m.group(1)), []
            continue
        if cur is None:
            continue
        if re.match(r"\.Lfunc_end\d+:", ln.strip()) or ln.strip().startswith(".end_amdhsa_kernel"):
            out[cur] = normalise(body)
            cur = None
            continue
        body.append(ln)
    if cur is not None:
        out[cur] = normalise(body)
    return out


def count(body):
    return sum(1 for ln in body if not ln.endswith(":"))


def compile_asm(src, flags=None):
    with tempfile.TemporaryDirectory() as td:
        o = os.path.join(td, "k.s")
        p = subprocess.run(["/opt/rocm/bin/hipcc", *(flags or kernel_resources.flags(src)), "-I", os.path.dirname(src),
                            "--cuda-device-only", "-S", src, "-o", o], capture_output=True, text=True)
        if p.returncode:
            sys.exit(p.stderr[-4000:])
        return open(o).read()


def side(paths, flags=None):
    ks = {}
    for p in paths:
        if os.path.isdir(p):
            files = sorted(glob.glob(os.path.join(p, "hakai-fem_amd", "csrc", "*.hip")))
            files += glob.glob(os.path.join(p, "hakai-fem_amd", "csrc", "hakai_comm.cpp"))
        else:
            files = [p]
        for f in files:
            text = open(f).read() if f.endswith(".s") else compile_asm(f, flags)
            for k, b in kernels(text).items():
                if k in ks:
                    sys.exit(f"kernel {k} twice on one side ({f})")
                ks[k] = b
    return ks


def compare(old, new, only=None, nlines=12, out=sys.stdout):
    """Prints the per-kernel report; returns (per-kernel records, number of kernels not `same`)."""
    recs, bad = {}, 0
    for k in sorted(set(old) | set(new)):
        if only and not re.search(only, k):
            continue
        a, b = old.get(k), new.get(k)
        r = {"old": count(a) if a is not None else None, "new": count(b) if b is not None else None}
        if a is None or b is None:
            r["result"] = "only old" if b is None else "only new"
        else:
            r["result"] = "same" if a == b else "differs"
        recs[k] = r
        print(f"{k:40s} {str(r['old']):>7s} {str(r['new']):>7s}  {r['result']}", file=out)
        if r["result"] != "same":
            bad += 1
        if r["result"] == "differs":
            d = [ln for ln in difflib.unified_diff(a, b, "old", "new", lineterm="", n=1)][2:]
            r["diff"] = d[:nlines]
            for ln in r["diff"]:
                print("    " + ln, file=out)
    return recs, bad


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--old-flags", help="compile flags for the OLD sources in place of their Makefile's")
    ap.add_argument("--new-flags", help="the same for the NEW sources")
    ap.add_argument("--only", help="regular expression: kernels to compare")
    ap.add_argument("--json", help="write the per-kernel records here")
    ap.add_argument("--lines", type=int, default=12, help="differing lines shown per kernel")
    a = ap.parse_args()
    recs, bad = compare(side(a.old, (a.old_flags or "").split()), side(a.new, (a.new_flags or "").split()),
                        a.only, a.lines)
    print(f"{len(recs)} kernels, {bad} not the same")
    if a.json:
        with open(a.json, "w") as f:
            json.dump({"kernels": recs, "not_same": bad}, f, indent=1)
            f.write("\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
