"""The build description has one source, hakai-fem_amd/Makefile: the tools take their flags from it,
tools/variants.sh its objects, and every source under csrc/ is compiled once (CPU; `make -n` and
`make print-flags` only, nothing is compiled)."""
import glob
import os
import re
import shlex
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "hakai-fem_amd")
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_resources  # noqa: E402


def _dry(*args):
    """The commands `make -n ARGS` prints, as argument lists."""
    p = subprocess.run(["make", "-n", "-C", PKG, *args], capture_output=True, text=True, check=True)
    return [shlex.split(ln) for ln in p.stdout.splitlines() if ln.strip() and not ln.startswith("make")]


def _compiles(cmds):
    """{object: command} of the compile commands (`... -c SRC -o OBJ`)."""
    return {c[c.index("-o") + 1]: c for c in cmds if "-c" in c and "-o" in c}


def _src(cmd):
    return cmd[cmd.index("-c") + 1]


def _link(cmds, target):
    (c,) = [c for c in cmds if "-shared" in c and c[c.index("-o") + 1] == target]
    return [w for w in c if w.endswith(".o")]


def _pinned(flags):
    """The flags that decide a kernel's code: contraction (or none), optimisation, standard, atomics."""
    return sorted(f for f in flags if re.match(r"-ffp-contract=|-O|-std=|-munsafe-fp-atomics$", f))


ALL = _dry("-B")


def test_tools_take_the_makefiles_flags():
    comp = _compiles(ALL)
    srcs = sorted(glob.glob(os.path.join(PKG, "csrc", "*.hip"))) + [os.path.join(PKG, "csrc", "hakai_comm.cpp")]
    assert len(srcs) >= 10
    seen = set()
    for src in srcs:
        obj = "build/" + os.path.splitext(os.path.basename(src))[0] + ".o"
        cmd = comp[obj]
        assert _src(cmd) == os.path.relpath(src, PKG)
        got = kernel_resources.flags(src)
        assert _pinned(got) == _pinned(cmd), (src, got, cmd)
        assert "--offload-arch=gfx950" in got and "-O3" in got and "-std=c++17" in got
        seen.add(tuple(f for f in got if f.startswith("-ffp-contract")))
    # the three settings the library uses are all met: on (element), off, none (hakai_comm.cpp)
    assert seen == {("-ffp-contract=on",), ("-ffp-contract=off",), ()}
    assert "-ffp-contract=on" in kernel_resources.flags(os.path.join(PKG, "csrc", "hakai_element.hip"))


def test_every_csrc_source_is_one_object_of_the_library():
    comp = _compiles(ALL)
    objs = _link(ALL, "lib/libhakai_hip.so")
    assert len(objs) == len(set(objs)) and set(objs) == set(comp)
    by_src = {}
    for obj, cmd in comp.items():
        by_src.setdefault(_src(cmd), []).append(obj)
    csrc = {os.path.relpath(f, PKG) for ext in ("hip", "cpp") for f in glob.glob(os.path.join(PKG, "csrc", "*." + ext))}
    assert csrc <= set(by_src), csrc - set(by_src)
    assert all(len(v) == 1 for v in by_src.values()), by_src
    assert {s for s in by_src if s.startswith("csrc/")} == csrc


def test_variants_link_every_product_object_but_the_element_one():
    text = open(os.path.join(ROOT, "tools", "variants.sh")).read()
    code = "\n".join(ln for ln in text.splitlines() if not ln.lstrip().startswith("#"))
    assert 'variant NAME="$1" DEFS="$2"' in code
    # no object, source or flag of its own
    assert not re.search(r"\.o\b|\.hip\b|\.cpp\b|hipcc|-ffp-contract|--offload-arch|-O\d|-std=", code), code
    j = re.search(r"-j\s*(\d+)", code)
    assert j and int(j.group(1)) <= 16
    cmds = _dry("variant", "NAME=zz", "DEFS=-DHK_ZZ -DHK_YY=2")
    product = _link(ALL, "lib/libhakai_hip.so")
    elem = "build/hakai_element.o"
    assert elem in product
    want = ["build/variants/zz.o" if o == elem else o for o in product]
    got = _link(cmds, "lib/variants/zz.so")
    assert sorted(got) == sorted(want) and elem not in got
    vc = _compiles(cmds)["build/variants/zz.o"]
    assert _src(vc) == "csrc/hakai_element.hip" and "-DHK_ZZ" in vc and "-DHK_YY=2" in vc
    assert _pinned(vc) == _pinned(_compiles(ALL)[elem])
