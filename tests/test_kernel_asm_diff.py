"""tools/kernel_asm_diff.py compares device assembly per kernel (CPU, short synthetic assembly text)."""
import io
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

import kernel_asm_diff  # noqa: E402


def _kernel(sym, fn, lb, body):
    """One kernel as the compiler writes it: directives, the symbol, labelled blocks, the descriptor."""
    return "\n".join([
        "\t.text", f"\t.globl\t{sym}", "\t.p2align\t8", f"\t.type\t{sym},@function",
        f"{sym}:                                 ; @{sym}",
        "; %bb.0:",
        "\ts_load_dwordx2 s[0:1], s[4:5], 0x0",
        "\ts_waitcnt lgkmcnt(0)",
        f"\ts_cbranch_scc1 .LBB{fn}_{lb + 1}",
        f".LBB{fn}_{lb}:                                ; =>This Inner Loop Header: Depth=1",
        *body,
        f"\ts_cbranch_vccnz .LBB{fn}_{lb}                  ; comment {fn}",
        f".LBB{fn}_{lb + 1}:",
        "\ts_endpgm",
        f".Lfunc_end{fn}:",
        f"\t.size\t{sym}, .Lfunc_end{fn}-{sym}",
        f"\t.amdhsa_kernel {sym}", "\t\t.amdhsa_next_free_vgpr 8", "\t.end_amdhsa_kernel", ""])


ADD = ["\tv_add_f64 v[0:1], v[0:1], v[2:3]", "\tglobal_store_dwordx2 v4, v[0:1], s[0:1]"]
OLD_BIN = "_ZN12_GLOBAL__N_18k_ct_binENS_6StepInEPKi"
NEW_BIN = "_ZN12_GLOBAL__N_18k_ct_binEN3hkc2ck6StepInEPKi"
OLD_BOX = "_ZN12_GLOBAL__N_112k_xr_boxflipEPyi"


def _compare(old, new):
    out = io.StringIO()
    recs, bad = kernel_asm_diff.compare(kernel_asm_diff.kernels(old), kernel_asm_diff.kernels(new), out=out)
    return recs, bad, out.getvalue()


def _check_base_names():
    assert kernel_asm_diff.base_name(OLD_BIN) == kernel_asm_diff.base_name(NEW_BIN) == "k_ct_bin"
    assert kernel_asm_diff.base_name("_ZN2hk4k_bcENS_6BCArgsE") == "k_bc"
    a = kernel_asm_diff.base_name("_ZN2hk14k_element_pipeILb1ELi3EEEvNS_8ElemArgsE")
    b = kernel_asm_diff.base_name("_ZN2hk14k_element_pipeILb0ELi3EEEvNS_8ElemArgsE")
    assert a.startswith("k_element_pipe<") and a != b  # instantiations stay apart


def _check_same_kernel_under_a_renamed_symbol_and_renumbered_labels():
    old = _kernel(OLD_BOX, 0, 1, ADD) + _kernel(OLD_BIN, 1, 4, ADD)
    new = _kernel(NEW_BIN, 0, 7, ADD)  # another file, another namespace, other label numbers
    new2 = _kernel(OLD_BOX, 3, 2, ADD)
    recs, bad, _ = _compare(old, new + new2)
    assert bad == 0 and set(recs) == {"k_ct_bin", "k_xr_boxflip"}
    assert all(r["result"] == "same" and r["old"] == r["new"] == 7 for r in recs.values())


def _check_a_differing_instruction_is_reported():
    mul = [ADD[0].replace("v_add_f64", "v_mul_f64"), ADD[1]]
    recs, bad, text = _compare(_kernel(OLD_BIN, 0, 1, ADD), _kernel(NEW_BIN, 0, 1, mul))
    assert bad == 1 and recs["k_ct_bin"]["result"] == "differs" and recs["k_ct_bin"]["old"] == recs["k_ct_bin"]["new"]
    assert any(ln.startswith("-v_add_f64") for ln in recs["k_ct_bin"]["diff"])
    assert any(ln.startswith("+v_mul_f64") for ln in recs["k_ct_bin"]["diff"])
    assert "v_mul_f64" in text
    # a branch to another block is a difference too, renumbering or not
    swapped = _kernel(NEW_BIN, 0, 1, ADD).replace("s_cbranch_vccnz .LBB0_1", "s_cbranch_vccnz .LBB0_2")
    assert _compare(_kernel(OLD_BIN, 0, 1, ADD), swapped)[1] == 1


def _check_a_kernel_on_one_side_only_is_reported():
    old = _kernel(OLD_BOX, 0, 1, ADD) + _kernel(OLD_BIN, 1, 4, ADD)
    recs, bad, _ = _compare(old, _kernel(NEW_BIN, 0, 1, ADD))
    assert bad == 1 and recs["k_xr_boxflip"] == {"old": 7, "new": None, "result": "only old"}
    recs, bad, _ = _compare(_kernel(NEW_BIN, 0, 1, ADD), old)
    assert bad == 1 and recs["k_xr_boxflip"]["result"] == "only new" and recs["k_ct_bin"]["result"] == "same"


def test_compare_synthetic_kernels():
    _check_base_names()
    _check_same_kernel_under_a_renamed_symbol_and_renumbered_labels()
    _check_a_differing_instruction_is_reported()
    _check_a_kernel_on_one_side_only_is_reported()
