"""tools/kernel_diff.py on hand-written assembly: what it must ignore (comments, debug directives,
branch-label numbers, the kernel's own symbol) and what it must report (an instruction, an
.amdhsa_ directive, a kernel that only one side has)."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_diff", os.path.join(ROOT, "tools", "kernel_diff.py"))
kernel_diff = importlib.util.module_from_spec(spec)
spec.loader.exec_module(kernel_diff)


def asm(symbol, fn, vgprs=8, add="v_add_f32_e32 v1, v0, v0", note="", debug=""):
    return f"""\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"
\t.section\t.text.{symbol},"axG",@progbits,{symbol},comdat
\t.globl\t{symbol} ; -- Begin function {symbol}
\t.p2align\t8
\t.type\t{symbol},@function
{symbol}: ; @{symbol}
; %bb.0:
{debug}\ts_load_dwordx2 s[2:3], s[0:1], 0x0 {note}
\ts_cbranch_execz .LBB{fn}_2
; %bb.1:
\t{add}
\t;;#ASMSTART
\ts_nop 2
\t;;#ASMEND
.LBB{fn}_2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {symbol}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_accum_offset 8
\t.end_amdhsa_kernel
\t.section\t.text.{symbol},"axG",@progbits,{symbol},comdat
.Lfunc_end{fn}:
\t.size\t{symbol}, .Lfunc_end{fn}-{symbol}
\t.set {symbol}.num_vgpr, {vgprs}
; NumVgprs: {vgprs}
"""


def run(tmp_path, capsys, old, new, *args):
    a, b = tmp_path / "old.s", tmp_path / "new.s"
    a.write_text(old)
    b.write_text(new)
    status = kernel_diff.main([str(a), str(b), *args])
    return status, capsys.readouterr().out.splitlines()


def test_equal_up_to_names_labels_comments_and_debug_lines(tmp_path, capsys):
    old = asm("first", 0) + asm("coop128_kernel", 1)
    new = asm("coop_kernel_w128", 0, note="; a comment", debug="\t.loc\t1 20 5\n\t.cfi_startproc\n") + asm("first", 3)
    status, out = run(tmp_path, capsys, old, new, "--rename", "coop128_kernel=coop_kernel_w128")
    assert status == 0
    assert out == ["identical: first", "identical: coop_kernel_w128"]


def test_a_changed_instruction_is_reported(tmp_path, capsys):
    old = asm("first", 0) + asm("second", 1)
    new = asm("first", 0) + asm("second", 1, add="v_add_f32_e32 v1, v0, v2")
    status, out = run(tmp_path, capsys, old, new)
    assert status == 1
    assert out[0] == "identical: first"
    assert out[1] == ("differs: second (first difference at instruction 2: "
                      "'v_add_f32_e32 v1, v0, v0' | 'v_add_f32_e32 v1, v0, v2')")


def test_a_changed_directive_is_reported(tmp_path, capsys):
    status, out = run(tmp_path, capsys, asm("first", 0), asm("first", 0, vgprs=9))
    assert status == 1
    assert out == ["differs: first (first difference at directive 1: "
                   "'.amdhsa_next_free_vgpr 8' | '.amdhsa_next_free_vgpr 9')"]


def test_a_kernel_on_one_side_only_fails(tmp_path, capsys):
    status, out = run(tmp_path, capsys, asm("first", 0) + asm("gone", 1), asm("first", 0) + asm("added", 1))
    assert status == 1
    assert out[0] == "identical: first"
    assert out[1].startswith("only in ") and out[1].endswith("old.s: gone")
    assert out[2].startswith("only in ") and out[2].endswith("new.s: added")
