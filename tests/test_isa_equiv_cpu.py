"""tools/isa_kernel_equiv.py on synthetic assembly text (no compiler, no GPU): what it must call equal, and what it must report."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_spec = importlib.util.spec_from_file_location("isa_kernel_equiv", os.path.join(ROOT, "tools", "isa_kernel_equiv.py"))
equiv = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(equiv)


def _kernel(name, fn, vgpr=60, mid="v_add_f32_e32 v1, v1, v2", first_block=3):
    """one kernel as hipcc -S writes it: labels numbered by function index `fn`, blocks from `first_block` on"""
    a, b = first_block, first_block + 4
    return f"""\t.section\t.text.{name},"axG",@progbits,{name},comdat
\t.globl\t{name} ; -- Begin function {name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\ts_load_dwordx4 s[8:11], s[0:1], 0x8
\ts_cbranch_execz .LBB{fn}_{b}
.LBB{fn}_{a}: ; =>This Inner Loop Header: Depth=1
\t{mid}
\ts_cbranch_scc1 .LBB{fn}_{a}
.LBB{fn}_{b}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 9216
\t\t.amdhsa_next_free_vgpr {vgpr}
\t\t.amdhsa_next_free_sgpr 20
\t.end_amdhsa_kernel
\t.section\t.text.{name},"axG",@progbits,{name},comdat
.Lfunc_end{fn}:
\t.size\t{name}, .Lfunc_end{fn}-{name}
                                        ; -- End function
\t.set {name}.num_vgpr, {vgpr}
"""


def _file(kernels, cuid):
    head = '\t.amdgcn_target "amdgcn-amd-amdhsa--gfx950"\n\t.amdhsa_code_object_version 6\n'
    tail = f'\t.type\t__hip_cuid_{cuid},@object\n__hip_cuid_{cuid}:\n\t.byte\t0\n\t.ident\t"clang {cuid}"\n'
    return head + "".join(kernels) + tail


OLD = _file([_kernel("_Z5alphav", 0), _kernel("_Z4betav", 1), _kernel("_Z5gammav", 2)], "aaaa")


def test_label_numbering_and_function_order_do_not_matter():
    new = [_file([_kernel("_Z5gammav", 0, first_block=7), _kernel("_Z5alphav", 1, first_block=1)], "bbbb"), _file([_kernel("_Z4betav", 0, first_block=12)], "cccc")]
    report, bad = equiv.compare([OLD], new)
    assert bad == 0 and report == ["3 kernels old, 3 kernels new: 0 on one side only, 0 different"]
    assert set(equiv.kernels(OLD)) == {"_Z5alphav", "_Z4betav", "_Z5gammav"}


def test_a_changed_instruction_is_reported_with_its_kernel():
    new = _file([_kernel("_Z5alphav", 0), _kernel("_Z4betav", 1, mid="v_add_f32_e32 v1, v1, v3"), _kernel("_Z5gammav", 2)], "aaaa")
    report, bad = equiv.compare([OLD], [new])
    assert bad == 1 and len(report) == 2
    assert report[0].startswith("differs: _Z4betav (body) line 4:") and "v1, v1, v2" in report[0] and "v1, v1, v3" in report[0]
    assert report[-1] == "3 kernels old, 3 kernels new: 0 on one side only, 1 different"


def test_a_branch_to_another_block_is_a_difference():
    """renumbering must keep WHICH label an instruction names: the loop's back edge pointed at the exit block instead"""
    new = OLD.replace("s_cbranch_scc1 .LBB2_3", "s_cbranch_scc1 .LBB2_7")
    assert new != OLD
    report, bad = equiv.compare([OLD], [new])
    assert bad == 1 and report[0].startswith("differs: _Z5gammav (body)")


def test_a_changed_register_count_is_reported():
    new = _file([_kernel("_Z5alphav", 0, vgpr=64), _kernel("_Z4betav", 1), _kernel("_Z5gammav", 2)], "aaaa")
    report, bad = equiv.compare([OLD], [new])
    assert bad == 1 and len(report) == 2
    assert report[0].startswith("differs: _Z5alphav (descriptor) line 2:") and ".amdhsa_next_free_vgpr 60" in report[0] and ".amdhsa_next_free_vgpr 64" in report[0]


def test_a_kernel_missing_on_one_side_is_reported():
    new = _file([_kernel("_Z5alphav", 0), _kernel("_Z5gammav", 1)], "aaaa")
    report, bad = equiv.compare([OLD], [new])
    assert bad == 1 and report == ["only in old: _Z4betav", "3 kernels old, 2 kernels new: 1 on one side only, 0 different"]
    report, bad = equiv.compare([new], [OLD])
    assert bad == 1 and report[0] == "only in new: _Z4betav"
    twice, bad = equiv.compare([OLD], [OLD, new])
    assert bad == 2 and twice[:2] == ["twice in new: _Z5alphav", "twice in new: _Z5gammav"]


def test_command_line_exit_status(tmp_path):
    import subprocess
    import sys
    (tmp_path / "a.s").write_text(OLD)
    (tmp_path / "b.s").write_text(OLD.replace(".amdhsa_next_free_sgpr 20", ".amdhsa_next_free_sgpr 24", 1))
    tool = os.path.join(ROOT, "tools", "isa_kernel_equiv.py")
    same = subprocess.run([sys.executable, tool, "--old", str(tmp_path / "a.s"), "--new", str(tmp_path / "a.s")], capture_output=True, text=True)
    assert same.returncode == 0 and same.stdout.strip() == "3 kernels old, 3 kernels new: 0 on one side only, 0 different"
    other = subprocess.run([sys.executable, tool, "--old", str(tmp_path / "a.s"), "--new", str(tmp_path / "b.s")], capture_output=True, text=True)
    assert other.returncode == 1 and "differs: _Z5alphav (descriptor)" in other.stdout
