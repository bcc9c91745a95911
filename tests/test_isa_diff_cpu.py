"""profiles/isa_diff.py, the script that holds a change's gfx950 kernels against the parent's (profiles/README.md), on hand-written
assembly of a few lines: a kernel whose template parameters were renamed is matched through --rename and passes when its body is the
parent's, a changed body fails, and a kernel the change no longer has fails.  Text in, text out: no compiler, no GPU."""
import importlib.util
import os
import sys

import pytest

SCRIPT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "isa_diff.py")
OLD, NEW, OTHER = "_ZN6legion3k_aILb0EEEvPi", "_ZN6legion3k_aILNS_4ModeE0EEEvPi", "_ZN6legion3k_bEvPi"
RENAME = r"(3k_aI)Lb(\d)E=\1LNS_4ModeE\2E"


def kernel(symbol, index, add="v_add_u32_e32 v1, 1, v1", vgprs=2):
    """one kernel as hipcc --save-temps writes it: the function (its block labels carry the function's index in the unit) ..."""
    return """\t.text
\t.globl\t{s}
\t.type\t{s},@function
{s}:                                   ; @{s}
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v0, 0
.LBB{i}_1:                             ; =>This Inner Loop Header
\ts_waitcnt lgkmcnt(0)
\tglobal_load_dword v1, v0, s[0:1]
\ts_waitcnt vmcnt(0)
\t{add}
\tglobal_store_dword v0, v1, s[0:1]
\ts_cbranch_scc1 .LBB{i}_1
\ts_endpgm
.Lfunc_end{i}:
\t.size\t{s}, .Lfunc_end{i}-{s}
""".format(s=symbol, i=index, add=add), """  - .args:           []
    .group_segment_fixed_size: 0
    .name:           {s}
    .private_segment_fixed_size: 0
    .sgpr_count:     8
    .vgpr_count:     {v}
    .wavefront_size: 64
""".format(s=symbol, v=vgprs)


def unit(path, *kernels):
    """... and the unit: every function, then the metadata entries"""
    path.write_text("".join(k[0] for k in kernels) + "\t.amdgpu_metadata\namdhsa.kernels:\n" + "".join(k[1] for k in kernels) + "\t.end_amdgpu_metadata\n")
    return str(path)


@pytest.fixture(scope="module")
def isa_diff():
    spec = importlib.util.spec_from_file_location("isa_diff", SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def run(isa_diff, monkeypatch, capsys, options, parent, change):
    monkeypatch.setattr(sys, "argv", ["isa_diff.py"] + options + [parent, "--", change])
    code = isa_diff.main()
    return code, capsys.readouterr().out


def test_identical_body_under_a_renamed_symbol_passes(isa_diff, monkeypatch, capsys, tmp_path):
    parent = unit(tmp_path / "parent.s", kernel(OLD, 0))
    change = unit(tmp_path / "change.s", kernel(OTHER, 0), kernel(NEW, 3))   # another place in its unit: other block labels
    code, out = run(isa_diff, monkeypatch, capsys, ["--rename", RENAME], parent, change)
    assert code == 0, out
    assert "1 kernels in the parent, 2 in the change, 1 identical." in out, out
    assert sum("| identical |" in line for line in out.splitlines()) == 1 and sum("| new |" in line for line in out.splitlines()) == 1, out
    # without the rename the parent's kernel has no partner
    code, out = run(isa_diff, monkeypatch, capsys, [], parent, change)
    assert code == 1 and "| missing |" in out, out


def test_renames_apply_in_the_order_given(isa_diff, monkeypatch, capsys, tmp_path):
    parent = unit(tmp_path / "parent.s", kernel(OLD, 0))
    change = unit(tmp_path / "change.s", kernel(NEW, 0))
    code, out = run(isa_diff, monkeypatch, capsys, ["--rename", r"Lb0E=LX0E", "--rename", r"(3k_aI)LX(\d)E=\1LNS_4ModeE\2E"], parent, change)
    assert code == 0 and "1 identical" in out, out


@pytest.mark.parametrize("changed", [dict(add="v_add_u32_e32 v1, 2, v1"), dict(vgprs=3)], ids=["instruction", "vgpr_count"])
def test_changed_kernel_under_a_renamed_symbol_fails(isa_diff, monkeypatch, capsys, tmp_path, changed):
    parent = unit(tmp_path / "parent.s", kernel(OLD, 0))
    change = unit(tmp_path / "change.s", kernel(NEW, 0, **changed))
    code, out = run(isa_diff, monkeypatch, capsys, ["--rename", RENAME], parent, change)
    assert code == 1, out
    assert "DIFFERENT: " + ("vgpr_count" if "vgprs" in changed else "body (parent: 9 instructions)") in out, out
    assert "1 kernels in the parent, 1 in the change, 0 identical." in out, out


def test_kernel_missing_in_the_change_fails(isa_diff, monkeypatch, capsys, tmp_path):
    parent = unit(tmp_path / "parent.s", kernel(OLD, 0), kernel(OTHER, 1))
    change = unit(tmp_path / "change.s", kernel(NEW, 0))
    code, out = run(isa_diff, monkeypatch, capsys, ["--rename", RENAME], parent, change)
    assert code == 1, out
    missing = [line for line in out.splitlines() if "| missing |" in line]
    assert len(missing) == 1 and "k_b" in missing[0], out
    assert "2 kernels in the parent, 1 in the change, 1 identical." in out, out
