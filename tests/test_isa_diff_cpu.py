"""tools/isa_diff.py on short synthetic listings (no GPU, no compiler): what it calls the same, what it calls different, and
when a missing kernel is accepted."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_diff  # noqa: E402


def kernel(name, fn_no, operand="v1", vgprs=12, comment="first build"):
    """One kernel as the compiler lists it: body with a local branch target, then its descriptor."""
    return f"""\t.text
\t.globl\t{name}
\t.p2align\t8
\t.type\t{name},@function
{name}:                                 ; @{name}
; %bb.0:                                ; {comment}
\ts_load_dwordx2 s[0:1], s[4:5], 0x0
\tv_mov_b32_e32 v1, 0                   ; {comment}
.LBB{fn_no}_1:                          ; =>This Inner Loop Header: Depth=1
\tv_add_f32_e32 v0, v0, {operand}
\ts_cbranch_scc1 .LBB{fn_no}_1
; %bb.2:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.p2align\t6, 0x0
\t.amdhsa_kernel {name}
\t\t.amdhsa_group_segment_fixed_size 0
\t\t.amdhsa_next_free_vgpr {vgprs}
\t\t.amdhsa_next_free_sgpr 8
\t.end_amdhsa_kernel
\t.text
.Lfunc_end{fn_no}:
\t.size\t{name}, .Lfunc_end{fn_no}-{name}
                                        ; -- End function
"""


def write(tmp_path, name, text):
    p = tmp_path / name
    p.write_text(text)
    return str(p)


def run(capsys, *argv):
    rc = isa_diff.main(list(argv))
    return rc, capsys.readouterr().out


def test_equal_up_to_label_numbers_and_comments_is_same(tmp_path, capsys):
    a = write(tmp_path, "a.s", kernel("k_one", 0) + kernel("k_two", 1))
    # the same kernels in the other order: other label numbers, other comments, other spacing
    b = write(tmp_path, "b.s", (kernel("k_two", 0, comment="second build") + kernel("k_one", 1, comment="second build")).replace("\ts_endpgm", "\ts_endpgm   "))
    rc, out = run(capsys, a, b)
    assert rc == 0, out
    assert out.count("same") >= 2 and "differs" not in out and "MISSING" not in out


def test_one_changed_operand_differs_and_names_the_kernel(tmp_path, capsys):
    a = write(tmp_path, "a.s", kernel("k_one", 0) + kernel("k_two", 1))
    b = write(tmp_path, "b.s", kernel("k_one", 0) + kernel("k_two", 1, operand="v2"))
    rc, out = run(capsys, a, b)
    assert rc == 1
    lines = out.splitlines()
    assert [ln for ln in lines if ln.startswith("differs")] == [ln for ln in lines if "k_two" in ln] and "instructions" in out
    assert any(ln.startswith("same") and "k_one" in ln for ln in lines)
    # the descriptor counts too: same instructions, one more register
    c = write(tmp_path, "c.s", kernel("k_one", 0, vgprs=13) + kernel("k_two", 1))
    rc, out = run(capsys, a, c)
    assert rc == 1
    assert any(ln.startswith("differs") and "k_one" in ln and "descriptor" in ln for ln in out.splitlines())


def test_a_missing_kernel_is_reported_and_accepted_only_when_named(tmp_path, capsys):
    a = write(tmp_path, "a.s", kernel("k_one", 0) + kernel("k_two", 1))
    b = write(tmp_path, "b.s", kernel("k_one", 0))
    rc, out = run(capsys, a, b)
    assert rc == 1
    assert any(ln.startswith("MISSING") and "k_two" in ln for ln in out.splitlines())
    rc, out = run(capsys, a, b, "--allow-missing", "k_one")   # naming another kernel does not help
    assert rc == 1
    rc, out = run(capsys, a, b, "--allow-missing", "k_two")
    assert rc == 0, out
    assert "k_two" in out and "MISSING" not in out
    rc, out = run(capsys, b, a, "--allow-missing", "k_two")   # either side
    assert rc == 0, out
    # where the kernel went: the other unit's listing holds it unchanged
    moved = write(tmp_path, "moved.s", kernel("k_other", 0) + kernel("k_two", 1, comment="another unit"))
    rc, out = run(capsys, a, moved, "--allow-missing", "k_one", "--allow-missing", "k_other")
    assert rc == 0 and any(ln.startswith("same") and "k_two" in ln for ln in out.splitlines()), out
