"""The wavefront-priority schedule of the persistent DS-CNN kernels, checked in the device assembly (CPU: hipcc cross-compiles).

`s_setprio` is a scalar instruction: it ignores EXEC and the wavefront runs it whichever lanes are active.  A raise that is
meant for one half of the workgroup (wavefronts 4-7, or 0-3) therefore has to sit behind a SCALAR branch.  Under a condition
the compiler cannot prove wave-uniform it becomes `s_and_saveexec` + an unconditional `s_setprio`: every wavefront is raised,
which is no change at all -- silently, with every result still right (csrc/kws_dscnn_stages.h, "Wavefront priority";
DESIGN 4.2).  The rule held here, for every `s_setprio` with a non-zero operand in kws_dscnn.hip:

* walking back from it to the head of its basic block there is no write of EXEC;
* the block is entered only through `s_cbranch_scc*` / `s_cbranch_vcc*`: the instruction it falls through from is one (or an
  unconditional `s_branch`, which does not fall through), and so is every branch to its label.

The listing comes from the reader behind tests/test_isa_hazards.py (tools/isa_hazard_lint.py: one compile per source state,
cached); that reader flattens a function into one instruction list and drops the labels, so the basic blocks are read here."""
import os
import re
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "tools"))
import isa_hazard_lint as lint  # noqa: E402

CSRC = os.path.join(REPO, "keyword-spotting_amd", "csrc")
pytestmark = pytest.mark.skipif(not os.path.exists(lint.HIPCC), reason="hipcc not installed")

SCALAR_COND = ("s_cbranch_scc0", "s_cbranch_scc1", "s_cbranch_vccz", "s_cbranch_vccnz")
_LABEL = re.compile(r"^([.\w$]+):")


def listing(path):
    """{function: [(line number, label or None, instruction text or None)]} in text order."""
    funcs, cur = {}, None
    with open(path) as f:
        for n, raw in enumerate(f, 1):
            line = raw.split(";", 1)[0].rstrip()
            if not line:
                continue
            if not line.startswith(("\t", " ")):
                m = _LABEL.match(line)
                if not m:
                    continue
                if m.group(1).startswith(".L"):
                    if cur is not None:
                        cur.append((n, m.group(1), None))
                else:
                    cur = funcs.setdefault(m.group(1), [])
                continue
            t = line.strip()
            if t.startswith(".section"):
                cur = None
            elif cur is not None and re.match(r"^[a-z]", t):
                cur.append((n, None, t))
    return {k: v for k, v in funcs.items() if any(t for _, _, t in v)}


def writes_exec(text):
    op = text.split()[0]
    if "saveexec" in op or op.startswith("v_cmpx"):
        return True
    dst = text.split(None, 1)[1].split(",")[0].strip() if " " in text else ""
    return op.startswith("s_") and dst in ("exec", "exec_lo", "exec_hi")


def priority_findings(items):
    """What is wrong with the non-zero s_setprio of one function: [(line, message)]; and how many it has."""
    branches_to = {}
    for n, _, t in items:
        if t and t.startswith(("s_cbranch", "s_branch")):
            branches_to.setdefault(t.split()[-1], []).append((n, t.split()[0]))
    findings, raises = [], 0
    for i, (n, _, t) in enumerate(items):
        if not t or not t.startswith("s_setprio") or int(t.split()[1], 0) == 0:
            continue
        raises += 1
        j = i - 1
        while j >= 0:
            _, label, prev = items[j]
            if label is not None:
                # the head of the block: who falls into it, who jumps to it
                k = j - 1
                while k >= 0 and items[k][2] is None:
                    k -= 1
                above = items[k][2].split()[0] if k >= 0 else "s_branch"
                if above not in SCALAR_COND + ("s_branch", "s_endpgm", "s_setpc_b64"):
                    findings.append((n, f"`{t}` is reached by falling through from `{items[k][2]}`"))
                for bn, bop in branches_to.get(label, []):
                    if bop not in SCALAR_COND:
                        findings.append((n, f"`{t}` is reached by `{bop}` (line {bn})"))
                break
            if prev.startswith("s_cbranch") or prev.startswith("s_branch"):
                if prev.split()[0] not in SCALAR_COND:
                    findings.append((n, f"`{t}` follows `{prev}`"))
                break
            if writes_exec(prev):
                findings.append((n, f"`{t}` follows a write of EXEC, `{prev}`, in its block"))
                break
            j -= 1
        else:
            findings.append((n, f"`{t}` is not behind any branch"))
    return findings, raises


@pytest.fixture(scope="module")
def dscnn_isa():
    return listing(lint.compile_to_isa(os.path.join(CSRC, "kws_dscnn.hip")))


def test_the_rule_reports_the_exec_mask_lowering():
    """The two lowerings of the guides, as text: the scalar branch passes, the exec mask and the bare raise are reported."""
    good = [(1, None, "s_cmp_lt_u32 s4, 4"), (2, None, "s_cbranch_scc1 .LBB0_2"), (3, None, "s_setprio 1"), (4, ".LBB0_2", None), (5, None, "s_nop 0")]
    bad = [(1, None, "v_cmp_lt_u32_e32 vcc, 0xff, v0"), (2, None, "s_and_saveexec_b64 s[0:1], vcc"), (3, None, "s_setprio 1"),
           (4, None, "s_or_b64 exec, exec, s[0:1]")]
    skipped = [(1, None, "s_and_saveexec_b64 s[0:1], vcc"), (2, None, "s_cbranch_execz .LBB0_2"), (3, None, "s_setprio 1"), (4, ".LBB0_2", None)]
    target = [(1, None, "s_cbranch_execnz .LBB0_3"), (2, None, "s_branch .LBB0_4"), (3, ".LBB0_3", None), (4, None, "s_setprio 2"), (5, ".LBB0_4", None)]
    assert priority_findings(good) == ([], 1)
    assert priority_findings([(1, None, "s_setprio 0")]) == ([], 0)
    for case in (bad, skipped, target, [(1, None, "s_setprio 3")]):
        f, n = priority_findings(case)
        assert n == 1 and len(f) == 1, case


def test_every_priority_raise_sits_behind_a_scalar_branch(dscnn_isa):
    total, flat = 0, []
    for name, items in dscnn_isa.items():
        f, n = priority_findings(items)
        total += n
        flat += [(name[:70], line, msg) for line, msg in f]
    assert total >= 1, "kws_dscnn.hip holds no s_setprio with a non-zero operand: the schedule has been compiled out"
    assert not flat, flat[:5]


def test_only_the_persistent_kernels_change_priority(dscnn_isa):
    """kws_dscnn_fwd_kernel<MODE, DIAG, PRECONV, STREAM, CLUSTER, PERSIST, SCAN>: the one-clip, streaming, cluster and
    pre-convolved instantiations hold no s_setprio at all; every persistent one raises and ends each block at 0."""
    seen = 0
    for name, items in dscnn_isa.items():
        m = re.search(r"kws_dscnn_fwd_kernelILi(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)ELb(\d)E", name)
        if not m:
            continue
        seen += 1
        persist = m.group(6) == "1"
        prios = [int(t.split()[1], 0) for _, _, t in items if t and t.startswith("s_setprio")]
        if persist:
            assert any(prios) and prios[-1] == 0 and set(prios) <= {0, 1, 2}, (name, prios)
        else:
            assert not prios, (name, prios)
    assert seen >= 20
