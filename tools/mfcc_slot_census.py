#!/usr/bin/env python3
"""Issue-slot census of an MFCC kernel's frame-pair loop (CPU: hipcc cross-compiles to ISA without a GPU).

DESIGN.md 4.1 ("Where the floor is"): a wavefront of the MFCC kernels issues one instruction per ~6.8 cycles with four
wavefronts on the SIMD, whatever the instruction's kind, so every slot counts -- arithmetic or not.  This tool compiles
kws_mfcc.hip the way tools/isa_hazard_lint.py does (its ISA reader is reused), finds the loop that holds the packed transform
and prints that loop's instructions by kind: plain VALU, packed, DPP, select, compare, move, lane ops, LDS, vector memory,
scratch, scalar, branch, s_nop, s_waitcnt.  Counts are static: both sides of every branch inside the loop are counted once.

The loops come from the compiler's own block comments (`in Loop: Header=BBn_m Depth=d`).  The PAIR loop is the innermost loop
whose body holds a whole transform (its first exchange's eight hand-written `ds_read_b64`); the number of transform copies in
the body is printed with it -- two when the compiler duplicated the transform into both sides of a uniform branch (the level
equalisation's) or unrolled the pair loop into the chunk loop.  The CHUNK loop is the outermost loop around the pair loop.

Usage:  python tools/mfcc_slot_census.py [kernel-name-fragment ...] [-DMACRO ...]
        (default kernels: kws_mfcc_i16_kernel kws_mfcc_i16_ref_kernel)
"""
from __future__ import annotations

import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import isa_hazard_lint as lint  # noqa: E402

SRC = os.path.join(lint.CSRC, "kws_mfcc.hip")
KINDS = ["valu", "packed", "dpp", "select", "compare", "move", "lane", "trans", "lds", "vmem", "scratch", "scalar", "branch", "s_nop",
         "s_waitcnt"]
_LOOP = re.compile(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)")
_PARENT = re.compile(r"Parent Loop (BB\d+_\d+) Depth=(\d+)")
_HEADER = re.compile(r"This (?:Inner )?Loop Header: Depth=(\d+)")


def kind_of(ins) -> str:
    op = ins.op
    if op == "s_nop":
        return "s_nop"
    if op == "s_waitcnt":
        return "s_waitcnt"
    if op.startswith(("s_cbranch", "s_branch", "s_setpc", "s_endpgm")):
        return "branch"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("scratch_"):
        return "scratch"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "buffer_", "flat_")):
        return "vmem"
    if op.startswith(("v_readlane", "v_readfirstlane", "v_writelane", "v_permlane", "v_mbcnt")):
        return "lane"
    if lint.is_dpp(ins):
        return "dpp"
    if op.startswith("v_cndmask"):
        return "select"
    if op.startswith("v_cmp"):
        return "compare"
    if op.startswith(("v_mov_b32", "v_mov_b64", "v_accvgpr")):
        return "move"
    if op.startswith("v_pk_"):
        return "packed"
    if op.startswith(("v_log_", "v_exp_", "v_rcp_", "v_rsq_", "v_sqrt_", "v_sin_", "v_cos_")):
        return "trans"
    return "valu"


def blocks_of(isa_path: str):
    """{function: [(loop path, [Ins])]} -- the basic blocks of every function in layout order; loop path = headers of the loops
    a block lies in, outermost first (() outside every loop)."""
    funcs, cur = {}, None  # function -> [[label, [comments], [Ins]]]
    with open(isa_path) as f:
        for n, raw in enumerate(f, 1):
            code, _, comment = raw.partition(";")
            m = re.match(r"^\.L(BB\d+_\d+):", raw) or re.match(r"^; %(bb\.\d+):", raw)
            if m:
                if cur is not None:
                    cur.append([m.group(1), [raw], []])
                continue
            m = re.match(r"^([A-Za-z_][\w$.]*):", raw)
            if m and not m.group(1).startswith("__hip_cuid"):
                cur = funcs.setdefault(m.group(1), [["entry", [], []]])
                continue
            if cur is None:
                continue
            t = code.strip()
            if not t:
                if comment:
                    cur[-1][1].append(comment)
            elif t.startswith((".section", ".end_amdhsa_kernel")):
                cur = None
            elif raw.startswith(("\t", " ")) and re.match(r"^[a-z]", t):
                cur[-1][2].append(lint.Ins(n, t))
    out = {}
    for name, blocks in funcs.items():
        chains = {}
        for label, comments, _ in blocks:
            text = " ".join(comments)
            if _HEADER.search(text):
                chains[label] = tuple(h for h, _ in _PARENT.findall(text)) + (label,)
        res = []
        for label, comments, body in blocks:
            m = _LOOP.search(" ".join(comments))
            res.append((chains.get(label, chains.get(m.group(1), ()) if m else ()), body))
        if any(b for _, b in res):
            out[name] = res
    return out


def _is_transform_gather(ins) -> bool:
    return ins.op == "ds_read_b64" and "offset:448" in ins.text


def census(isa_path: str, kernel: str):
    """Counts for the kernel whose mangled name contains `kernel` (followed by a letter E, the end of an Itanium name part):
    {"pair": {kind: n}, "chunk": {kind: n}, "transforms": transforms in the pair loop's body, "pair_loop": header,
     "chunk_loop": header, "vgpr_count": n, "scratch_in_chunk_loop": [instruction text]}."""
    blocks = None
    for name, b in blocks_of(isa_path).items():
        if re.search(r"\d+" + re.escape(kernel) + "E", name):
            blocks, mangled = b, name
    if blocks is None:
        raise KeyError(f"no kernel {kernel} in {isa_path}")
    loops = {}
    for path, body in blocks:
        for h in path:
            loops.setdefault(h, []).extend(body)
    holding = {h: sum(_is_transform_gather(i) for i in body) for h, body in loops.items()}
    depth = {h: max(len(p[:p.index(h) + 1]) for p, _ in blocks if h in p) for h in loops}
    cands = [h for h in loops if holding[h] >= 1]
    if not cands:
        raise ValueError(f"{kernel}: no loop holds a transform")
    pair = max(cands, key=lambda h: depth[h])
    chunk = min((h for h in cands if any(h in p and pair in p for p, _ in blocks)), key=lambda h: depth[h])

    def count(body):
        c = dict.fromkeys(KINDS, 0)
        for i in body:
            c[kind_of(i)] += 1
        return c
    vgpr = None
    with open(isa_path) as f:
        text = f.read()
    m = re.search(r"\.name:\s+" + re.escape(mangled) + r"\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", text)
    if m:
        vgpr = int(m.group(1))
    return {"kernel": mangled, "pair": count(loops[pair]), "chunk": count(loops[chunk]), "transforms": holding[pair],
            "pair_loop": pair, "chunk_loop": chunk, "vgpr_count": vgpr,
            "scratch_in_chunk_loop": [i.text for i in loops[chunk] if i.op.startswith("scratch_")]}


def main(argv):
    flags = [a for a in argv if a.startswith("-")]
    kernels = [a for a in argv if not a.startswith("-")] or ["kws_mfcc_i16_kernel", "kws_mfcc_i16_ref_kernel"]
    isa = lint.compile_to_isa(SRC, tuple(flags))
    res = [census(isa, k) for k in kernels]
    print(f"ISA {isa}")
    print(f"{'pair loop, static':28s}" + "".join(f"{k[-22:]:>24s}" for k in kernels))
    for kind in KINDS:
        print(f"{kind:28s}" + "".join(f"{r['pair'][kind]:24d}" for r in res))
    print(f"{'total':28s}" + "".join(f"{sum(r['pair'].values()):24d}" for r in res))
    for r, k in zip(res, kernels):
        print(f"{k}: pair loop {r['pair_loop']} ({r['transforms']} transform copies in its body), chunk loop {r['chunk_loop']}, "
              f"{r['vgpr_count']} VGPRs, {len(r['scratch_in_chunk_loop'])} scratch instruction(s) in the chunk loop")
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
