#!/usr/bin/env python3
"""Compare two gfx950 device listings function by function: did a source change leave the generated code alone?

A refactor of a kernel's surroundings (moving code between files, changing how the host picks an instantiation) must not
change what the compiler emits for it.  DESIGN.md 4.9 and 4.10 made that comparison by hand; this does it for every symbol.

Input: two listings from `hipcc --offload-device-only -S` (build both with the flags of tools/isa_hazard_lint.py's BASE_FLAGS;
`isa_hazard_lint.compile_to_isa(src)` makes one).  For every function symbol the tool compares

  * the instruction stream, with comments stripped, whitespace collapsed and local labels (.LBB12_3, .Ltmp7 ...) renamed in
    order of first appearance, so that the position of a kernel inside its unit does not matter;
  * for kernels, the kernel descriptor (the .amdhsa_* lines: registers, LDS, scratch, enabled user SGPRs ...)

and prints `same` or `differs` per symbol, plus the symbols that exist on one side only.  Exit code 1 on any difference or
one-sided symbol, 0 otherwise.  `--allow-missing NAME` (repeatable) accepts a symbol whose name contains NAME being absent
from either side: a kernel that moved to another translation unit is then compared from that unit's listing.

The tool compares text only; it knows nothing about particular instructions.

Usage:  python tools/isa_diff.py before.s after.s [--allow-missing kws_softmax_f32_kernel ...]
"""
from __future__ import annotations

import argparse
import re
import sys

_LOCAL = re.compile(r"\.L[\w$.]+")
_TYPE_FN = re.compile(r"^\s*\.type\s+([\w$.]+),@function")
_LABEL = re.compile(r"^([\w$.]+):")


def parse(text: str):
    """{symbol: (instructions, descriptor)}: both lists of normalised lines; descriptor is None for a non-kernel function."""
    is_fn, body, desc = set(), {}, {}
    cur = None       # instruction list being filled
    labels = None    # local label -> canonical name, per function
    cur_desc = None
    for raw in text.splitlines():
        line = raw.split(";", 1)[0].rstrip()
        if not line.strip():
            continue
        m = _TYPE_FN.match(line)
        if m:
            is_fn.add(m.group(1))
            continue
        t = " ".join(line.split())
        if t.startswith(".amdhsa_kernel "):
            cur_desc = desc.setdefault(t.split()[1], [])
            continue
        if t == ".end_amdhsa_kernel":
            cur_desc = None
            continue
        if cur_desc is not None:
            if t.startswith(".amdhsa_"):
                cur_desc.append(t)
            continue
        m = _LABEL.match(line)
        if m and m.group(1) in is_fn:
            cur, labels = body.setdefault(m.group(1), []), {}
            continue
        if cur is None:
            continue
        if t.startswith((".Lfunc_end", ".section", ".text")):
            cur = None
            continue
        if t.startswith(".") and not _LOCAL.match(t):
            continue  # directives (.p2align, .cfi ...) are not part of the stream
        cur.append(_LOCAL.sub(lambda k: labels.setdefault(k.group(0), f".L{len(labels)}"), t))
    return {name: (ins, desc.get(name)) for name, ins in body.items()}


def first_difference(a, b):
    for i, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return f"#{i}: `{x}` | `{y}`"
    return f"length {len(a)} | {len(b)}"


def compare(a: dict, b: dict, allow_missing=()):
    """(report lines, number of failures) for two parsed listings."""
    lines, bad = [], 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            side = "first" if name in a else "second"
            ok = any(n in name for n in allow_missing)
            lines.append(f"{'moved  ' if ok else 'MISSING'} {name}  (only in the {side} listing{', allowed' if ok else ''})")
            bad += not ok
            continue
        (ia, da), (ib, db) = a[name], b[name]
        what = []
        if ia != ib:
            what.append("instructions " + first_difference(ia, ib))
        if da != db:
            what.append("descriptor " + first_difference(da or [], db or []))
        lines.append(f"{'differs' if what else 'same   '} {name}" + (f"  ({'; '.join(what)})" if what else ""))
        bad += bool(what)
    return lines, bad


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("before")
    ap.add_argument("after")
    ap.add_argument("--allow-missing", action="append", default=[], metavar="NAME",
                    help="a symbol whose name contains NAME may be absent from one listing (repeatable)")
    args = ap.parse_args(argv)
    with open(args.before) as f:
        a = parse(f.read())
    with open(args.after) as f:
        b = parse(f.read())
    lines, bad = compare(a, b, args.allow_missing)
    print("\n".join(lines))
    print(f"{len(lines) - bad} of {len(lines)} symbols same or allowed" + (f", {bad} FAILED" if bad else ""))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
