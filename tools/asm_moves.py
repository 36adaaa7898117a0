#!/usr/bin/env python3
"""Register moves of ONE kernel in a gfx950 device assembly file, by source line: every v_mov_b32 / v_mov_b64 / v_pk_mov_b32 / v_accvgpr_* whose source is an inline constant, a literal or
another VGPR (not an SGPR: that is a broadcast the lanes need), counted per .loc line.  Build the assembly with line tables:
  hipcc <the Makefile's HIPFLAGS> -gline-tables-only --cuda-device-only -S csrc/rtx_kernels.hip -o file.s
usage: asm_moves.py file.s <substring of the mangled kernel name> [first-last instruction, as tools/asm_loops.py numbers them]"""
import collections, re, sys
name = sys.argv[2]
lo, hi = (int(x) for x in sys.argv[3].split("-")) if len(sys.argv) > 3 else (0, 1 << 30)
files, on, n, loc = {}, False, 0, ("?", 0)
by_line, valu, kinds = collections.Counter(), 0, collections.Counter()
for l in open(sys.argv[1]):
    m = re.match(r'\s+\.file\s+(\d+)\s+"([^"]*)"(?:\s+"([^"]*)")?', l)
    if m:
        files[m.group(1)] = (m.group(3) or m.group(2)).split("/")[-1]
        continue
    if re.match(r"^_Z\w*:", l):
        on = name in l.split(":")[0]
        continue
    if not on:
        continue
    if l.startswith(".Lfunc_end"):
        break
    m = re.match(r"\s+\.loc\s+(\d+)\s+(\d+)", l)
    if m:
        loc = (files.get(m.group(1), m.group(1)), int(m.group(2)))
        continue
    m = re.match(r"^\s+([a-z]\w+)\s*(.*)", l)
    if not m or l.strip().startswith((".", ";")):
        continue
    op, args = m.group(1), m.group(2).split(";")[0]
    if lo <= n <= hi and op.startswith("v_"):
        valu += 1
        if op.startswith(("v_mov_b32", "v_mov_b64", "v_pk_mov_b32", "v_accvgpr")):
            src = [a.strip() for a in args.split(",")][1:]
            if src and not any(s.startswith(("s", "vcc", "exec", "ttmp", "m0")) for s in src):
                kind = "v" if src[0].startswith(("v", "a")) else "const"
                by_line[loc] += 1; kinds[(loc, kind)] += 1
    n += 1
print(f"{valu} VALU in range, {sum(by_line.values())} moves from a constant or a VGPR")
print("| source line | moves | from a constant | from a VGPR |\n|---|---|---|---|")
for k, c in sorted(by_line.items(), key=lambda kv: (-kv[1], kv[0])):
    print(f"| {k[0]}:{k[1]} | {c} | {kinds[(k, 'const')]} | {kinds[(k, 'v')]} |")
