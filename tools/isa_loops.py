#!/usr/bin/env python3
"""Instruction mix per innermost loop of a kernel's ISA (hipcc -S output), attributing every
instruction to the loop LLVM's comments place its basic block in ("This Loop Header: Depth=d",
"in Loop: Header=BBx_y").

Usage: python3 tools/isa_loops.py <kernel.s> [loop-header | all | blocks]   (with a header: its opcode histogram; all: every loop, not the 30 largest;
blocks: every basic block that decodes a wide node's bytes -- 40 or more v_cvt_f32_ubyte*, a block of eight of spw::visit or
spw::visit_plain -- with its loop, its v_max3 / v_min3 count and the canonicalising v_max_f32 x, x it holds)
The DirectLighting kernel's ISA: hipcc --offload-arch=gfx950 <the Makefile's flags> -S
--offload-device-only -c simplepath_amd/csrc/hip/sp_mega_direct.hip, then the lines of
sp_render_kernel<6, 4>.

Since DESIGN.md §25 a loop's header block is counted with its loop also where the header names its
parent loops first (a nested loop: the "This [Inner] Loop Header" comment is on a later line of the
label).  Tables made before that (profiles/r08/straightline/isa_loops.txt and the other rounds')
counted such a header block outside the loop: their rows of nested loops are lower, by some 30
instructions for a walk loop, and are not to be set beside rows made since."""
import collections
import re
import sys


def blocks(lines):
    cur = "top"
    lab = None  # the label whose comment lines are being read
    for l in lines:
        s = l.strip()
        if re.match(r"^\.LBB\d+_\d+:|^; %bb\.\d+:", s):
            m = re.search(r"Header=(BB\d+_\d+) Depth=(\d+)", s)
            lab = s.split(":")[0].lstrip(".").replace("LBB", "BB")
            cur = lab if re.search(r"This (Inner )?Loop Header: Depth=", s) else (m.group(1) if m else "top")
            continue
        if lab and s.startswith(";"):
            # a header inside other loops names its parents first: "=> This [Inner] Loop Header" comes
            # on a later comment line of the same label, and the header block belongs to its own loop
            if re.search(r"This (Inner )?Loop Header: Depth=", s):
                cur = lab
            continue
        if not s or s.startswith((";", ".")) or s.endswith(":"):
            continue
        lab = None
        yield cur, s.split()[0]


def visit_blocks(lines):
    cur = None
    out = []
    for l in lines:
        s = l.strip()
        if re.match(r"^\.LBB\d+_\d+:|^; %bb\.\d+:", s):
            cur = {"label": s.split(":")[0].lstrip("; ."), "loop": "-", "c": collections.Counter()}
            out.append(cur)
        if cur is not None and (s.startswith(";") or s.startswith(".LBB")):
            m = re.search(r"Header=(BB\d+_\d+)", s)
            if m and cur["loop"] == "-":
                cur["loop"] = m.group(1)
            continue
        if cur is None or not s or s.startswith(".") or s.endswith(":"):
            continue
        op, c = s.split()[0], cur["c"]
        c["n"] += 1
        for key, pre in (("valu", "v_"), ("s_nop", "s_nop"), ("ubyte", "v_cvt_f32_ubyte"), ("v_cmp", "v_cmp"), ("v_cndmask", "v_cndmask"),
                         ("max3/min3", ("v_max3_f32", "v_min3_f32")), ("max/min", ("v_max_f32", "v_min_f32")), ("scratch", "scratch_")):
            if op.startswith(pre):
                c[key] += 1
        if op.startswith("s_") and not op.startswith("s_nop"):
            c["salu"] += 1
        a = [x.strip(",") for x in s.split()[1:4]]
        if op.startswith("v_max_f32") and len(a) == 3 and a[1] == a[2]:
            c["canonicalise"] += 1
    for b in out:
        if b["c"]["ubyte"] >= 40:
            print(b["label"], "in loop", b["loop"], dict(b["c"]))


def main(path, header=None):
    lines = open(path).read().split("\n")
    if header == "blocks":
        return visit_blocks(lines)
    if header and header != "all":
        c = collections.Counter(op for loop, op in blocks(lines) if loop == header)
        for op, n in c.most_common(50):
            print(op, n)
        return
    stats = collections.defaultdict(collections.Counter)
    for loop, op in blocks(lines):
        c = stats[loop]
        c["n"] += 1
        if op.startswith("v_readlane"):
            c["readlane"] += 1
        elif op.startswith("v_writelane"):
            c["writelane"] += 1
        elif op.startswith("scratch_"):
            c["scratch"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("v_"):
            c["valu"] += 1
        if "f64" in op:
            c["f64"] += 1
        # exec-mask traffic and select plumbing
        for key, pre in (("saveexec", None), ("cbr_exec", "s_cbranch_exec"), ("s_nop", "s_nop"), ("v_cmp", "v_cmp"),
                         ("v_cndmask", "v_cndmask"), ("v_mov", "v_mov"), ("ubyte", "v_cvt_f32_ubyte")):
            if (pre is None and "saveexec" in op) or (pre is not None and op.startswith(pre)):
                c[key] += 1
        if op.startswith(("v_min_f32", "v_max_f32", "v_med3_f32")):
            c["minmax"] += 1
    for k, c in sorted(stats.items(), key=lambda x: -x[1]["n"])[:None if header == "all" else 30]:
        print(k, dict(c))


if __name__ == "__main__":
    main(*sys.argv[1:])
