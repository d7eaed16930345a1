#!/usr/bin/env python3
"""Instruction accounting of the flat table walks from gfx950 assembly listings.

  hipcc <unit flags of csrc/Makefile> -S --cuda-device-only kernels_msm.hip -o g1.s      (and kernels_msm_g2.hip -o g2.s)
  python3 profiles/f29_scan_accounting.py parent:g1_parent.s parent:g2_parent.s new:g1.s new:g2.s

One line per (label, kernel) for k_msm_flat and k_msm_flat_redo of either field.  The "addition loop" is every basic block that lies
inside a loop (between a label and a backward branch to it) and holds at least 100 v_mad_u64_u32: the straight-line code of the
mixed addition, without the first addition from infinity's neighbours outside the loop and without the conversion of the result (in
the redo kernels the inline doubling of the same-x case lies in the loop and counts).  Columns: instructions in those blocks, of which multiply-adds
(v_mad_u64_u32), 64-bit adds (v_lshl_add_u64, which is how the compiler adds two 64-bit registers, and v_add_co / v_addc pairs
counted once), 64-bit shifts (v_lshrrev_b64), s_nop; then the kernel's VGPRs, AGPRs, scratch bytes per lane and waves per SIMD from
its descriptor comments.  A kernel marked * closes its loop with an indirect jump (the body is too long for a relative branch); its
line counts every block of the kernel with at least 100 multiply-adds, the conversion of the result included.
"""
import re
import sys

KERNELS = ("k_msm_flat", "k_msm_flat_redo")


def kernels(text):
    """symbol -> (lines of the body, resource comments)"""
    out = {}
    lines = text.split("\n")
    i = 0
    while i < len(lines):
        m = re.match(r"^(_ZN3spp\w+):\s*(;.*)?$", lines[i])
        if m:
            j = i + 1
            while j < len(lines) and "s_endpgm" not in lines[j]:
                j += 1
            k = j
            res = {}
            while k < len(lines) and k < j + 80:
                for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
                                 ("occ", r"; Occupancy: (\d+)")):
                    mm = re.match(pat, lines[k])
                    if mm and key not in res:
                        res[key] = int(mm.group(1))
                k += 1
            out[m.group(1)] = (lines[i + 1:j], res)
            i = j
        i += 1
    return out


def loop_blocks(body, whole=False):
    """opcode lists of the basic blocks that lie inside a loop (whole: of all blocks)"""
    blocks = [("", [], [])]                      # label, opcodes, branch targets
    for line in body:
        s = line.strip()
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            blocks.append((m.group(1), [], []))
        elif s and not s.startswith((".", ";")) and not s.split()[0].endswith(":"):
            blocks[-1][1].append(s.split()[0])
            if s.startswith(("s_cbranch", "s_branch")):
                blocks[-1][2].append(s.split()[1])
    index = {b[0]: n for n, b in enumerate(blocks)}
    inside = set()
    for n, (_, _, targets) in enumerate(blocks):
        for t in targets:
            if t in index and index[t] <= n:
                inside.update(range(index[t], n + 1))
    if whole:
        inside = set(range(len(blocks)))
    return [blocks[n][1] for n in sorted(inside)]


def pretty(sym):
    for name in sorted(KERNELS, key=len, reverse=True):
        tag = "%d%sI" % (len(name), name)
        if tag in sym:
            field = "Fq2" if "Fp2" in sym or "Fq2" in sym else "Fq"
            return "%s<%s>" % (name, field)
    return None


def main():
    print("%-8s %-24s %6s %6s %6s %6s %6s %5s %5s %8s %5s" % ("commit", "kernel", "instr", "mad64", "add64", "shr64", "s_nop", "VGPR", "AGPR", "scratch", "waves"))
    for arg in sys.argv[1:]:
        label, path = arg.split(":", 1)
        for sym, (body, res) in sorted(kernels(open(path).read()).items()):
            name = pretty(sym)
            if not name:
                continue
            tot = mad = add = shr = nop = 0
            chosen = [b for b in loop_blocks(body) if b.count("v_mad_u64_u32") >= 100]
            if not chosen:   # a loop too long for a relative branch closes through s_setpc_b64: every large block of the kernel instead
                chosen = [b for b in loop_blocks(body + ["s_branch .LBB_all"], whole=True) if b.count("v_mad_u64_u32") >= 100]
                name += " *"
            for b in chosen:
                tot += len(b)
                mad += b.count("v_mad_u64_u32")
                add += b.count("v_lshl_add_u64") + sum(1 for op in b if op.startswith("v_addc_co_u32"))
                shr += b.count("v_lshrrev_b64")
                nop += b.count("s_nop")
            print("%-8s %-24s %6d %6d %6d %6d %6d %5s %5s %8s %5s" % (label, name, tot, mad, add, shr, nop, res.get("vgpr"), res.get("agpr"),
                                                                   res.get("scratch"), res.get("occ")))


if __name__ == "__main__":
    main()
