#!/usr/bin/env python3
"""Per-kernel ISA identity of two builds of one translation unit.

    hipcc <the Makefile's CXXFLAGS [+ the unit's own flags]> -S --cuda-device-only unit.hip -o a.s      (at commit A; b.s at commit B)
    python profiles/isa_identity.py a.s b.s [a2.s b2.s ...]

For every kernel symbol: the text from its label to its .Lfunc_end plus its .amdhsa_kernel descriptor (registers, scratch, LDS),
without `;` comments and with local .L labels renamed to one token, hashed.  Prints symbol, VGPRs, scratch bytes, the two hashes
and SAME / DIFF; exit status 1 unless both files define the same kernels with equal text."""
import hashlib
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel (\S+)", txt, re.M):
        body = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(name), txt, re.M | re.S).group(1)
        desc = re.search(r"^\s*\.amdhsa_kernel %s\n(.*?)^\s*\.end_amdhsa_kernel" % re.escape(name), txt, re.M | re.S).group(1)
        norm = []
        for line in (body + desc).split("\n"):
            line = re.sub(r"\.L\w+", ".L", line.split(";")[0]).strip()
            if line:
                norm.append(line)
        field = lambda k: int(re.search(r"\.amdhsa_%s (\d+)" % k, desc).group(1))
        out[name] = (hashlib.sha256("\n".join(norm).encode()).hexdigest()[:16], field("next_free_vgpr"), field("private_segment_fixed_size"),
                     len(norm))
    return out


def main(argv):
    ok = True
    for a_path, b_path in zip(argv[0::2], argv[1::2]):
        a, b = kernels(a_path), kernels(b_path)
        print("# %s  against  %s" % (a_path, b_path))
        print("# %-100s %5s %8s %6s  %-16s  %-16s" % ("kernel", "VGPRs", "scratch", "lines", "hash A", "hash B"))
        for k in sorted(set(a) | set(b)):
            x, y = a.get(k), b.get(k)
            same = x is not None and x == y
            ok &= same
            ref = x or y
            print("%-102s %5d %8d %6d  %-16s  %-16s  %s" % (k, ref[1], ref[2], ref[3], x[0] if x else "-", y[0] if y else "-",
                                                         "SAME" if same else "DIFF"))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
