#!/usr/bin/env python3
"""Did a source change alter any kernel's machine code?  kernel_isa_diff.py OLD.s NEW.s [NEW2.s ...]

The inputs are device assembly files, one per translation unit:
    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only -S FILE.hip -o FILE.s
Each file is cut into per-kernel pieces: the text from the kernel's symbol label to the end of its
.amdhsa_kernel block (instructions and kernel descriptor: registers, LDS, scratch).  The pieces of
OLD are compared, as text, with the union of the pieces of the NEW files -- so a file may be split
into several, or kernels moved between files.  Two things that are not code are left out of the
comparison: lines that name __hip_cuid_ (a hash of the translation unit), and the ordinal of the
function inside its file, which the assembler's local labels carry (.LBB7_12 -> .LBB_12; runs of
blanks count as one, since the comment column moves with the width of that number).
Exit status 1 when a kernel is only on one side or a piece differs (the first such piece is shown)."""
import difflib
import re
import sys

LABEL = re.compile(r"^([^\s:]+):")
KERNEL = re.compile(r"^\s*\.amdhsa_kernel\s+(\S+)")
ORDINAL = re.compile(r"(BB|JTI)\d+(_\d+)")


def pieces(path):
    lines = open(path).read().split("\n")
    label = {}                                   # symbol -> line of its label (the last one seen)
    out, name = {}, None
    for i, line in enumerate(lines):
        m = LABEL.match(line)
        if m:
            label[m.group(1)] = i
        m = KERNEL.match(line)
        if m:
            name = m.group(1)
        elif name and line.strip() == ".end_amdhsa_kernel":
            body = [" ".join(ORDINAL.sub(r"\1\2", l).split()) for l in lines[label[name]:i + 1] if "__hip_cuid_" not in l]
            out[name], name = body, None
    return out


def main(argv):
    if len(argv) < 3:
        sys.exit(__doc__)
    old, new = pieces(argv[1]), {}
    for path in argv[2:]:
        for k, v in pieces(path).items():
            if k in new:
                sys.exit("kernel %s is in more than one NEW file" % k)
            new[k] = v
    only_old, only_new = sorted(set(old) - set(new)), sorted(set(new) - set(old))
    differ = sorted(k for k in set(old) & set(new) if old[k] != new[k])
    print("kernels: %d in OLD, %d in NEW; only in OLD: %d, only in NEW: %d, pieces that differ: %d"
          % (len(old), len(new), len(only_old), len(only_new), len(differ)))
    for tag, names in (("only in OLD", only_old), ("only in NEW", only_new), ("differs", differ)):
        for k in names:
            print("  %s: %s" % (tag, k))
    if differ:
        k = differ[0]
        print("\n".join(difflib.unified_diff(old[k], new[k], "OLD " + k, "NEW " + k, lineterm="", n=3)))
    return 1 if only_old or only_new or differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
