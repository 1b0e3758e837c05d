#!/usr/bin/env python3
"""Compare device assembly function by function, as text.

    kernel_code_diff.py OLD.s NEW.s [NEW2.s ...]

The files are what `hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S`
writes.  For every function (kernel or out-of-line device function) of OLD.s
the script takes its body from its label to its end label (a kernel's
.amdhsa_kernel block lies in between) and its entry in the amdgpu_metadata
note, renumbers the local labels relative to the function, and compares that text with the
same function's in the NEW files (a function may be in several: every copy is
compared).  Function order and label numbers are the only differences it
tolerates.  Exit status 1 if any function differs or is missing.
"""
import re
import sys

# .LBB12_7, BB12_7 (in comments), .LJTI12_0, .Lfunc_end12: numbered by the function's place in its file
PER_FUNCTION = re.compile(r"(\.L|\b)(BB|JTI|CPI|func_end|func_begin)\d+")
TMP = re.compile(r"\.Ltmp\d+")  # numbered through the file: renumbered by first use in the function

def functions(path):
    """name -> [body (a kernel's holds its .amdhsa_kernel block), metadata entry ('' for a plain function)]."""
    lines = open(path).read().split("\n")
    out = {}
    i, n = 0, len(lines)
    while i < n:
        m = re.match(r"(_Z\w+):", lines[i])
        if m and i and ".type\t" + m.group(1) + ",@function" in lines[i - 1]:
            j = i
            while not lines[j].startswith(".Lfunc_end"):
                j += 1
            out[m.group(1)] = ["\n".join(lines[i:j + 1]), ""]
            i = j
        if lines[i].startswith("  - .agpr_count:"):  # one entry of amdhsa.kernels
            j = i + 1
            while lines[j].startswith("    ") or lines[j].startswith("      "):
                j += 1
            name = next(l.split()[1] for l in lines[i:j] if l.startswith("    .name:"))
            out[name][1] = "\n".join(lines[i:j])
            i = j - 1
        i += 1
    for parts in out.values():
        labels = {}
        body = PER_FUNCTION.sub(lambda m: m.group(1) + m.group(2), parts[0])
        body = TMP.sub(lambda m: labels.setdefault(m.group(0), ".Ltmp%d" % len(labels)), body)
        parts[0] = re.sub(r"[ \t]+", " ", body)  # (the padding before a comment follows the label's width)
    return out


def main():
    old = functions(sys.argv[1])
    new = [(p, functions(p)) for p in sys.argv[2:]]
    bad = 0
    for name, parts in old.items():
        copies = [(p, f[name]) for p, f in new if name in f]
        same = bool(copies) and all(c == parts for _, c in copies)
        bad += not same
        meta = dict(re.findall(r"\.(vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size):\s+(\d+)",
                               parts[1]))
        kind = "kernel" if parts[1] else "function"
        where = ", ".join(p for p, _ in copies) or "MISSING"
        print("%-9s %-8s %s  %s  [%s]" % ("identical" if same else "DIFFERS", kind, name,
                                          " ".join("%s=%s" % kv for kv in sorted(meta.items())), where))
        if copies and not same:
            for p, c in copies:
                for what, a, b in zip(("body", "metadata"), parts, c):
                    if a != b:
                        al, bl = a.split("\n"), b.split("\n")
                        first = next((k for k, (x, y) in enumerate(zip(al, bl)) if x != y), min(len(al), len(bl)))
                        print("    %s: %s differs from line %d (%d against %d lines)" % (p, what, first, len(al), len(bl)))
    extra = sorted({n for _, f in new for n in f} - set(old))
    for name in extra:
        print("EXTRA     %s" % name)
    print("%d functions in %s, %d differ or missing, %d extra" % (len(old), sys.argv[1], bad, len(extra)))
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main())
