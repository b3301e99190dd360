#!/usr/bin/env python3
"""Compare the kernels of two device assembly files, instruction for instruction.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S -o before.s caffe-escoin_amd/csrc/sconv_tiled.hip   (at the parent)
    hipcc <the Makefile's FLAGS> --cuda-device-only -S -o after.s  caffe-escoin_amd/csrc/sconv_tiled.hip   (at the new tree)
    tools/isa_compare.py before.s after.s

For every function symbol of either file: its instruction stream with comments and assembler directives stripped and
the labels the function defines (.LBB*, and the ones inline asm numbers with %=) renamed in order of first appearance,
so that neither the order of the functions in the file nor the compiler's block and asm numbering counts.  Prints one
line per kernel -- instruction counts and whether the streams are identical -- and exits 1 when any kernel differs or
exists in one file only.  A refactor of a kernel file that is meant to leave the device code alone proves it with
this, without a GPU.
"""
import re
import subprocess
import sys

TYPE_FN = re.compile(r"^\s*\.type\s+([^,\s]+),@function")
LABEL = re.compile(r"^([.\w$]+):")
TOKEN = re.compile(r"[.\w$]+")


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
        return dict(zip(names, out.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """symbol -> list of normalised lines (instructions and label definitions)"""
    out, sym, body = {}, None, None
    pending = None
    with open(path, errors="replace") as f:
        for raw in f:
            line = raw.split(";", 1)[0].strip()
            if not line:
                continue
            m = TYPE_FN.match(line)
            if m:
                pending = m.group(1)
                continue
            m = LABEL.match(line)
            if m and sym is None:
                if m.group(1) == pending:
                    sym, body, pending = m.group(1), [], None
                continue
            if sym is None:
                continue
            if m and m.group(1).startswith(".Lfunc_end"):
                out[sym] = body
                sym = None
                continue
            if line.startswith(".") and not m:
                continue        # assembler directive
            body.append(line)
    return {sym: renamed(body) for sym, body in out.items()}


def renamed(body):
    """the labels the function defines (.LBB*, and what inline asm names with %=), numbered by first appearance"""
    defined = {LABEL.match(l).group(1) for l in body if LABEL.match(l)}
    order = {}
    return [TOKEN.sub(lambda t: order.setdefault(t.group(0), "L%d" % len(order)) if t.group(0) in defined else t.group(0), l)
            for l in body]


def n_instr(body):
    return sum(1 for l in body if not LABEL.match(l))


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    names = demangle(sorted(set(a) | set(b)))
    bad = 0
    for sym in sorted(names, key=lambda s: names[s]):
        if sym not in a or sym not in b:
            verdict = "ONLY IN " + (sys.argv[1] if sym in a else sys.argv[2])
        elif a[sym] == b[sym]:
            verdict = "identical"
        else:
            first = next((i for i, (x, y) in enumerate(zip(a[sym], b[sym])) if x != y), min(len(a[sym]), len(b[sym])))
            verdict = "DIFFERENT (first at line %d of the stream)" % first
        bad += verdict != "identical"
        print("%-70s %6s %6s  %s" % (names[sym], n_instr(a[sym]) if sym in a else "-", n_instr(b[sym]) if sym in b else "-",
                                     verdict))
    print("%d kernels, %d differ" % (len(names), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
