#!/usr/bin/env python3
"""kernel_isa_diff.py OLD.s NEW.s [NEW2.s ...]: compares, kernel symbol by kernel symbol, the device listings
(hipcc ... --offload-device-only -S) of a translation unit before and after a change that must not alter its
kernels -- code moved between files, shared pieces folded into functions.  Per kernel: the instruction stream, the
kernel descriptor (every .amdhsa_* line) and its entry in the code object's metadata (register and spill counts,
LDS and scratch sizes, arguments).  What a move between files changes is normalised away: label numbers, comments,
file / line / ident directives and the order of the functions.  The NEW listings together must define exactly the
kernels of OLD.  Prints one line per kernel that differs, is missing or is new, then a count; exit status 1 on any."""
import re
import sys

LABEL = re.compile(r"\.L[A-Za-z_$]*\d+(?:_\d+)?\b")
DROP = re.compile(r"\s*\.(file|loc|ident|cfi_\w+)\b")


def kernels(path):
    """{symbol: (instruction lines, descriptor lines, metadata lines)}"""
    lines = open(path).read().split("\n")
    out, entry_of = {}, {}
    for i, l in enumerate(lines):
        m = re.match(r"(\w+):", l)
        if m:
            entry_of[m.group(1)] = i
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if not m:
            continue
        name = m.group(1)
        if name in out:
            sys.exit("%s: kernel %s defined twice" % (path, name))
        st = entry_of[name]
        end_kd = next(j for j in range(i, len(lines)) if ".end_amdhsa_kernel" in lines[j])
        en = next(j for j in range(end_kd, len(lines)) if lines[j].startswith(".Lfunc_end"))
        labels = {}
        body = []
        for l2 in lines[st + 1:i] + lines[end_kd + 1:en]:
            t = l2.split(";")[0].rstrip()
            if not t.strip() or DROP.match(t):
                continue
            body.append(LABEL.sub(lambda mm: labels.setdefault(mm.group(0), ".L%d" % len(labels)), t))
        out[name] = [body, [x.strip() for x in lines[i + 1:end_kd]], None]
    # metadata: the entries of amdhsa.kernels, each from "  - " to the next one
    ms = next(j for j, l in enumerate(lines) if l.startswith("amdhsa.kernels:"))
    me = next(j for j in range(ms, len(lines)) if lines[j] and not lines[j].startswith(" ") and j > ms)
    entry = []
    for l in lines[ms + 1:me] + ["  - "]:
        if l.startswith("  - ") and entry:
            name = next(re.match(r"\s*\.name:\s+(\S+)", x).group(1) for x in entry if re.match(r"\s*\.name:\s+_Z", x))
            out[name][2] = entry
            entry = []
        entry.append(l)
    return out


def first_diff(a, b):
    for n, (x, y) in enumerate(zip(a, b)):
        if x != y:
            return "line %d: %r | %r" % (n + 1, x.strip(), y.strip())
    return "%d | %d lines" % (len(a), len(b))


def main(old_path, new_paths):
    old, new = kernels(old_path), {}
    for p in new_paths:
        k = kernels(p)
        for name in k:
            if name in new:
                sys.exit("kernel %s defined in two of the new listings" % name)
        new.update(k)
    bad = 0
    for name in old:
        if name not in new:
            print("MISSING %s" % name)
            bad += 1
            continue
        what = [w + " (" + first_diff(a, b) + ")"
                for w, a, b in zip(("instructions", "descriptor", "metadata"), old[name], new[name]) if a != b]
        if what:
            print("DIFFERS %s: %s" % (name, ", ".join(what)))
            bad += 1
    extra = [name for name in new if name not in old]
    for name in extra:
        print("EXTRA   %s" % name)
    print("%d kernels before, %d after: %d of %d identical, %d extra"
          % (len(old), len(new), len(old) - bad, len(old), len(extra)))
    sys.exit(1 if bad or extra else 0)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2:])
