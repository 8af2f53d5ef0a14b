#!/usr/bin/env python3
"""Do two hipcc -S listings hold the same kernels?  tools/isa_diff.py <old.s> <new.s> [--demangle]

For every kernel symbol (.amdhsa_kernel) of either listing: whether its instruction lines (comments and directives
stripped, labels kept) and its .amdhsa_* descriptor lines (registers, LDS, scratch, ...) are equal.  For a kernel
that differs: the instruction counts, whether the mnemonic sequences agree (then only operands differ, e.g. register
names), and otherwise the mnemonics whose counts differ.  Ends with the totals; exit status 1 unless every kernel of
both listings is identical.  The check for a refactor that is meant to leave the generated code alone."""
import re
import shutil
import subprocess
import sys
from collections import Counter


def parse(path):
    """{kernel symbol: (instruction lines, descriptor lines)}"""
    lines = open(path).read().split("\n")
    desc, k = {}, 0
    while k < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[k])
        if m:
            d = []
            k += 1
            while not lines[k].strip().startswith(".end_amdhsa_kernel"):
                s = lines[k].split(";")[0].split()
                if s and s[0].startswith(".amdhsa_"):
                    d.append(" ".join(s))
                k += 1
            desc[m.group(1)] = d
        k += 1
    start = {l.split(":")[0]: k for k, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ".", ";") and ":" in l}
    out = {}
    for sym, d in desc.items():
        i = start[sym]
        ins = []
        for l in lines[i + 1 :]:
            s = l.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if not s or (s.startswith(".") and not s.endswith(":")):
                continue  # comment or directive
            # (block labels carry the function's index in the file: .LBB12_3)
            ins.append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))
        out[sym] = (ins, d)
    return out


def mnemonics(ins):
    return [s.split()[0] for s in ins if not s.endswith(":")]


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if len(args) != 2:
        sys.exit(__doc__)
    a, b = parse(args[0]), parse(args[1])
    names = {}
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt")
    if "--demangle" in sys.argv and filt:
        syms = sorted(set(a) | set(b))
        res = subprocess.run([filt], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")
        names = dict(zip(syms, res))
    show = lambda s: names.get(s, s)

    for s in sorted(set(a) - set(b)):
        print("only in", args[0] + ":", show(s))
    for s in sorted(set(b) - set(a)):
        print("only in", args[1] + ":", show(s))
    same, differ = 0, []
    for s in sorted(set(a) & set(b)):
        (ia, da), (ib, db) = a[s], b[s]
        if ia == ib and da == db:
            same += 1
            continue
        differ.append(s)
        ma, mb = mnemonics(ia), mnemonics(ib)
        print("DIFFERS", show(s))
        print("  descriptor:", "equal" if da == db else "DIFFERS")
        for x in sorted(set(da) ^ set(db)):
            print("    " + ("- " if x in da else "+ ") + x)
        print(f"  instructions: {'equal' if ia == ib else 'differ'}, {len(ma)} -> {len(mb)};",
              "mnemonic sequence", "equal" if ma == mb else "differs")
        if ma != mb:
            ca, cb = Counter(ma), Counter(mb)
            d = {m: (ca[m], cb[m]) for m in sorted(set(ca) | set(cb)) if ca[m] != cb[m]}
            if d:
                for m, (x, y) in d.items():
                    print(f"    {m:32s} {x} -> {y}")
            else:
                print("    (every mnemonic's count equal: reordered)")
    print(f"{args[1]}: {len(set(a) & set(b))} kernels in both, {same} identical, {len(differ)} differing")
    for s in differ:
        print("  differs:", show(s))
    sys.exit(0 if not differ and set(a) == set(b) else 1)


if __name__ == "__main__":
    main()
