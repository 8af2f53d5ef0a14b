#!/usr/bin/env python3
"""Where does a kernel wait for its global loads?  tools/isa_waits.py <listing.s> [kernel-name-substring ...]

For every kernel of a hipcc -S listing (or those whose demangled name holds one of the substrings): its register, LDS
and scratch figures from the metadata, then one line per basic block with the block's events in program order:
  Ln   n global/buffer loads issued in a row        Sn   n global/buffer stores in a row
  w(N) s_waitcnt vmcnt(N)                           -> L  a branch to label L (c: conditional)
Blocks that are the target of a backward branch are marked LOOP.  vmcnt retires in order, so a w(N) with N below the
number of loads the block issued before it waits for some of those; w(0) drains the queue."""
import re
import shutil
import subprocess
import sys


def kernels(path):
    lines = open(path).read().split("\n")
    meta, cur = {}, None
    for l in lines:
        m = re.match(r"\s+(?:- )?\.(\w+):\s+(\S+)", l)
        if m:
            k, v = m.groups()
            if k == "group_segment_fixed_size":
                cur = {"lds": v}
            elif cur is not None:
                if k == "name":
                    meta[v] = cur
                elif k == "private_segment_fixed_size":
                    cur["scratch"] = v
                elif k in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "agpr_count"):
                    cur[k] = v
    start = {l.split(":")[0]: k for k, l in enumerate(lines) if l[:1] not in ("", "\t", " ", ".", ";") and ":" in l}
    out = {}
    for sym in meta:
        if sym not in start:
            continue
        body = []
        for l in lines[start[sym] + 1 :]:
            s = l.split(";")[0].strip()
            if s.startswith(".Lfunc_end"):
                break
            if s and not (s.startswith(".") and not s.endswith(":")):
                body.append(s)
        out[sym] = (meta[sym], body)
    return out


def blocks(body):
    """[(label, [events])], and the set of labels a later block branches back to"""
    res, cur, order = [], ("entry", []), {}
    for s in body:
        if s.endswith(":"):
            res.append(cur)
            cur = (s[:-1], [])
            continue
        op = s.split()[0]
        ev = cur[1]
        if re.match(r"(global|buffer|flat|scratch)_load", op):
            if ev and ev[-1][0] == "L":
                ev[-1] = ("L", ev[-1][1] + 1)
            else:
                ev.append(("L", 1))
        elif re.match(r"(global|buffer|flat|scratch)_(store|atomic)", op):
            if ev and ev[-1][0] == "S":
                ev[-1] = ("S", ev[-1][1] + 1)
            else:
                ev.append(("S", 1))
        elif op == "s_waitcnt":
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                ev.append(("w", int(m.group(1))))
        elif op.startswith("s_cbranch") or op == "s_branch":
            ev.append(("c->" if op != "s_branch" else "->", s.split()[-1]))
    res.append(cur)
    for k, (lab, _) in enumerate(res):
        order[lab] = k
    loops = set()
    for k, (_, ev) in enumerate(res):
        for e in ev:
            if e[0].endswith("->") and order.get(e[1], 1 << 30) <= k:
                loops.add(e[1])
    return res, loops


def main():
    if len(sys.argv) < 2:
        sys.exit(__doc__)
    ks = kernels(sys.argv[1])
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    syms = sorted(ks)
    names = dict(zip(syms, subprocess.run([filt], input="\n".join(syms), capture_output=True, text=True).stdout.split("\n")))
    for sym in syms:
        name = names[sym]
        if sys.argv[2:] and not any(a in name for a in sys.argv[2:]):
            continue
        meta, body = ks[sym]
        print(f"== {name}")
        print("   " + "  ".join(f"{k}={v}" for k, v in sorted(meta.items())) + f"  instructions={len(body)}")
        bl, loops = blocks(body)
        for lab, ev in bl:
            if not ev:
                continue
            txt = " ".join(f"{a}{b}" if a in "LS" else (f"w({b})" if a == "w" else f"{a}{b}") for a, b in ev)
            print(f"   {lab + (' LOOP' if lab in loops else ''):18s} {txt}")


if __name__ == "__main__":
    main()
