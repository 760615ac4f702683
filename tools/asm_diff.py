#!/usr/bin/env python3
"""Here (no GPU): compare the device code of two builds kernel by kernel.

  tools/asm_diff.py A.s A.remarks B.s B.remarks [--names parent,branch]

A.s / B.s: device assembly (the device flags of ptamd/build.py plus `--cuda-device-only -S`); *.remarks: the compiler's stderr of the same
command with -Rpass-analysis=kernel-resource-usage (tools/resources.sh).  Per kernel the instruction streams are compared after comments,
directives and label names are stripped:
  class 1  identical stream
  class 2  same instruction count, same mnemonic histogram, same resource line: only the order of instructions or register names differ
  class 3  anything else
and one table row is printed: instruction counts, class, VGPRs, SGPRs, LDS, scratch, occupancy (B's; A's in brackets where they differ)."""
import collections
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def kernels(path):
    """name -> list of instructions (labels replaced by a placeholder) for every .amdhsa_kernel of the file"""
    lines = open(path).read().split("\n")
    wanted = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out, cur = {}, None
    for l in lines:
        l = l.split(";")[0].rstrip()
        m = re.match(r"^([A-Za-z_$][\w$.]*):\s*$", l)
        if m and m.group(1) in wanted:
            cur = out.setdefault(m.group(1), [])
            continue
        s = l.strip()
        if cur is None or not s:
            continue
        if s.startswith(".Lfunc_end"):
            cur = None
            continue
        if s.startswith(".") or s.endswith(":"):  # directives, labels
            continue
        cur.append(re.sub(r"\.L\w+", "L", re.sub(r"\s+", " ", s)))
    return out


def resources(path):
    """name -> {VGPRs, SGPRs, LDS, scratch, occupancy} from the resource-usage remarks"""
    out, cur = {}, None
    keys = {"VGPRs": "VGPRs", "TotalSGPRs": "SGPRs", "LDS Size [bytes/block]": "LDS", "ScratchSize [bytes/lane]": "scratch", "Occupancy [waves/SIMD]": "occupancy"}
    for l in open(path):
        m = re.search(r"remark: (?:.*?:\d+:\d+: )?\s*(.+?): (\S+) \[-Rpass", l) or re.search(r"remark:\s*(.+?): (\S+) \[-Rpass", l)
        if not m:
            continue
        k, v = m.group(1).strip(), m.group(2)
        if k == "Function Name":
            cur = out.setdefault(v, {})
        elif cur is not None and k in keys:
            cur[keys[k]] = v
    return out


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--names")]
    names = ("A", "B")
    for i, a in enumerate(sys.argv):
        if a == "--names":
            names = tuple(sys.argv[i + 1].split(","))
            args.remove(sys.argv[i + 1])
    sa, ra, sb, rb = args
    ka, kb, resA, resB = kernels(sa), kernels(sb), resources(ra), resources(rb)
    pretty = demangle(sorted(set(ka) | set(kb)))
    cols = ("VGPRs", "SGPRs", "LDS", "scratch", "occupancy")
    print(f"{'kernel':100s} {'instr ' + names[0]:>12s} {'instr ' + names[1]:>12s} class " + " ".join(f"{c:>12s}" for c in cols))
    tally = collections.Counter()
    for k in sorted(set(ka) | set(kb), key=lambda n: pretty[n]):
        a, b = ka.get(k), kb.get(k)
        if a is None or b is None:
            print(f"{pretty[k][:100]:100s} only in {names[0] if b is None else names[1]}")
            tally["3"] += 1
            continue
        hist = lambda seq: collections.Counter(i.split(" ")[0] for i in seq)
        same_res = resA.get(k) == resB.get(k)
        cls = "1" if a == b else ("2" if len(a) == len(b) and hist(a) == hist(b) and same_res else "3")
        tally[cls] += 1
        cell = lambda c: resB.get(k, {}).get(c, "?") + ("" if resA.get(k, {}).get(c) == resB.get(k, {}).get(c) else f" [{resA.get(k, {}).get(c, '?')}]")
        print(f"{pretty[k][:100]:100s} {len(a):12d} {len(b):12d} {cls:>5s} " + " ".join(f"{cell(c):>12s}" for c in cols))
    print(f"{sum(tally.values())} kernels: class 1 {tally['1']}, class 2 {tally['2']}, class 3 {tally['3']}")


if __name__ == "__main__":
    main()
