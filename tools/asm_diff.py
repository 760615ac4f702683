#!/usr/bin/env python3
"""Here (no GPU): compare the device code of two builds kernel by kernel.

  tools/asm_diff.py A.s A.remarks B.s B.remarks [--names parent,branch]

A.s / B.s: device assembly (the device flags of ptamd/build.py plus `--cuda-device-only -S`); *.remarks: the compiler's stderr of the same
command with -Rpass-analysis=kernel-resource-usage (tools/resources.sh).  Per kernel the instruction streams are compared after comments,
directives and label names are stripped:
  class 1  identical stream
  class 2  same instruction count, same mnemonic histogram, same resource line: only the order of instructions or register names differ
  class 3  anything else
and one table row is printed: instruction counts, class, VGPRs, SGPRs, LDS, scratch, occupancy (B's; A's in brackets where they differ).

  tools/asm_diff.py --votes A.s [kernel-name regex]

counts what the wave votes of a kernel cost, whole kernel and per loop header (see `votes`)."""
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


def votes(path, pattern):
    """tools/asm_diff.py --votes A.s [kernel-name regex]: per kernel, and per loop header of it (label to first branch), the vector instructions and among them
      pairs   v_cndmask_b32 vN, 0, 1, s[..] answered by v_cmp_ne_u32 .., 0, vN: a lane mask that already sits in scalar registers turned into 0 / 1 per
              lane and compared with 0 again -- how the compiler lowers the ballot of anything but a single compare
      cmp64   64-bit vector compares whose operands are scalar registers or constants (a wave-uniform count compared on the vector unit)"""
    lines = open(path).read().split("\n")
    wanted = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    pretty = demangle(sorted(wanted))
    body, cur = {}, None
    for l in lines:
        m = re.match(r"^([A-Za-z_$][\w$.]*):", l)
        if m and m.group(1) in wanted:
            cur = body.setdefault(m.group(1), [])
            continue
        if l.startswith(".Lfunc_end"):
            cur = None
        if cur is not None:
            cur.append(l)

    def count(seq):
        ins = [re.sub(r"\s+", " ", l.split(";")[0].strip()) for l in seq]
        ins = [i for i in ins if i and not i.startswith(".") and not i.endswith(":")]
        valu = sum(1 for i in ins if i.startswith("v_"))
        pairs = 0
        for n, i in enumerate(ins):
            m = re.match(r"v_cndmask_b32_e64 (v\d+), 0, 1, s\[", i)
            if m:
                for j in ins[n + 1:n + 9]:
                    if re.match(r"v_cmp_ne_u32_e(32 vcc|64 s\[\d+:\d+\]), 0, " + m.group(1) + "$", j):
                        pairs += 1
                        break
                    if re.match(r"v_\w+ " + m.group(1) + r"\b", j):  # overwritten
                        break
        cmp64 = sum(1 for i in ins if re.match(r"v_cmp_\w+_[ui]64_e\d+ ", i) and not re.search(r"\bv\[?\d", i.split(" ", 1)[1]))
        return valu, pairs, cmp64

    print(f"{'kernel / loop header':100s} {'depth':>5s} {'VALU':>6s} {'pairs':>6s} {'cmp64':>6s}")
    for k in sorted(body, key=lambda n: pretty[n]):
        if not re.search(pattern, pretty[k]):
            continue
        seq = body[k]
        # pairs by the loop depth of the basic block they sit in (the compiler notes it on every block's label)
        by_depth, block, depth = collections.Counter(), [], 0
        for l in seq + [".LBB_end:"]:
            if re.match(r"^(\.LBB\w+:|; %bb\.\d+:)", l):
                by_depth[depth] += count(block)[1]
                block, depth = [], 0
            d = re.search(r"^\s*;.*Depth=(\d+)|^\S+:.*Depth=(\d+)", l)
            if d:
                depth = max(depth, int(d.group(1) or d.group(2)))
            block.append(l)
        where = ", ".join(f"depth {d}: {n}" for d, n in sorted(by_depth.items()) if n)
        print(f"{pretty[k][:100]:100s} {'':>5s} {count(seq)[0]:6d} {count(seq)[1]:6d} {count(seq)[2]:6d}" + (f"   pairs at loop {where}" if where else ""))
        for n, l in enumerate(seq):
            m = re.match(r"^(\.LBB\d+_\d+):", l)
            if not m:
                continue
            note = l  # the compiler's loop note: on the label's line and the comment lines below it
            for j in range(n + 1, len(seq)):
                if not re.match(r"\s*;", seq[j]):
                    break
                note += seq[j]
            d = re.search(r"Loop Header: Depth=(\d+)", note)
            if not d:
                continue
            name = m.group(1) + (" (encloses a loop)" if "Child Loop" in note else "")
            end = next((j for j in range(n + 1, len(seq)) if re.match(r"\s+s_c?branch", seq[j])), len(seq) - 1)
            v, p, c = count(seq[n + 1:end + 1])
            print(f"{'    ' + name + ' to first branch':100s} {d.group(1):>5s} {v:6d} {p:6d} {c:6d}")


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--votes":
        return votes(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else ".")
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
