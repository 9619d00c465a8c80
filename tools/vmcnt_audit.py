"""Audit the vector-memory waits of a kernel's matrix loops in hipcc's ISA (-S output).

Vector memory operations retire in order, so `s_waitcnt vmcnt(N)` waits for all but the N youngest.  Two things undo a
hand-built look-ahead (loads issued k-tiles before their use and retired by COUNTED waits):
  * a reload from scratch inside the loop: it is a vector-memory operation itself, the wait in front of its use is
    vmcnt(0), and that drains every look-ahead load in flight;
  * a counted wait that reaches an operation issued only a few dozen instructions earlier (or a store of the same pass):
    a stall for a full memory round trip -- typically a false register dependency hipcc's waitcnt pass sees.
For every loop that holds matrix instructions -- closed by a conditional OR an unconditional back-branch; hipcc ends the
unrolled k-loops with `s_cbranch <exit>; s_branch <header>` -- and for every stretch of matrix instructions outside such a
loop (the tail k-tiles behind it, or a kernel without a loop), the report gives: matrix instructions, scratch operations,
vmcnt(0) waits, counted waits; and for every counted wait of a loop in steady state (second pass), the youngest operation
that has to be complete and how many instructions ago it was issued.  Lines are counted textually: both arms of a branch
inside the region count.
usage: python3 tools/vmcnt_audit.py <file.s> <kernel name substring> [min_age] [--brief]"""
import re
import sys

VMEM = re.compile(r"(global|buffer|flat|scratch)_(load|store|atomic)")
WAIT = re.compile(r"s_waitcnt.*vmcnt\((\d+)\)")
BRANCH = re.compile(r"s_c?branch\w* (\.LBB\w+)")


def instructions(lines):
    return [l.strip() for l in lines if l.strip() and not l.strip().startswith(";") and not l.startswith(".")]


def counts(lines):
    ins = instructions(lines)
    waits = [int(m.group(1)) for m in map(WAIT.match, ins) if m]
    return {"mfma": sum(t.startswith("v_mfma") for t in ins), "scratch": sum(t.startswith("scratch_") for t in ins),
            "vmcnt0": sum(n == 0 for n in waits), "counted": sum(n > 0 for n in waits)}


def kernels(lines, name):
    """(symbol, first line, last line) of every kernel whose symbol holds `name`"""
    out = []
    for i, l in enumerate(lines):
        if l.startswith("_Z") and ":" in l and name in l.split(":")[0]:
            end = next(j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end"))
            out.append((l.split(":")[0], i, end))
    return out


def regions(body):
    """matrix loops (innermost first when nested) and the stretches of matrix instructions outside them"""
    labels = {l.split(":")[0]: i for i, l in enumerate(body) if l.startswith(".LBB")}
    loops = set()
    for i, l in enumerate(body):
        m = BRANCH.search(l)
        if m and labels.get(m.group(1), i) < i:
            loops.add((labels[m.group(1)], i))
    # one loop per header: its furthest back-branch
    by_head = {}
    for a, b in loops:
        by_head[a] = max(b, by_head.get(a, b))
    loops = sorted((a, b) for a, b in by_head.items() if counts(body[a:b])["mfma"])
    outer = [(a, b) for a, b in loops if not any(c <= a and b <= d and (c, d) != (a, b) for c, d in loops)]
    covered = [False] * len(body)
    for a, b in outer:
        for i in range(a, b + 1):
            covered[i] = True
    # stretches outside: from the block that holds the first matrix instruction to the end of the block that holds the last
    tails, i = [], 0
    while i < len(body):
        if covered[i]:
            i += 1
            continue
        j = i
        while j < len(body) and not covered[j]:
            j += 1
        mf = [k for k in range(i, j) if body[k].strip().startswith("v_mfma")]
        if mf:
            a = max([k for k in range(i, mf[0]) if body[k].startswith(".LBB")], default=i)
            b = next((k for k in range(mf[-1], j) if body[k].startswith(".LBB")), j)
            tails.append((a, b))
        i = j
    return loops, tails


def wait_ages(loop, min_age):
    seq = loop + loop      # two passes: the second one is steady state
    ops = []               # (position, text) of vector memory operations in issue order
    for pos, t in enumerate(seq):
        if VMEM.match(t):
            ops.append((pos, t))
        m = WAIT.match(t)
        if m and pos >= len(loop):
            n = int(m.group(1))
            if len(ops) > n:
                ypos, ytxt = ops[len(ops) - n - 1]
                age = pos - ypos
                flag = "  <-- STALL RISK" if age < min_age else ""
                yield f"    line {pos - len(loop):4d}  vmcnt({n:2d}) needs `{ytxt[:60]}` issued {age} instructions earlier{flag}"


def audit(path, name, min_age=150, brief=False, out=sys.stdout):
    lines = open(path).read().split("\n")
    found = kernels(lines, name)
    if not found:
        raise SystemExit(f"no kernel matches {name!r}")
    for sym, start, end in found:
        body = lines[start:end]
        loops, tails = regions(body)
        print(f"{sym}: {len(loops)} matrix loop(s), {len(tails)} stretch(es) of matrix instructions outside them", file=out)
        for kind, spans in (("loop", loops), ("tail", tails)):
            for a, b in spans:
                c = counts(body[a:b + 1])
                print(f"  {kind} lines {a}..{b}: {c['mfma']} matrix instructions, {c['scratch']} scratch ops, {c['vmcnt0']} vmcnt(0), "
                      f"{c['counted']} counted waits", file=out)
                if kind == "loop" and not brief:
                    for row in wait_ages(instructions(body[a:b + 1]), min_age):
                        print(row, file=out)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--brief"]
    audit(args[0], args[1], int(args[2]) if len(args) > 2 else 150, brief="--brief" in sys.argv)
