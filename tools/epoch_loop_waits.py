#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: the epoch loop of the 9-state kernel waits for no vector-memory
operation it has only just issued.

The kernel runs one wavefront per SIMD, so nothing hides a memory round trip: an `s_waitcnt vmcnt(N)` a few
instructions behind a load or a store stalls the whole SIMD for an L2 hit (~200 cycles) or an HBM miss (~900 cycles) in
every epoch, with every parity test still green. vmcnt counts loads AND stores, in issue order: vmcnt(N) returns once at
most N vector-memory operations are outstanding, i.e. it can still be waiting for the (N+1)-th youngest one.

For every listed kernel this finds the outermost loop (the largest cycle of the control-flow graph, its instructions
taken in layout order) and, for every `s_waitcnt` with a vmcnt field inside it, the static distance in instructions -- layout order,
walking backwards and around the loop's back-edge -- to the youngest vector-memory instruction the wait can still be
waiting for. It fails when that distance is under --min-distance (300: a 900-cycle HBM miss / at least 4 cycles per
instruction = 225, plus margin). It looks at s_waitcnt and vector-memory mnemonics only.

usage: epoch_loop_waits.py LIB [--kernel REGEX ...] [--min-distance 300] [--quiet]
(LIB: the library, or a disassembly as .s / .txt; --quiet: the verdict without the list of waits)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

# k_step_imu9<double,float,8,true> (the bench kernel) and k_step_imu9<p48,float,8,true>, mangled
KERNELS = (r"k_step_imu9IdfLi8ELb1E", r"k_step_imu9I\w*p48\w*fLi8ELb1E")
MIN_DISTANCE = 300
VMEM = ("global_", "flat_", "buffer_", "scratch_", "tbuffer_")
LINE = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*[0-9A-Fa-f ]*(?:<\S+?(?:\+0x([0-9a-fA-F]+))?>)?\s*$")


def parse(text):
    """{function: [(address, opcode, operands, branch target offset from the function start or None)]}"""
    func, insns = None, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            func = m.group(1)
            insns[func] = []
            continue
        m = LINE.match(line)
        if m and func:
            off = None
            if m.group(1).startswith(("s_cbranch", "s_branch")) and "<" in line:
                off = int(m.group(4), 16) if m.group(4) else 0
            insns[func].append((int(m.group(3), 16), m.group(1), m.group(2), off))
    return insns


def outermost_loop(ins):
    """Instruction indices, in layout order, of the largest strongly connected component of the control-flow graph (the
    epoch loop with everything nested in it), or None when the function has no loop"""
    base = ins[0][0]
    index = {a: i for i, (a, _, _, _) in enumerate(ins)}
    target = [index.get(base + off) if off is not None else None for _, _, _, off in ins]
    leaders = {0}
    for i, (_, op, _, _) in enumerate(ins):
        if target[i] is not None:
            leaders.add(target[i])
        if (target[i] is not None or op == "s_endpgm") and i + 1 < len(ins):
            leaders.add(i + 1)
    starts = sorted(leaders)
    ends = starts[1:] + [len(ins)]
    block_at = {st: b for b, st in enumerate(starts)}
    succ = []
    for st, en in zip(starts, ends):
        out, op = [], ins[en - 1][1]
        if target[en - 1] is not None:
            out.append(block_at[target[en - 1]])
        if op not in ("s_branch", "s_endpgm") and en < len(ins):
            out.append(block_at[en])
        succ.append(out)
    # Tarjan's strongly connected components, iterative
    n = len(starts)
    num, low, on, stack, comps, counter = [None] * n, [0] * n, [False] * n, [], [], 0
    for root in range(n):
        if num[root] is not None:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                num[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on[v] = True
            if k < len(succ[v]):
                w = succ[v][k]
                work.append((v, k + 1))
                if num[w] is None:
                    work.append((w, 0))
                elif on[w]:
                    low[v] = min(low[v], num[w])
                continue
            if low[v] == num[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on[w] = False
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(comp)
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
    if not comps:
        return None
    size = lambda comp: sum(ends[b] - starts[b] for b in comp)
    return sorted(i for b in max(comps, key=size) for i in range(starts[b], ends[b]))


def waits_in_loop(ins):
    """[(address, N, distance or None)] for every s_waitcnt vmcnt(N) of the outermost loop; None: the loop has no
    N+1 vector-memory instructions, the wait cannot be waiting for one of its own"""
    body = outermost_loop(ins)
    if body is None:
        return None
    n = len(body)
    out = []
    for p, i in enumerate(body):
        a, op, args, _ = ins[i]
        m = re.search(r"vmcnt\((\d+)\)", args) if op == "s_waitcnt" else None
        if not m:
            continue
        skip, dist = int(m.group(1)), None
        for d in range(1, n):
            if ins[body[(p - d) % n]][1].startswith(VMEM):
                if skip == 0:
                    dist = d
                    break
                skip -= 1
        out.append((a, int(m.group(1)), dist))
    return out


def check(text, kernels=KERNELS, min_distance=MIN_DISTANCE, report=None):
    problems = []
    insns = parse(text)
    for pattern in kernels:
        names = [f for f in insns if re.search(pattern, f) and insns[f]]
        if not names:
            problems.append(f"{pattern}: no kernel of that name")
        for f in names:
            waits = waits_in_loop(insns[f])
            if waits is None:
                problems.append(f"{f}: no loop")
                continue
            for a, cnt, dist in waits:
                line = f"{f}: s_waitcnt vmcnt({cnt}) at {a:#x}: " + (
                    "nothing of this loop to wait for" if dist is None else
                    f"{dist} instructions behind the youngest vector-memory instruction it can wait for")
                if report is not None:
                    report.append(line)
                if dist is not None and dist < min_distance:
                    problems.append(line + f" (minimum {min_distance})")
    return problems


if __name__ == "__main__":
    args = sys.argv[1:]
    kernels, md = [], MIN_DISTANCE
    quiet = "--quiet" in args
    if quiet:
        args.remove("--quiet")
    while "--kernel" in args:
        i = args.index("--kernel"); kernels.append(args[i + 1]); del args[i:i + 2]
    if "--min-distance" in args:
        i = args.index("--min-distance"); md = int(args[i + 1]); del args[i:i + 2]
    if args[0].endswith((".s", ".txt")):
        text = open(args[0]).read()
    else:
        from check_scratch import disassemble
        text = disassemble(args[0])
    rep = []
    probs = check(text, tuple(kernels) or KERNELS, md, rep)
    if rep and not quiet:
        print("\n".join(rep))
    if probs:
        print("epoch loop waits for a vector-memory operation it has just issued:\n" + "\n".join(probs))
        sys.exit(1)
    print(f"no epoch loop waits for a vector-memory operation issued fewer than {md} instructions before")
