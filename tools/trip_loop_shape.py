#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: a trip of the 9-state gain iteration pays for arithmetic only.

The bench kernel runs one wavefront per SIMD and spends 70 % of an epoch in the trip loop of the information-form gain
iteration (sweep over the anchors + pass, 16-20 trips per wavefront and epoch). A wavefront issues in order and nothing
else is resident on its SIMD, so whatever a trip executes besides its ~510 fp64 instructions is paid in full, twenty times
per epoch: an LDS read with its `s_waitcnt lgkmcnt` drains the pipeline, and every branch is a VALU -> SALU hand-off.
What the trip reads from the park (B^-1, Sigma^-1) is constant over the loop and belongs in registers in front of it.

For every listed kernel this finds the trip loops -- the innermost cycles of the control-flow graph whose blocks hold at
least --min-fp64 (400) fp64 arithmetic instructions: a strongly connected component is split again, without its entry
blocks, as long as a part of it still holds that many -- and fails when one of them contains
  * a DS or vector-memory instruction,
  * an `s_waitcnt` with an lgkmcnt or vmcnt field,
  * more than the agreed number of branch instructions on the usual path of a trip: of all simple cycles through the
    loop's entry block that carry at least --min-fp64 fp64 instructions, the one with the fewest instructions; every
    s_branch / s_cbranch of its blocks counts, taken or not. The agreed number is --max-branches (4: the vote of the
    convergence test, the skip of the solve for lanes that have converged, the loop's exit and its back-edge) for the
    fast form -- diagonal and every lane with a sample, which is what the bench runs -- and one more for the per-lane
    form, which looks at `imu.has` lane by lane: that is a second masked region, and the form is recognised by it (more
    than one `s_and_saveexec` in the loop; the fast form has one, around the solve). Every kernel must have a fast
    form: if the per-lane branch came back into it, no loop with a single masked region would be left, and that fails.
Two kinds of loop are listed but not judged:
  * the pairs' loop (two lanes per tag), which has a rule of its own (tools/pairs_loop_shape.py); it is recognised by its
    DPP exchange (an instruction with a quad_perm modifier);
  * loops with more than --max-fp64 (700) fp64 instructions: the (I + M B) form of the iteration, taken right after a
    fixed start while B is singular, whose loop holds an adjugate and a pivoted solve side by side (~950).
It prints the instruction mix of every loop it looked at.

usage: trip_loop_shape.py LIB [--kernel REGEX ...] [--min-fp64 400] [--max-fp64 700] [--max-branches 4] [--quiet]
(LIB: the library, or a disassembly as .s / .txt; --quiet: the verdict without the instruction mix)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epoch_loop_waits import KERNELS, VMEM, parse  # noqa: E402  (same kernels, same disassembly parsing)

MIN_FP64 = 400
MAX_FP64 = 700
MAX_BRANCHES = 4
FP64 = re.compile(r"^v_(mul|fmac|fma|add|rsq|rcp|sqrt|min|max|ldexp|div_\w+|trig_preop|frexp_mant|fract|floor|ceil|rndne|trunc)_f64")


def is_fp64(op):
    return bool(FP64.match(op))


def is_branch(op):
    return op.startswith(("s_cbranch", "s_branch"))


def is_mem(op):
    return op.startswith("ds_") or op.startswith(VMEM)


def is_mem_wait(op, args):
    return op == "s_waitcnt" and ("lgkmcnt" in args or "vmcnt" in args)


def blocks_of(ins):
    """(starts, ends, succ): basic blocks as instruction index ranges and their successor lists"""
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
        if op not in ("s_branch", "s_endpgm") and en < len(ins) and block_at[en] not in out:
            out.append(block_at[en])
        succ.append(out)
    return starts, ends, succ


def components(nodes, succ):
    """strongly connected components with a cycle, of the graph restricted to `nodes` (Tarjan, iterative)"""
    nodes = set(nodes)
    num, low, on, stack, comps, counter = {}, {}, set(), [], [], 0
    for root in sorted(nodes):
        if root in num:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                num[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on.add(v)
            out = [w for w in succ[v] if w in nodes]
            if k < len(out):
                w = out[k]
                work.append((v, k + 1))
                if w not in num:
                    work.append((w, 0))
                elif w in on:
                    low[v] = min(low[v], num[w])
                continue
            if low[v] == num[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(sorted(comp))
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
    return comps


def trip_loops(ins, min_fp64=MIN_FP64):
    """[(blocks of the loop, its entry blocks)] for the innermost cycles that hold at least min_fp64 fp64 instructions;
    with (starts, ends, succ) as a second result"""
    starts, ends, succ = blocks_of(ins)
    n = len(starts)
    pred = [[] for _ in range(n)]
    for b, out in enumerate(succ):
        for w in out:
            pred[w].append(b)
    fp = [sum(is_fp64(ins[i][1]) for i in range(starts[b], ends[b])) for b in range(n)]
    found = []
    todo = [c for c in components(range(n), succ) if sum(fp[b] for b in c) >= min_fp64]
    while todo:
        comp = todo.pop()
        inside = set(comp)
        entries = [b for b in comp if any(p not in inside for p in pred[b])] or [comp[0]]
        inner = [c for c in components(inside - set(entries), succ) if sum(fp[b] for b in c) >= min_fp64]
        if inner:
            todo += inner
        else:
            found.append((comp, entries))
    return sorted(found), (starts, ends, succ)


def usual_path(ins, comp, entries, cfg, min_fp64=MIN_FP64):
    """blocks of the cycle through the loop's entry that carries the trip with the fewest instructions, or None"""
    starts, ends, succ = cfg
    inside = set(comp)
    size = {b: ends[b] - starts[b] for b in comp}
    fp = {b: sum(is_fp64(ins[i][1]) for i in range(starts[b], ends[b])) for b in comp}
    best = None
    for head in entries:
        work = [(head, [head])]
        while work:  # every simple path from the entry back to it (these loops have a handful of blocks)
            v, path = work.pop()
            for w in succ[v]:
                if w == head:
                    if sum(fp[b] for b in path) >= min_fp64:
                        cost = sum(size[b] for b in path)
                        if best is None or cost < best[0]:
                            best = (cost, path)
                elif w in inside and w not in path:
                    work.append((w, path + [w]))
    return None if best is None else best[1]


def mix(ins, idx):
    ops = [(ins[i][1], ins[i][2]) for i in idx]
    return {
        "instructions": len(ops),
        "fp64": sum(is_fp64(o) for o, _ in ops),
        "ds": sum(o.startswith("ds_") for o, _ in ops),
        "vmem": sum(o.startswith(VMEM) for o, _ in ops),
        "mem_waits": sum(is_mem_wait(o, a) for o, a in ops),
        "branches": sum(is_branch(o) for o, _ in ops),
        "salu": sum(o.startswith("s_") and not is_branch(o) and o not in ("s_waitcnt", "s_nop") for o, _ in ops),
        "v_mov": sum(o.startswith("v_mov_b") for o, _ in ops),
        "accvgpr": sum(o.startswith("v_accvgpr") for o, _ in ops),
        "saveexec": sum("saveexec" in o for o, _ in ops),
    }


def check(text, kernels=KERNELS, min_fp64=MIN_FP64, max_branches=MAX_BRANCHES, report=None, max_fp64=MAX_FP64):
    problems = []
    insns = parse(text)
    for pattern in kernels:
        names = [f for f in insns if re.search(pattern, f) and insns[f]]
        if not names:
            problems.append(f"{pattern}: no kernel of that name")
        for f in names:
            ins = insns[f]
            loops, cfg = trip_loops(ins, min_fp64)
            starts, ends, _ = cfg
            if not loops:
                problems.append(f"{f}: no loop with {min_fp64} fp64 instructions: where is the trip?")
            looked = []
            for comp, entries in loops:
                idx = [i for b in comp for i in range(starts[b], ends[b])]
                whole = mix(ins, idx)
                aside = ("the pairs' loop" if any("quad_perm" in ins[i][2] for i in idx) else
                         "the (I + M B) form" if whole["fp64"] > max_fp64 else None)
                looked.append((comp, entries, idx, whole, aside))
            judged = [l[3]["saveexec"] for l in looked if l[4] is None]
            if loops and not judged:
                problems.append(f"{f}: no trip loop of the information form")
            elif judged and min(judged) > 1:
                problems.append(f"{f}: no fast form: every trip loop has more than one masked region (s_and_saveexec)")
            for comp, entries, idx, whole, aside in looked:
                where = f"{f}: loop at {ins[idx[0]][0]:#x}"
                pairs = aside is not None
                allowed = max_branches if whole["saveexec"] <= 1 else max_branches + 1
                path = usual_path(ins, comp, entries, cfg, min_fp64)
                on_path = mix(ins, [i for b in path for i in range(starts[b], ends[b])]) if path else None
                if report is not None:
                    report.append(where + (f" ({aside}: listed only)" if pairs else "")
                                  + f": {len(comp)} blocks, " + ", ".join(f"{k} {v}" for k, v in whole.items()))
                    if on_path:
                        report.append(where + ": usual path: " + ", ".join(f"{k} {v}" for k, v in on_path.items()))
                if pairs:
                    continue
                for i in idx:
                    a, op, args, _ = ins[i]
                    if is_mem(op):
                        problems.append(f"{where}: {op} at {a:#x}: a trip reads or writes memory")
                    elif is_mem_wait(op, args):
                        problems.append(f"{where}: s_waitcnt {args} at {a:#x}: a trip waits for memory")
                if on_path is None:
                    problems.append(f"{where}: no cycle through its entry carries {min_fp64} fp64 instructions")
                elif on_path["branches"] > allowed:
                    problems.append(f"{where}: {on_path['branches']} branch instructions on the usual path of a trip "
                                    f"(maximum {allowed})")
    return problems


if __name__ == "__main__":
    args = sys.argv[1:]
    kernels, mf, mb, xf = [], MIN_FP64, MAX_BRANCHES, MAX_FP64
    quiet = "--quiet" in args
    if quiet:
        args.remove("--quiet")
    while "--kernel" in args:
        i = args.index("--kernel"); kernels.append(args[i + 1]); del args[i:i + 2]
    if "--min-fp64" in args:
        i = args.index("--min-fp64"); mf = int(args[i + 1]); del args[i:i + 2]
    if "--max-fp64" in args:
        i = args.index("--max-fp64"); xf = int(args[i + 1]); del args[i:i + 2]
    if "--max-branches" in args:
        i = args.index("--max-branches"); mb = int(args[i + 1]); del args[i:i + 2]
    if args[0].endswith((".s", ".txt")):
        text = open(args[0]).read()
    else:
        from check_scratch import disassemble
        text = disassemble(args[0])
    rep = []
    probs = check(text, tuple(kernels) or KERNELS, mf, mb, rep, xf)
    if rep and not quiet:
        print("\n".join(rep))
    if probs:
        print("a trip of the 9-state gain iteration pays for more than arithmetic:\n" + "\n".join(probs))
        sys.exit(1)
    print(f"the trip loops of the 9-state gain iteration hold no memory access or wait and at most {mb} branches a trip")
