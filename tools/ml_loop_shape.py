#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: a pass of the Gauss-Newton seed loop pays for arithmetic only.

Every epoch of the 9-state bench kernels solves the multilateration problem once (ml_estimate, kfpos_core_ml.h) to seed
the gain iteration, and the wavefront pays its slowest lane: about six passes per wavefront and epoch at ~350 fp64
instructions each. The first pass is peeled off in front of the loop -- its convergence test compares two constants --
so a pass of the loop is a sweep over the anchors, the voted convergence test and the step. Like a trip of the gain
iteration (tools/trip_loop_shape.py, whose machinery this uses) it is run by a lone wavefront that issues in order: a
wait for memory drains the pipeline and every branch is a VALU -> SALU hand-off, paid in every pass.

For every listed kernel this finds the Gauss-Newton loops -- the innermost cycles of the control-flow graph that hold
between --min-fp64 (300) and --max-fp64 (399) fp64 arithmetic instructions and no DPP exchange (the pairs' loop of the
gain iteration, which has a rule of its own, is of that size too and is known by its quad_perm modifier) -- and fails
when one of them contains
  * a DS or vector-memory instruction,
  * an `s_waitcnt` with an lgkmcnt or vmcnt field,
  * more than --max-branches (4: the vote of the convergence test, the skip of the step for lanes that have converged,
    the loop's exit and its back-edge) branch instructions on the usual path of a pass: of all simple cycles through the
    loop's entry block that carry at least --min-fp64 fp64 instructions, the one with the fewest instructions; every
    s_branch / s_cbranch of its blocks counts, taken or not,
or when a kernel does not hold --copies (2: the ML start of a tag and the seed of every step) such loops.
It prints the instruction mix of every loop it looked at.

usage: ml_loop_shape.py LIB [--kernel REGEX ...] [--min-fp64 300] [--max-fp64 399] [--max-branches 4] [--copies 2] [--quiet]
(LIB: the library, or a disassembly as .s / .txt; --quiet: the verdict without the instruction mix)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epoch_loop_waits import KERNELS, parse  # noqa: E402  (same kernels, same disassembly parsing)
from trip_loop_shape import is_mem, is_mem_wait, mix, trip_loops, usual_path  # noqa: E402

MIN_FP64 = 300
MAX_FP64 = 399
MAX_BRANCHES = 4
COPIES = 2


def check(text, kernels=KERNELS, min_fp64=MIN_FP64, max_fp64=MAX_FP64, max_branches=MAX_BRANCHES, copies=COPIES,
          report=None):
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
            found = 0
            for comp, entries in loops:
                idx = [i for b in comp for i in range(starts[b], ends[b])]
                whole = mix(ins, idx)
                if whole["fp64"] > max_fp64 or any("quad_perm" in ins[i][2] for i in idx):
                    continue  # a trip loop of the gain iteration, per lane or in pairs: not this rule's business
                found += 1
                where = f"{f}: Gauss-Newton loop at {ins[idx[0]][0]:#x}"
                path = usual_path(ins, comp, entries, cfg, min_fp64)
                on_path = mix(ins, [i for b in path for i in range(starts[b], ends[b])]) if path else None
                if report is not None:
                    report.append(where + f": {len(comp)} blocks, " + ", ".join(f"{k} {v}" for k, v in whole.items()))
                    if on_path:
                        report.append(where + ": usual path: " + ", ".join(f"{k} {v}" for k, v in on_path.items()))
                for i in idx:
                    a, op, args, _ = ins[i]
                    if is_mem(op):
                        problems.append(f"{where}: {op} at {a:#x}: a pass reads or writes memory")
                    elif is_mem_wait(op, args):
                        problems.append(f"{where}: s_waitcnt {args} at {a:#x}: a pass waits for memory")
                if on_path is None:
                    problems.append(f"{where}: no cycle through its entry carries {min_fp64} fp64 instructions")
                elif on_path["branches"] > max_branches:
                    problems.append(f"{where}: {on_path['branches']} branch instructions on the usual path of a pass "
                                    f"(maximum {max_branches})")
            if found != copies:
                problems.append(f"{f}: {found} loop(s) with {min_fp64}-{max_fp64} fp64 instructions and no exchange, "
                                f"{copies} expected: where is the Gauss-Newton loop?")
    return problems


if __name__ == "__main__":
    args = sys.argv[1:]
    kernels, mf, xf, mb, cp = [], MIN_FP64, MAX_FP64, MAX_BRANCHES, COPIES
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
    if "--copies" in args:
        i = args.index("--copies"); cp = int(args[i + 1]); del args[i:i + 2]
    if args[0].endswith((".s", ".txt")):
        text = open(args[0]).read()
    else:
        from check_scratch import disassemble
        text = disassemble(args[0])
    rep = []
    probs = check(text, tuple(kernels) or KERNELS, mf, xf, mb, cp, rep)
    if rep and not quiet:
        print("\n".join(rep))
    if probs:
        print("a pass of the Gauss-Newton seed loop pays for more than arithmetic:\n" + "\n".join(probs))
        sys.exit(1)
    print(f"the Gauss-Newton loops of the 9-state kernels hold no memory access or wait and at most {mb} branches a pass")
