#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: a trip of the PAIRS' loop of the 9-state gain iteration pays for
arithmetic only.

The tail of the iteration runs two lanes per tag (iekf9_pairs_held in the two headline kernels): each lane sweeps four
anchors, a DPP exchange completes the sums, both run the pass. As in the one-tag-per-lane trip (tools/trip_loop_shape.py)
nothing else is resident on the SIMD, so an LDS read with its `s_waitcnt lgkmcnt` inside a pair trip is paid in full in
every trip: B^-1, Sigma^-1 and the lane's anchors belong in registers in front of the loop.

For every listed kernel this finds the pairs' loops -- the innermost cycles of the control-flow graph that hold at least
--min-fp64 (300) fp64 arithmetic instructions and a DPP move with a quad_perm modifier (the exchange) -- and fails when
one of them contains
  * a DS or vector-memory instruction,
  * an `s_waitcnt` with an lgkmcnt or vmcnt field,
  * more than the agreed number of branch instructions on the usual path of a trip (the cycle through the loop's entry
    with the fewest instructions among those that carry --min-fp64 fp64 instructions): --max-branches (4) for the fast
    form, one more for the per-lane form, which looks at `imu.has` lane by lane (recognised by its second
    `s_and_saveexec`, as in trip_loop_shape.py).
Every kernel must have a pairs' loop of the fast form: the pair pass takes the form its wavefront runs.
It prints the instruction mix of every loop it looked at.

usage: pairs_loop_shape.py LIB [--kernel REGEX ...] [--min-fp64 300] [--max-branches 4] [--quiet]
(LIB: the library, or a disassembly as .s / .txt; --quiet: the verdict without the instruction mix)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epoch_loop_waits import KERNELS, parse  # noqa: E402
from trip_loop_shape import is_mem, is_mem_wait, mix, trip_loops, usual_path  # noqa: E402  (blocks_of through trip_loops)

MIN_FP64 = 300
MAX_BRANCHES = 4


def is_exchange(args):
    return "quad_perm" in args


def check(text, kernels=KERNELS, min_fp64=MIN_FP64, max_branches=MAX_BRANCHES, report=None):
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
            found = []
            for comp, entries in loops:
                idx = [i for b in comp for i in range(starts[b], ends[b])]
                if any(is_exchange(ins[i][2]) for i in idx):
                    found.append((comp, entries, idx, mix(ins, idx)))
            if not found:
                problems.append(f"{f}: no loop with {min_fp64} fp64 instructions and a quad_perm exchange: where are the pairs?")
            elif min(l[3]["saveexec"] for l in found) > 1:
                problems.append(f"{f}: no fast form: every pairs' loop has more than one masked region (s_and_saveexec)")
            for comp, entries, idx, whole in found:
                where = f"{f}: pairs' loop at {ins[idx[0]][0]:#x}"
                fast = whole["saveexec"] <= 1
                allowed = max_branches if fast else max_branches + 1
                path = usual_path(ins, comp, entries, cfg, min_fp64)
                on_path = mix(ins, [i for b in path for i in range(starts[b], ends[b])]) if path else None
                if report is not None:
                    report.append(where + (" (fast form)" if fast else " (per-lane form)")
                                  + f": {len(comp)} blocks, " + ", ".join(f"{k} {v}" for k, v in whole.items()))
                    if on_path:
                        report.append(where + ": usual path: " + ", ".join(f"{k} {v}" for k, v in on_path.items()))
                for i in idx:
                    a, op, args, _ = ins[i]
                    if is_mem(op):
                        problems.append(f"{where}: {op} at {a:#x}: a pair trip reads or writes memory")
                    elif is_mem_wait(op, args):
                        problems.append(f"{where}: s_waitcnt {args} at {a:#x}: a pair trip waits for memory")
                if on_path is None:
                    problems.append(f"{where}: no cycle through its entry carries {min_fp64} fp64 instructions")
                elif on_path["branches"] > allowed:
                    problems.append(f"{where}: {on_path['branches']} branch instructions on the usual path of a pair trip "
                                    f"(maximum {allowed})")
    return problems


if __name__ == "__main__":
    args = sys.argv[1:]
    kernels, mf, mb = [], MIN_FP64, MAX_BRANCHES
    quiet = "--quiet" in args
    if quiet:
        args.remove("--quiet")
    while "--kernel" in args:
        i = args.index("--kernel"); kernels.append(args[i + 1]); del args[i:i + 2]
    if "--min-fp64" in args:
        i = args.index("--min-fp64"); mf = int(args[i + 1]); del args[i:i + 2]
    if "--max-branches" in args:
        i = args.index("--max-branches"); mb = int(args[i + 1]); del args[i:i + 2]
    if args[0].endswith((".s", ".txt")):
        text = open(args[0]).read()
    else:
        from check_scratch import disassemble
        text = disassemble(args[0])
    rep = []
    probs = check(text, tuple(kernels) or KERNELS, mf, mb, rep)
    if rep and not quiet:
        print("\n".join(rep))
    if probs:
        print("a pair trip of the 9-state gain iteration pays for more than arithmetic:\n" + "\n".join(probs))
        sys.exit(1)
    print(f"the pairs' loops of the 9-state gain iteration hold no memory access or wait and at most {mb} branches a trip")
