#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: the epoch loop of the 9-state kernel carries no covariance across
its back-edge in registers.

The bench kernel runs one wavefront per SIMD, and a register copy costs it what an fma costs. Whatever a lane keeps in
registers from one epoch to the next has to end every way through the loop body (ML initialisation, too few ranges,
update skipped, both forms of the gain iteration) in the registers the loop's header expects: the compiler pays for
that with copies in the latch block, and for the 45 covariance entries with a second and third round of copies around
the phases that need the same registers. The covariance's home between two epochs is the LDS park; what a lane
legitimately carries across the back-edge is position, velocity, `invertible` and a few words.

For every listed kernel this finds the epoch loop (the largest cycle of the control-flow graph), takes away the loops
nested in it (the gain iteration's trips, the Gauss-Newton loop, ...) and prints the instruction mix of every block that
is left -- the turnaround, executed once per epoch -- and the totals: fp64 arithmetic, other VALU, AGPR reads and writes,
v_mov, lane reads and writes, DS, SALU, branches. It fails on one fact only: the latch blocks of the epoch loop (the
blocks that branch back to its header) hold more than --max-copies (32) register copies (v_mov*, v_accvgpr_*: reads,
writes and the AGPR-to-AGPR v_accvgpr_mov, which has no column of its own in the listing): six doubles and a few words
are 16 registers at most, and 32 allows twice that.

usage: epoch_turnaround_shape.py LIB [--kernel REGEX ...] [--max-copies 32] [--quiet]
(LIB: the library, or a disassembly as .s / .txt; --quiet: the verdict without the listing)
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from epoch_loop_waits import KERNELS, VMEM, parse  # noqa: E402  (same kernels, same disassembly parsing)
from trip_loop_shape import blocks_of, components, is_branch, is_fp64  # noqa: E402

MAX_COPIES = 32
COLUMNS = ("instructions", "fp64", "valu_other", "agpr_read", "agpr_write", "v_mov", "lane_read", "lane_write", "ds",
           "vmem", "salu", "branches")


def is_copy(op):
    return op.startswith(("v_mov_b", "v_accvgpr_"))


def mix(ins, idx):
    ops = [ins[i][1] for i in idx]
    return {
        "instructions": len(ops),
        "fp64": sum(is_fp64(o) for o in ops),
        "valu_other": sum(o.startswith("v_") and not is_fp64(o) for o in ops),
        "agpr_read": sum(o.startswith("v_accvgpr_read") for o in ops),
        "agpr_write": sum(o.startswith("v_accvgpr_write") for o in ops),
        "v_mov": sum(o.startswith("v_mov_b") for o in ops),
        "lane_read": sum(o.startswith("v_readlane") or o.startswith("v_readfirstlane") for o in ops),
        "lane_write": sum(o.startswith("v_writelane") for o in ops),
        "ds": sum(o.startswith("ds_") for o in ops),
        "vmem": sum(o.startswith(VMEM) for o in ops),
        "salu": sum(o.startswith("s_") and not is_branch(o) and o not in ("s_waitcnt", "s_nop") for o in ops),
        "branches": sum(is_branch(o) for o in ops),
    }


def epoch_loop(ins):
    """(blocks of the epoch loop, its header blocks, its latch blocks, its blocks outside nested loops, cfg) or None"""
    cfg = blocks_of(ins)
    starts, ends, succ = cfg
    n = len(starts)
    comps = components(range(n), succ)
    if not comps:
        return None
    size = lambda comp: sum(ends[b] - starts[b] for b in comp)
    loop = max(comps, key=size)
    inside = set(loop)
    pred = [[] for _ in range(n)]
    for b, out in enumerate(succ):
        for w in out:
            pred[w].append(b)
    headers = [b for b in loop if any(p not in inside for p in pred[b])] or [loop[0]]
    latches = [b for b in loop if any(w in headers for w in succ[b])]
    nested = set()
    for c in components(inside - set(headers), succ):
        nested |= set(c)
    return loop, headers, latches, [b for b in loop if b not in nested], cfg


def check(text, kernels=KERNELS, max_copies=MAX_COPIES, report=None):
    problems = []
    insns = parse(text)
    for pattern in kernels:
        names = [f for f in insns if re.search(pattern, f) and insns[f]]
        if not names:
            problems.append(f"{pattern}: no kernel of that name")
        for f in names:
            ins = insns[f]
            found = epoch_loop(ins)
            if found is None:
                problems.append(f"{f}: no loop")
                continue
            loop, headers, latches, outside, (starts, ends, _) = found
            total = dict.fromkeys(COLUMNS, 0)
            if report is not None:
                report.append(f"{f}: epoch loop of {len(loop)} blocks, {len(outside)} of them outside nested loops")
                report.append("  " + "address".rjust(9) + " " + " ".join(c.rjust(12) for c in COLUMNS))
            for b in outside:
                m = mix(ins, range(starts[b], ends[b]))
                for c in COLUMNS:
                    total[c] += m[c]
                if report is not None:
                    mark = " header" if b in headers else " latch" if b in latches else ""
                    report.append(f"  {ins[starts[b]][0]:#9x} " + " ".join(str(m[c]).rjust(12) for c in COLUMNS) + mark)
            if report is not None:
                report.append("  " + "total".rjust(9) + " " + " ".join(str(total[c]).rjust(12) for c in COLUMNS))
            copies = sum(is_copy(ins[i][1]) for b in latches for i in range(starts[b], ends[b]))
            where = ", ".join(f"{ins[starts[b]][0]:#x}" for b in latches)
            if report is not None:
                report.append(f"{f}: latch block(s) at {where}: {copies} register copies")
            if copies > max_copies:
                problems.append(f"{f}: latch block(s) at {where}: {copies} register copies (maximum {max_copies})")
    return problems


if __name__ == "__main__":
    args = sys.argv[1:]
    kernels, mc = [], MAX_COPIES
    quiet = "--quiet" in args
    if quiet:
        args.remove("--quiet")
    while "--kernel" in args:
        i = args.index("--kernel"); kernels.append(args[i + 1]); del args[i:i + 2]
    if "--max-copies" in args:
        i = args.index("--max-copies"); mc = int(args[i + 1]); del args[i:i + 2]
    if args[0].endswith((".s", ".txt")):
        text = open(args[0]).read()
    else:
        from check_scratch import disassemble
        text = disassemble(args[0])
    rep = []
    probs = check(text, tuple(kernels) or KERNELS, mc, rep)
    if rep and not quiet:
        print("\n".join(rep))
    if probs:
        print("the 9-state epoch loop carries too much across its back-edge in registers:\n" + "\n".join(probs))
        sys.exit(1)
    print(f"the latch of the 9-state epoch loop holds at most {mc} register copies")
