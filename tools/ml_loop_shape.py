#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: a pass of the Gauss-Newton seed loop pays for arithmetic only.

Every epoch of the 9-state bench kernels solves the multilateration problem once (ml_estimate, kfpos_core_ml.h) to seed
the gain iteration, and the wavefront pays its slowest lane: about six passes per wavefront and epoch at ~350 fp64
instructions each. The first pass is peeled off in front of the loop -- its convergence test compares two constants --
so a pass of the loop is a sweep over the anchors, the voted convergence test and the step. Like a trip of the gain
iteration (tools/trip_loop_shape.py, which judges its loops in the same way) it is run by a lone wavefront that issues in
order: a wait for memory drains the pipeline and every branch is a VALU -> SALU hand-off, paid in every pass.

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
import sys

from kernel_text import KERNELS, arithmetic_only, indices, kernels_matching, main, mix, parsed, trip_loops

MIN_FP64 = 300
MAX_FP64 = 399
MAX_BRANCHES = 4
COPIES = 2
OPTIONS = (("--min-fp64", int, MIN_FP64), ("--max-fp64", int, MAX_FP64), ("--max-branches", int, MAX_BRANCHES),
           ("--copies", int, COPIES))
HEADING = "a pass of the Gauss-Newton seed loop pays for more than arithmetic"


def check(text, kernels=KERNELS, min_fp64=MIN_FP64, max_fp64=MAX_FP64, max_branches=MAX_BRANCHES, copies=COPIES,
          report=None):
    problems = []
    for f, ins in kernels_matching(parsed(text), kernels, problems):
        loops, cfg = trip_loops(ins, min_fp64)
        found = 0
        for loop in loops:
            idx = indices(cfg, loop[0])
            if mix(ins, idx, ("fp64",))["fp64"] > max_fp64 or any("quad_perm" in ins[i][2] for i in idx):
                continue  # a trip loop of the gain iteration, per lane or in pairs: not this rule's business
            found += 1
            problems += arithmetic_only(ins, cfg, loop, min_fp64, f"{f}: Gauss-Newton loop at {ins[idx[0]][0]:#x}",
                                        "a pass", max_branches, report)
        if found != copies:
            problems.append(f"{f}: {found} loop(s) with {min_fp64}-{max_fp64} fp64 instructions and no exchange, "
                            f"{copies} expected: where is the Gauss-Newton loop?")
    return problems


def verdict(insns, opts):
    return ("the Gauss-Newton loops of the 9-state kernels hold no memory access or wait and at most "
            f"{opts['max_branches']} branches a pass")


if __name__ == "__main__":
    main(sys.modules[__name__])
