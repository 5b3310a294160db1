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
import sys

from kernel_text import KERNELS, arithmetic_only, indices, kernels_matching, main, mix, parsed, trip_loops

MIN_FP64 = 300
MAX_BRANCHES = 4
OPTIONS = (("--min-fp64", int, MIN_FP64), ("--max-branches", int, MAX_BRANCHES))
HEADING = "a pair trip of the 9-state gain iteration pays for more than arithmetic"


def is_exchange(args):
    return "quad_perm" in args


def check(text, kernels=KERNELS, min_fp64=MIN_FP64, max_branches=MAX_BRANCHES, report=None):
    problems = []
    for f, ins in kernels_matching(parsed(text), kernels, problems):
        loops, cfg = trip_loops(ins, min_fp64)
        found = []
        for loop in loops:
            idx = indices(cfg, loop[0])
            if any(is_exchange(ins[i][2]) for i in idx):
                found.append((loop, ins[idx[0]][0], mix(ins, idx, ("saveexec",))["saveexec"] <= 1))
        if not found:
            problems.append(f"{f}: no loop with {min_fp64} fp64 instructions and a quad_perm exchange: where are the pairs?")
        elif not any(fast for _, _, fast in found):
            problems.append(f"{f}: no fast form: every pairs' loop has more than one masked region (s_and_saveexec)")
        for loop, address, fast in found:
            problems += arithmetic_only(ins, cfg, loop, min_fp64, f"{f}: pairs' loop at {address:#x}", "a pair trip",
                                        max_branches if fast else max_branches + 1, report,
                                        " (fast form)" if fast else " (per-lane form)")
    return problems


def verdict(insns, opts):
    return ("the pairs' loops of the 9-state gain iteration hold no memory access or wait and at most "
            f"{opts['max_branches']} branches a trip")


if __name__ == "__main__":
    main(sys.modules[__name__])
