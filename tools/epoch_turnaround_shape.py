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
import sys

from kernel_text import KERNELS, indices, is_copy, kernels_matching, largest_loop, main, mix, parsed

MAX_COPIES = 32
OPTIONS = (("--max-copies", int, MAX_COPIES),)
HEADING = "the 9-state epoch loop carries too much across its back-edge in registers"
COLUMNS = ("instructions", "fp64", "valu_other", "agpr_read", "agpr_write", "v_mov", "lane_read", "lane_write", "ds",
           "vmem", "salu", "branches")


def check(text, kernels=KERNELS, max_copies=MAX_COPIES, report=None):
    problems = []
    for f, ins in kernels_matching(parsed(text), kernels, problems):
        found = largest_loop(ins)
        if found is None:
            problems.append(f"{f}: no loop")
            continue
        loop, headers, latches, outside, cfg = found
        address = lambda b: ins[cfg[0][b]][0]
        if report is not None:
            report.append(f"{f}: epoch loop of {len(loop)} blocks, {len(outside)} of them outside nested loops")
            report.append("  " + "address".rjust(9) + " " + " ".join(c.rjust(12) for c in COLUMNS))
            for b in outside:
                m = mix(ins, indices(cfg, [b]), COLUMNS)
                mark = " header" if b in headers else " latch" if b in latches else ""
                report.append(f"  {address(b):#9x} " + " ".join(str(n).rjust(12) for n in m.values()) + mark)
            total = mix(ins, indices(cfg, outside), COLUMNS)
            report.append("  " + "total".rjust(9) + " " + " ".join(str(n).rjust(12) for n in total.values()))
        copies = sum(is_copy(ins[i][1]) for i in indices(cfg, latches))
        where = ", ".join(f"{address(b):#x}" for b in latches)
        if report is not None:
            report.append(f"{f}: latch block(s) at {where}: {copies} register copies")
        if copies > max_copies:
            problems.append(f"{f}: latch block(s) at {where}: {copies} register copies (maximum {max_copies})")
    return problems


def verdict(insns, opts):
    return f"the latch of the 9-state epoch loop holds at most {opts['max_copies']} register copies"


if __name__ == "__main__":
    main(sys.modules[__name__])
