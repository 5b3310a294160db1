#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: between the unpack of an epoch and the first trip loop of the gain
iteration, the 9-state bench kernel runs selects, not masked regions.

That stretch holds the working weights (set_weights_ml: 1 / errorEstimation or 0 for an absent range), the Gauss-Newton
solve of the seed, the test for an errorEstimation of exactly 0 (ml_covariance_throws) and the weights of the update
(set_weights_iekf). Apart from the solve it is a handful of comparisons and selects per anchor. Written with conditional
expressions whose arms compute something, or with a short-circuit, it compiles to one masked region per anchor -- an
`s_and_saveexec`, an `s_cbranch_execz` and an `s_or exec` around a few instructions, nested seven deep for the
short-circuit -- and a wavefront that has its SIMD to itself pays every one of them in every epoch.

For every listed kernel this finds the epoch loop (the largest cycle of the control-flow graph) and its blocks outside
nested loops, as tools/epoch_turnaround_shape.py does, then
  * the unpack block: the first of those blocks, in layout order, with at least --min-loads (8) vector-memory
    instructions (the read of the epoch's ranges and sample: 16),
  * the first trip loop: the trip loop of tools/trip_loop_shape.py (an innermost cycle with at least 400 fp64
    instructions, whatever its form) that starts first behind the unpack block,
and counts the `s_cbranch_execz` of the blocks outside nested loops that lie between the two in layout order, with the
one that ends the unpack block if it ends in one (the first masked region opens there). It prints
that count with the instruction mix of the stretch and fails when the count is above --max-execz (12).

usage: epoch_weights_branches.py LIB [--kernel REGEX ...] [--max-execz 12] [--min-loads 8] [--quiet]
(LIB: the library, or a disassembly as .s / .txt; --quiet: the verdict only)
"""
import sys

from kernel_text import KERNELS, VMEM, indices, kernels_matching, largest_loop, main, mix, parsed, trip_loops

MAX_EXECZ = 12
MIN_LOADS = 8
OPTIONS = (("--max-execz", int, MAX_EXECZ), ("--min-loads", int, MIN_LOADS))
HEADING = "the weights of a 9-state epoch are masked regions again, not selects"
COLUMNS = ("instructions", "fp64", "valu_other", "agpr_read", "agpr_write", "v_mov", "lane_read", "lane_write", "ds",
           "vmem", "salu", "branches", "saveexec", "mem_waits")


def stretch(ins, min_loads=MIN_LOADS):
    """(blocks of the stretch, address of the unpack block, address of the first trip loop, cfg), or a string that says
    what is missing"""
    found = largest_loop(ins)
    if found is None:
        return "no loop"
    _, _, _, outside, cfg = found
    starts = cfg[0]
    loads = lambda b: sum(ins[i][1].startswith(VMEM) for i in indices(cfg, [b]))
    unpack = next((b for b in sorted(outside) if loads(b) >= min_loads), None)
    if unpack is None:
        return f"no block of the epoch loop with {min_loads} vector-memory instructions: where is the unpack?"
    loops, _ = trip_loops(ins)
    heads = sorted(min(comp) for comp, _ in loops if min(comp) > unpack)
    if not heads:
        return "no trip loop behind the unpack block"
    between = [b for b in sorted(outside) if unpack < b < heads[0]]
    return between, ins[starts[unpack]][0], ins[starts[heads[0]]][0], cfg


def check(text, kernels=KERNELS, max_execz=MAX_EXECZ, min_loads=MIN_LOADS, report=None):
    problems = []
    for f, ins in kernels_matching(parsed(text), kernels, problems):
        found = stretch(ins, min_loads)
        if isinstance(found, str):
            problems.append(f"{f}: {found}")
            continue
        between, a_unpack, a_trip, cfg = found
        idx = indices(cfg, between)
        last_of_unpack = max(i for i in range(len(ins)) if ins[i][0] < ins[idx[0]][0]) if between else None
        execz = sum(ins[i][1] == "s_cbranch_execz" for i in idx)
        execz += last_of_unpack is not None and ins[last_of_unpack][1] == "s_cbranch_execz"
        if report is not None:
            report.append(f"{f}: unpack block at {a_unpack:#x}, first trip loop at {a_trip:#x}, {len(between)} blocks "
                          "outside nested loops between them: "
                          + ", ".join(f"{c} {n}" for c, n in mix(ins, idx, COLUMNS).items()))
            report.append(f"{f}: {execz} s_cbranch_execz between the unpack and the first trip loop")
        if execz > max_execz:
            problems.append(f"{f}: {execz} s_cbranch_execz between the unpack block at {a_unpack:#x} and the first "
                            f"trip loop at {a_trip:#x} (maximum {max_execz})")
    return problems


def verdict(insns, opts):
    return f"at most {opts['max_execz']} s_cbranch_execz between the unpack of a 9-state epoch and its first trip loop"


if __name__ == "__main__":
    main(sys.modules[__name__])
