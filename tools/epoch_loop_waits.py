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
import re
import sys

from kernel_text import KERNELS, VMEM, indices, kernels_matching, largest_loop, main, parse, parsed  # noqa: F401

MIN_DISTANCE = 300
OPTIONS = (("--min-distance", int, MIN_DISTANCE),)
HEADING = "epoch loop waits for a vector-memory operation it has just issued"


def outermost_loop(ins):
    """Instruction indices, in layout order, of the largest strongly connected component of the control-flow graph (the
    epoch loop with everything nested in it), or None when the function has no loop"""
    found = largest_loop(ins)
    return None if found is None else sorted(indices(found[4], found[0]))


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
    for f, ins in kernels_matching(parsed(text), kernels, problems):
        waits = waits_in_loop(ins)
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


def verdict(insns, opts):
    return ("no epoch loop waits for a vector-memory operation issued fewer than "
            f"{opts['min_distance']} instructions before")


if __name__ == "__main__":
    main(sys.modules[__name__])
