#!/usr/bin/env python3
"""Build-time performance rule for libkfpos_hip.so: no kernel touches scratch memory inside a loop.

Every kernel keeps its per-tag state in VGPRs / AGPRs / LDS. A scratch (private memory) access inside the epoch loop or
an iteration loop costs a memory round trip per trip with nothing to hide it behind (one wavefront per SIMD), so it is a
build error; a few values parked in scratch ONCE per launch -- the compiler does that to a lane's tag offsets across the
9-state kernel's epoch loop -- cost nothing measurable and are tolerated up to 64 bytes per lane. This is a rule about
speed, not correctness.

The check disassembles the gfx950 code object, rebuilds each kernel's control-flow graph and fails on any scratch_*
instruction in a basic block that lies on a cycle. usage: check_scratch.py LIB [--max-bytes 64] [--resource-log build.log]
                                                         [--min-occupancy 'REGEX=N' ...]
(LIB: the library, or a disassembly as .s / .txt)

--min-occupancy: kernels whose (mangled) name matches REGEX must reach N wavefronts per SIMD according to the compiler's
resource report. The kernels that serve banks with more wavefronts than the chip has SIMDs are written to share a SIMD
two at a time; two registers too many drop them to one and cost 25-40 % with every test still green (it happened: the
48-bit-covariance 16-anchor kernel, round 3), so the build checks what no parity test can.
"""
import os
import re
import sys

from kernel_text import blocks_of, components, indices, main, parsed

MAX_BYTES = 64


def occupancy(rule):
    pattern, need = rule.rsplit("=", 1)
    return pattern, int(need)


OPTIONS = (("--max-bytes", int, MAX_BYTES), ("--resource-log", str, None), ("--min-occupancy", occupancy, ()))
HEADING = None


def n_scratch(ins):
    return sum(op.startswith("scratch_") for _, op, _, _ in ins)


def scratch_in_cycles(ins):
    """Number of scratch_* instructions that lie on a cycle of the function's control-flow graph."""
    cfg = blocks_of(ins)
    return n_scratch(ins[i] for comp in components(range(len(cfg[0])), cfg[2]) for i in indices(cfg, comp))


def check(text, max_bytes=MAX_BYTES, resource_log=None, min_occupancy=(), report=None):
    """text: the disassembly or what parse() made of it. The occupancy and bytes-per-lane rules read the compiler's
    resource log; this rule has nothing to list in `report`."""
    problems = []
    for func, ins in parsed(text).items():
        inside = scratch_in_cycles(ins) if n_scratch(ins) else 0
        if inside:
            problems.append(f"{func}: {inside} scratch access(es) inside a loop")
    if resource_log and os.path.exists(resource_log):
        name, seen = None, {}
        for line in open(resource_log):
            m = re.search(r"Function Name: (\S+)", line)
            if m:
                name = m.group(1)
            m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
            if m and int(m.group(1)) > max_bytes:
                problems.append(f"{name}: {m.group(1)} bytes/lane of scratch (limit {max_bytes})")
            m = re.search(r"Occupancy \[waves/SIMD\]: (\d+)", line)
            if m and name:
                for pattern, need in min_occupancy:
                    if re.search(pattern, name):
                        seen[pattern] = seen.get(pattern, 0) + 1
                        if int(m.group(1)) < need:
                            problems.append(f"{name}: {m.group(1)} wavefront(s) per SIMD, {need} required")
        for pattern, _ in min_occupancy:
            if not seen.get(pattern):
                problems.append(f"--min-occupancy {pattern}: no kernel of that name in {resource_log}")
    elif min_occupancy:
        problems.append("--min-occupancy needs --resource-log")
    return problems


def verdict(insns, opts):
    n, rules = sum(map(n_scratch, insns.values())), len(opts["min_occupancy"])
    return (f"no kernel touches scratch inside a loop ({n} scratch instructions in the library, all outside loops)"
            + (f"; {rules} occupancy rule(s) hold" if rules else ""))


if __name__ == "__main__":
    main(sys.modules[__name__], kernels=False)
