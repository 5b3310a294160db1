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
import sys

from kernel_text import KERNELS, TRIP_FP64, arithmetic_only, indices, kernels_matching, main, mix, parsed, trip_loops
from kernel_text import is_branch, parse, usual_path  # noqa: F401  (for who looks at a kernel through this module)

MIN_FP64 = TRIP_FP64
MAX_FP64 = 700
MAX_BRANCHES = 4
OPTIONS = (("--min-fp64", int, MIN_FP64), ("--max-fp64", int, MAX_FP64), ("--max-branches", int, MAX_BRANCHES))
HEADING = "a trip of the 9-state gain iteration pays for more than arithmetic"


def check(text, kernels=KERNELS, min_fp64=MIN_FP64, max_branches=MAX_BRANCHES, report=None, max_fp64=MAX_FP64):
    problems = []
    for f, ins in kernels_matching(parsed(text), kernels, problems):
        loops, cfg = trip_loops(ins, min_fp64)
        if not loops:
            problems.append(f"{f}: no loop with {min_fp64} fp64 instructions: where is the trip?")
        looked = []
        for loop in loops:
            idx = indices(cfg, loop[0])
            whole = mix(ins, idx, ("fp64", "saveexec"))
            aside = ("the pairs' loop" if any("quad_perm" in ins[i][2] for i in idx) else
                     "the (I + M B) form" if whole["fp64"] > max_fp64 else None)
            looked.append((loop, ins[idx[0]][0], whole["saveexec"], aside))
        judged = [saveexec for _, _, saveexec, aside in looked if aside is None]
        if loops and not judged:
            problems.append(f"{f}: no trip loop of the information form")
        elif judged and min(judged) > 1:
            problems.append(f"{f}: no fast form: every trip loop has more than one masked region (s_and_saveexec)")
        for loop, address, saveexec, aside in looked:
            found = arithmetic_only(ins, cfg, loop, min_fp64, f"{f}: loop at {address:#x}", "a trip",
                                    max_branches if saveexec <= 1 else max_branches + 1, report,
                                    f" ({aside}: listed only)" if aside else "")
            if aside is None:
                problems += found
    return problems


def verdict(insns, opts):
    return ("the trip loops of the 9-state gain iteration hold no memory access or wait and at most "
            f"{opts['max_branches']} branches a trip")


if __name__ == "__main__":
    main(sys.modules[__name__])
