#!/usr/bin/env python3
"""The build-time performance rules of libkfpos_hip.so, all of them, on one disassembly: what `make check` runs.

They guard what no parity test can see; each is a script of its own under tools/, with the reasons
and its thresholds in its docstring, and this is the list:
  check_scratch.py           no kernel touches scratch inside a loop, none parks more than 64 bytes a lane there, and the
                             kernels written to share a SIMD two at a time still fit twice (--min-occupancy)
  epoch_loop_waits.py        the epoch loop of the 9-state kernels waits for no load or store it has only just issued
  trip_loop_shape.py         a trip of their gain iteration holds no memory access, no wait for one and no more branches
                             than agreed
  pairs_loop_shape.py        nor does a trip of the pairs' loop behind it
  ml_loop_shape.py           nor a pass of the Gauss-Newton loop that seeds it
  epoch_turnaround_shape.py  the latch of that epoch loop copies no more registers than position, velocity and a few
                             words account for: no covariance crosses the back-edge in registers
  epoch_weights_branches.py  the weights of an epoch, between its unpack and the first trip loop, are selects, not one
                             masked region per anchor
Every rule prints its verdict, or its heading and what breaks it; the exit status is 1 if one broke.

usage: check_kernels.py LIB --resource-log LOG [--min-occupancy 'REGEX=N' ...]
(LIB: the library, or a disassembly as .s / .txt; LOG: the compiler's resource report, for check_scratch.py)
"""
import argparse
import sys

import check_scratch
import epoch_loop_waits
import epoch_turnaround_shape
import epoch_weights_branches
import ml_loop_shape
import pairs_loop_shape
import trip_loop_shape
from kernel_text import defaults, parse, read, run

RULES = (check_scratch, epoch_loop_waits, trip_loop_shape, pairs_loop_shape, ml_loop_shape, epoch_turnaround_shape,
         epoch_weights_branches)

if __name__ == "__main__":
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("lib", metavar="LIB")
    p.add_argument("--resource-log", required=True)
    p.add_argument("--min-occupancy", type=check_scratch.occupancy, action="append", default=[])
    args = p.parse_args()
    insns = parse(read(args.lib))
    given = {check_scratch: {"resource_log": args.resource_log, "min_occupancy": tuple(args.min_occupancy)}}
    held = [run(rule, insns, dict(defaults(rule.OPTIONS), **given.get(rule, {})), quiet=True) for rule in RULES]
    sys.exit(0 if all(held) else 1)
