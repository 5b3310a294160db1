#!/usr/bin/env python3
"""What can the pairs' tail of the 9-state gain iteration (iekf9_pairs, KFPOS_PAIR9=1) gain, and what does its hand-over
cost? Timing variants of the source of the commit BEFORE the tail was rebuilt (pass that commit's roskfpos_amd/csrc and
include as SRC_ROOT); only their duration is of interest, nothing here ships:
  nolds      the pair loop reads nothing from LDS: B^-1, Sigma^-1 and the lane's four anchors are read once in front of
             the loop and pinned there, the reads have arrived before the first trip, no sched_group_barrier
  handover   the hand-over in both directions, but no pair trip is ever run (the loop's condition is false at run time):
             the iteration then stops where the lanes met -- wrong results by construction
Output: tools/exp/_build/pairs_tail/<name>/libkfpos_hip.so (git-ignored).

usage: pairs_tail_build.py SRC_ROOT [nolds] [handover]
"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tools", "exp", "_build", "pairs_tail")


def rep(s, a, b):
    assert s.count(a) == 1, a
    return s.replace(a, b)


IN_LOOP = """        double bb[12];
        const int z = kf_opaque_zero();
        bb[0] = b0[0]; bb[1] = b0[1]; bb[2] = b0[2];
        KFPOS_UNROLL
        for (int k = 3; k < 12; ++k) bb[k] = b4[k + z];
        Iekf9Parked pk;
        iekf9_fetch<true, DIAG>(cbinv, binv_stride, ci, pk);
"""
IN_FRONT = """    double bb[12];
    KFPOS_UNROLL
    for (int k = 0; k < 12; ++k) { bb[k] = b4[k]; kf_pin(bb[k]); }
    Iekf9Parked pk;
    iekf9_fetch<false, DIAG, true>(cbinv, binv_stride, ci, pk);
    KFPOS_UNROLL
    for (int k = 0; k < 21; ++k) kf_pin(pk.binv[k]);
    __builtin_amdgcn_s_waitcnt(0xC07F);
"""
WHILE = "    while (act) { /* (both lanes of a pair leave together) */\n"


def nolds(s):
    s = rep(s, IN_LOOP, "")
    s = rep(s, "        iekf9_spread_reads();\n", "")
    return rep(s, WHILE, IN_FRONT + WHILE)


def handover(s):
    return rep(s, WHILE, "    while (act && kf_opaque_zero()) {\n")


def variant(src_root, name, edit):
    d = os.path.join(OUT, name)
    shutil.rmtree(d, ignore_errors=True)
    csrc = os.path.join(d, "a", "csrc")  # the sources include ../../include/kfpos.h
    os.makedirs(csrc)
    shutil.copytree(os.path.join(src_root, "include"), os.path.join(d, "include"))
    src = os.path.join(src_root, "roskfpos_amd", "csrc")
    for f in os.listdir(src):
        if f.endswith((".h", ".hip", ".inc", ".cpp")) or f == "Makefile":
            shutil.copy(os.path.join(src, f), csrc)
    p = os.path.join(csrc, "kfpos_core_imu9.h")
    text = edit(open(p).read())
    open(p, "w").write(text)
    subprocess.check_call(["make", "-s", "-j", "16", "-C", csrc, "libkfpos_hip.so"])
    shutil.copy(os.path.join(csrc, "libkfpos_hip.so"), os.path.join(d, "libkfpos_hip.so"))
    shutil.rmtree(os.path.join(d, "a"))
    shutil.rmtree(os.path.join(d, "include"))
    print("built", os.path.join(d, "libkfpos_hip.so"))


if __name__ == "__main__":
    which = sys.argv[2:] or ["nolds", "handover", "parent"]
    for name, edit in (("parent", lambda s: s), ("nolds", nolds), ("handover", handover)):
        if name in which:
            variant(sys.argv[1], name, edit)
