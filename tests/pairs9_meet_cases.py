"""What tests/test_pairs9_meet_gpu.py and tests/test_pairs9_meet_emu.py share: the 12-epoch trace on which the lanes of a
9-state wavefront meet in every way the schedule of iekf9_next_meet distinguishes, the scenarios as they are read off the
solve counts ((status >> 8) & 0xFF), the seed chosen with the oracle on the CPU -- and, run as a program, the child process
that replays the trace under ONE setting of KFPOS_PAIR9_MEET / KFPOS_PAIR9 (the parent sets the environment) and writes
every byte it produced to an .npz:

    python tests/pairs9_meet_cases.py OUT.npz [SEED]

The scenarios, in the kernel's terms: a lane with a final count g runs g + 1 passes (the last finds it converged), so the
meeting after s solves finds the lanes with g >= s. "first at s": more than 32 lanes at every meeting before s, at most 32
(and somebody) at s. The trace: synth.Workload from a fixed start, whose first epochs converge in a few solves, with the
epochs' dt stretched (x 1.2 from the third epoch, x 1.4 and x 3 for the last two) so that the later ones keep more and more
lanes iterating: within 12 epochs one wavefront goes from "nobody left at 7" to "more than 32 lanes beyond 11". MARGIN
lanes are kept clear on either side of every threshold the seed is chosen by, so that a solve count that differs by one
on a lane (KFPOS_STORE_P48 against the oracle) does not move a wavefront into another scenario."""
import functools
import os
import sys

import numpy as np

import conftest  # noqa: F401  (the import paths of the suite, also where this file runs as a program)
import step_checks as sc
from roskfpos_amd.capi import st_gain_iters as gain_iters  # noqa: F401  (the tests read the solve counts with it)
from roskfpos_amd.synth import Workload

A, S = 8, 12
SPLIT = 5          # launches of 5 and 7 epochs
DT_SCALE = np.array([1, 1, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.2, 1.4, 3.0])
MARGIN = 2
SHAPES = ((64, 2), (128, 2), (101, 2), (64, 3), (128, 3), (101, 3))   # (tags, storage: 2 = mixed, 3 = p48)
NAN_TAG, NAN_T = 5, 64
SETTINGS = {"default": {}, "7,10": {"KFPOS_PAIR9_MEET": "7,10"}, "8,8": {"KFPOS_PAIR9_MEET": "8,8"},
            "1,20": {"KFPOS_PAIR9_MEET": "1,20"}, "no pairs": {"KFPOS_PAIR9": "0"}}   # default: 8,10
SCENARIOS = ("first at 7", "first at 8", "first at 9 or 10", "more than 32 until at least 11", "at most 32 by 6",
             "nobody left at 7")


def dts():
    return sc.dts(S) * DT_SCALE


def scenarios(g, margin=0):
    """g: [epoch][64] solve counts of one full wavefront -> {scenario: [epochs]}. Pairs are formed only where every lane
    runs the iteration (a count > 0 on every lane: a lane without an update leaves the step early). margin: lanes kept
    clear of 32 on either side of every threshold looked at."""
    left = np.stack([(g >= s).sum(1) for s in range(21)], 1)       # [epoch][s]: whom a meeting after s solves finds
    all_in = (g > 0).all(1)
    many, few = 33 + margin, 32 - margin                            # "more than 32" / "at most 32", margin lanes clear

    def first_at(s, by=None):
        by = by or s
        return all_in & (left[:, s - 1] >= many) & (left[:, by] <= few) & (left[:, by] > 0)

    return {
        "first at 7": np.flatnonzero(first_at(7)),
        "first at 8": np.flatnonzero(first_at(8)),
        "first at 9 or 10": np.flatnonzero(first_at(9, 10)),   # more than 32 at 8, at most 32 by 10
        "more than 32 until at least 11": np.flatnonzero(all_in & (left[:, 10] >= many)),
        "at most 32 by 6": np.flatnonzero(all_in & (left[:, 6] <= few) & (left[:, 7] > 0)),
        "nobody left at 7": np.flatnonzero(all_in & (left[:, 7] == 0)),
    }


def oracle_run(T, seed):
    """the trace through the oracle alone, f32 measurements as the two storage modes hold them ->
    (poses [S][3][T], status [S][T])"""
    w = Workload(T, A, seed=seed)
    r = sc.Trace(w, S, 2, "cpu", gaps=True).r_host
    poses, status = sc.oracle_run(w, r, w.err_est(), dts(), real=np.float32, init=w.init_positions())[:2]
    return poses.transpose(0, 2, 1), status


@functools.lru_cache(maxsize=None)
def seed():
    """the first workload seed for which the ORACLE sees every scenario in the first wavefront (tags 0 .. 63: a tag's trace
    does not depend on how many tags the workload has, so the seed serves every shape), MARGIN lanes clear of every
    threshold"""
    return sc.first_seed(range(1, 41), lambda sd: all(len(v) for v in scenarios(gain_iters(oracle_run(64, sd)[1]),
                                                                              MARGIN).values()),
                         "every meeting scenario in one wavefront")


# ---- the child process: one setting, every shape

def _replay(T, storage, sd):
    """-> {name: array} for one shape: the 12 epochs as one launch, as 5 + 7, and as single calls (whose status words
    carry every epoch's solve counts). The banks keep the setting this process was started under."""
    w = Workload(T, A, seed=sd)
    tr = sc.Trace(w, S, storage, gaps=True)
    d = dts()
    out = {}

    def bank():
        return sc.bank(w, T, storage, pairs=os.environ.get("KFPOS_PAIR9"), meet=os.environ.get("KFPOS_PAIR9_MEET"))

    def keep(name, res):
        for part, a in zip(sc.Run._fields, res):
            out[f"{T}/{storage}/{name}/{part}"] = np.ascontiguousarray(a)

    for name, run in (("one launch", sc.fused), ("5 + 7", functools.partial(sc.fused_split, split=SPLIT)),
                      ("single calls", sc.single_calls)):
        b = bank()
        keep(name, run(b, tr, d, S))
        b.close()
    if (T, storage) in ((NAN_T, 2), (NAN_T, 3)):      # a NaN wave-mate: 5 epochs, the position of one tag made NaN, 7 epochs
        for name, run in (("nan, one launch", sc.fused), ("nan, single calls", sc.single_calls)):
            b = bank()
            sc.fused(b, tr, d, SPLIT)
            if name == "nan, one launch":
                x, P, fl = b.get_state()
                x[NAN_TAG, :3] = np.nan
            b.set_state(x, P, fl)                      # (the single calls start from the launch's state)
            keep(name, run(b, tr, d, S - SPLIT, SPLIT))
            b.close()
    return out


def main(path, sd=None):
    sd = seed() if sd is None else sd
    out = {"seed": np.array(sd)}
    for T, storage in SHAPES:
        out.update(_replay(T, storage, sd))
    np.savez(path, **out)


if __name__ == "__main__":
    main(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else None)
