#!/usr/bin/env python3
"""Where the lanes of a wavefront should meet to hand the 9-state gain iteration's tail to pairs, on the trace bench.py
times: solve counts per tag of synth.Workload(65 536 tags, 8 anchors), epochs 50 .. 249 (the timed ones behind 50
warm-up epochs), from the host build of the kernel body (tests/emu/libkfpos_emu.so, the epoch in registers; f32
measurements as KFPOS_STORE_MIXED stores them). No GPU.

Per wavefront (64 consecutive tags) and epoch, two histograms:
  * switch_iteration_L32_hist, as tools/exp/iter_hist.py lists it: the first k at which at most 32 lanes have a solve
    count ABOVE k;
  * first_meeting_that_hands_over_hist, in the kernel's terms: the first solve count s at which a meeting finds at
    most 32 lanes. A lane whose final count is g runs g + 1 passes (the last one finds it converged and solves nothing;
    a capped lane runs 20), so after s passes the lanes with g >= s are still iterating -- that is what the ballot of
    iekf9_info counts at the meeting `stop = s`. Hence s = k + 1: the wavefronts iter_hist.py lists under 7 can hand
    over at the meeting after 8 solves and no earlier.
From the counts, exactly: the trips every schedule (first, dense_until) of iekf9_next_meet runs per lane and on pairs, its
meetings, and its price against 8, 12, 16, 20 (profiles/HISTORY.md, "Where the lanes meet").

    python tools/exp/meet_hist.py [--tags 65536] [--first-epoch 50] [--epochs 200] [--procs N] > profiles/NAME.json
"""
import argparse
import json
import multiprocessing
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))   # (tests/impls.py imports the oracle beside the host build)

PER_LANE, PAIR, CAP = 534, 420, 20   # instructions of a per-lane trip and of a pairs' trip; the cap of the iteration


def solves(job):
    lo, n, first, epochs = job
    from cases import Case
    from impls import EmuStaticImpl
    from roskfpos_amd.synth import Workload
    w = Workload(n, 8, tag0=lo)
    f = EmuStaticImpl(Case("meet_hist", 1, 8, T=n), w, w.init_positions())
    err = w.err_est(np.float32).astype(np.float64)
    cov = w.accel_cov(np.float32).astype(np.float64)
    out = np.zeros((epochs, n), dtype=np.int8)
    for s in range(first + epochs):
        st = f.fused(w.ranges_mm(s), err, w.accel(s, np.float32).astype(np.float64), cov, w.dt_of(s))
        if s >= first:
            out[s - first] = (np.asarray(st).astype(np.uint32) >> 8) & 0xFF
    return out


def meetings(first, dense_until):
    out, stop = [], first
    while True:
        out.append(stop)
        if stop >= CAP:
            return out
        stop = min(stop + (1 if stop < dense_until else 4), CAP)


def walk(g, points):
    """g: [wavefront-epochs][64] final solve counts -> (per-lane trips, pairs' trips, meetings) of each under a schedule,
    as iekf9_info walks it: the wavefront runs min(g + 1, CAP) passes of its slowest lane in all; at the meeting `stop`
    the lanes with g >= stop are left (none at the cap: nobody goes beyond it); nobody left ends the iteration, at most
    32 hand over to the pairs, more go on per lane to the next meeting."""
    n = g.shape[0]
    passes = np.minimum(g + 1, CAP).max(1)
    left = np.stack([(g >= s).sum(1) if s < CAP else np.zeros(n, dtype=np.int64) for s in range(CAP + 1)], 1)
    hand = np.full(n, CAP)                 # the meeting that ends the per-lane trips
    met = np.zeros(n, dtype=np.int64)
    open_ = np.ones(n, dtype=bool)
    for p in points:
        met += open_
        done = open_ & (left[:, p] <= 32)  # handed over, or nobody left
        hand[done] = p
        open_ &= ~done
    per_lane = np.minimum(passes, hand)
    return per_lane, passes - per_lane, met


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tags", type=int, default=65536)
    ap.add_argument("--first-epoch", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=200)
    ap.add_argument("--procs", type=int, default=min(32, os.cpu_count() or 1))
    ap.add_argument("--meeting-cost", type=float, default=80.0,
                    help="quad-cycles of a meeting that does not hand over (measured: 7,10 against 8,10 on MI355X)")
    a = ap.parse_args()
    chunk = 1024
    jobs = [(lo, min(chunk, a.tags - lo), a.first_epoch, a.epochs) for lo in range(0, a.tags, chunk)]
    with multiprocessing.Pool(a.procs) as pool:
        its = np.concatenate(pool.map(solves, jobs, chunksize=1), axis=1).astype(np.int32)
    T = a.tags
    out = {"trace": f"synth.Workload({T}, 8), epochs {a.first_epoch} .. {a.first_epoch + a.epochs - 1}, host build of "
                    "the kernel body (epoch in registers), f32 measurements",
           "tags": T, "epochs": int(its.shape[0]), "hist": np.bincount(its.ravel(), minlength=21).tolist(),
           "mean": float(its.mean())}
    wv = its.reshape(its.shape[0], T // 64, 64)
    out["wavefront_epochs"] = int(wv.shape[0] * wv.shape[1])
    out["mean_wave_max"] = float(wv.max(2).mean())
    active = np.stack([(wv > k).sum(2) for k in range(21)], 0)   # [k][epoch][wave] lanes with more than k solves
    out["mean_active_after_k"] = [float(active[k].mean()) for k in range(21)]
    out["switch_iteration_L32_hist"] = np.bincount((active <= 32).argmax(0).ravel(), minlength=21).tolist()
    g = wv.reshape(-1, 64)
    left = np.stack([(g >= s).sum(1) for s in range(21)], 0)     # [s][wavefront-epoch] lanes a meeting at s finds
    out["first_meeting_that_hands_over_hist"] = np.bincount((left <= 32).argmax(0), minlength=21).tolist()
    m = a.meeting_cost
    base = walk(g, meetings(8, 8))
    table = {}
    for f0 in range(5, 11):
        for d in range(f0, 14):
            pl, pr, met = walk(g, meetings(f0, d))
            table[f"{f0},{d}"] = {
                "per_lane_trips": round(float(pl.mean()), 4), "pairs_trips": round(float(pr.mean()), 4),
                "meetings": round(float(met.mean()), 4),
                "gain_over_8_8": round(float(PER_LANE * (base[0] - pl).mean() + PAIR * (base[1] - pr).mean()
                                             + m * (base[2] - met).mean()), 1)}
    out["meeting_cost_assumed"] = m
    out["per_lane_trip_instructions"], out["pairs_trip_instructions"] = PER_LANE, PAIR
    out["schedules"] = table      # gain_over_8_8: instructions (about quad-cycles) per wavefront-epoch, positive = cheaper
    out["best"] = max(table, key=lambda k: table[k]["gain_over_8_8"])
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
