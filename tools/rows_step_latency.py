"""Latency of a row-list round against the whole-bank round (profiles/HISTORY.md).

For banks of 65 536 and 1 048 576 tags x 8 anchors, 6-state and 9-state, MIXED storage, and n reporters out of T
(n in {64, 1 024, 16 384, 65 536, T/4, T}, rows spread over the bank), the median host time, in one process, of
    rows_sync    kfpos_step_toa_rows / kfpos_step_toa_imu_rows: pageable arrays of the n listed tags, returns when done
    rows_slots   kfpos_slot_submit_rows pipelined over the three slots (records already in the slot): time per round
    dense_sync   kfpos_step_toa / kfpos_step_toa_imu with dt < 0 for the T - n others
    dense_slots  kfpos_slot_submit with KFPOS_SLOT_DT_PER_TAG pipelined over the slots: time per round
The dense figures are the baseline: that path is the code as it was before the row-list calls existed.

    python tools/rows_step_latency.py --out profiles/rows_step_latency.json [--reps 30]
    python tools/rows_step_latency.py --kernels-only     # a few rounds of each n, for a kernel trace
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from roskfpos_amd import capi  # noqa: E402
from roskfpos_amd.synth import Workload  # noqa: E402

CONFIGS = [
    dict(name="toa6_mixed_65536", model=capi.MODEL_TOA, T=1 << 16),
    dict(name="imu9_mixed_65536", model=capi.MODEL_TOA_IMU, T=1 << 16),
    dict(name="toa6_mixed_1048576", model=capi.MODEL_TOA, T=1 << 20),
    dict(name="imu9_mixed_1048576", model=capi.MODEL_TOA_IMU, T=1 << 20),
]


def ns_of(T):
    return sorted({n for n in (64, 1024, 16384, 65536, T // 4, T) if n <= T})


def stats(samples):
    a = np.asarray(samples) * 1e6
    return dict(n=int(a.size), median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)),
                p90_us=float(np.percentile(a, 90)))


class Case:
    def __init__(self, cfg):
        self.T, self.imu = cfg["T"], cfg["model"] == capi.MODEL_TOA_IMU
        T = self.T
        w = Workload(T, 8)
        self.bank = capi.KfposBank(cfg["model"], T, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions())
        self.r, self.err = w.ranges_mm(1), w.err_est(np.float32)
        self.acc, self.cov = w.accel(1, np.float32), w.accel_cov(np.float32)
        self.dense_sync(np.full(T, 0.1))  # every tag has started
        self.NS = self.bank.lib.kfpos_slot_count(self.bank._h)
        self.kind = capi.SLOT_TOA_IMU if self.imu else capi.SLOT_TOA
        for k in range(self.NS):  # the whole-bank slots hold a complete epoch
            v = self.bank.slot_acquire(k)
            v["range_mm"][:], v["err_est"][:] = self.r.T, self.err.T
            v["accel"][:], v["cov"][:] = self.acc.T, self.cov.T

    def dense_sync(self, dts):
        b = self.bank
        b.step_toa_imu(self.r, self.err, self.acc, self.cov, dts) if self.imu else b.step_toa(self.r, self.err, dts)

    def rows_sync(self, rows, part):
        b = self.bank
        if self.imu:
            b.step_toa_imu_rows(rows, part[0], part[1], part[2], part[3], 0.05)
        else:
            b.step_toa_rows(rows, part[0], part[1], 0.05)

    def pipelined(self, acquire, submit, reps):
        """per-round host time of reps rounds submitted back to back over the slots (includes the final wait)"""
        for s in range(2 * self.NS):
            acquire(s % self.NS)
            submit(s % self.NS)
        for k in range(self.NS):
            self.bank.slot_wait(k)
        out = []
        for _ in range(5):
            t0 = time.perf_counter()
            for s in range(reps):
                acquire(s % self.NS)
                submit(s % self.NS)
            for k in range(self.NS):
                self.bank.slot_wait(k)
            out.append((time.perf_counter() - t0) / reps)
        return out

    def measure(self, n, reps, kernels_only=False):
        T, b = self.T, self.bank
        rows = np.sort(np.random.default_rng(1).choice(T, size=n, replace=False)).astype(np.int32)  # spread over the bank
        part = [self.r[rows], self.err[rows], self.acc[rows], self.cov[rows]]
        dts = np.full(T, -1.0)
        dts[rows] = 0.05
        flags = self.kind | capi.SLOT_NO_POSE

        def rows_fill(k):
            v = b.slot_acquire_rows(k)
            v["rows"][:n] = rows
            v["range_mm"][:n], v["err_est"][:n] = part[0], part[1]
            v["accel"][:n], v["cov"][:n] = part[2], part[3]

        def dense_fill(k):
            b.slot_acquire(k)["dt"][:] = dts

        for k in range(self.NS):
            rows_fill(k)
        if kernels_only:
            for _ in range(5):
                self.rows_sync(rows, part)
            return None
        entry = dict(n=n, fraction=n / T)
        t_rows, t_dense = [], []
        for _ in range(3):
            self.rows_sync(rows, part)
            self.dense_sync(dts)
        for _ in range(reps):  # alternating: both see the same machine
            t0 = time.perf_counter()
            self.rows_sync(rows, part)
            t1 = time.perf_counter()
            self.dense_sync(dts)
            t2 = time.perf_counter()
            t_rows.append(t1 - t0)
            t_dense.append(t2 - t1)
        entry["rows_sync"], entry["dense_sync"] = stats(t_rows), stats(t_dense)
        entry["rows_slots"] = stats(self.pipelined(b.slot_acquire_rows, lambda k: b.slot_submit_rows(k, flags, n, 0.05), reps))
        for k in range(self.NS):
            dense_fill(k)
        entry["dense_slots"] = stats(self.pipelined(
            b.slot_acquire, lambda k: b.slot_submit(k, flags | capi.SLOT_DT_PER_TAG, 0.05), reps))
        return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--configs", default=",".join(c["name"] for c in CONFIGS))
    a = ap.parse_args()
    results = []
    for cfg in CONFIGS:
        if cfg["name"] not in a.configs.split(","):
            continue
        case = Case(cfg)
        per_n = []
        for n in ns_of(cfg["T"]):
            e = case.measure(n, a.reps, a.kernels_only)
            if e is None:
                continue
            per_n.append(e)
            print(f"{cfg['name']} n={n:8d} ({e['fraction']:.4f})  rows sync {e['rows_sync']['median_us']:10.1f} us  "
                  f"slots {e['rows_slots']['median_us']:10.1f} us | dense sync {e['dense_sync']['median_us']:10.1f} us  "
                  f"slots {e['dense_slots']['median_us']:10.1f} us", flush=True)
        # the smallest measured fraction from which on the whole-bank slot round is the cheaper one
        cross = next((e["fraction"] for e in per_n if e["dense_slots"]["median_us"] < e["rows_slots"]["median_us"]), None)
        results.append(dict(config=cfg["name"], tags=cfg["T"], per_n=per_n, dense_slots_cheaper_from_fraction=cross))
        case.bank.close()
    if a.kernels_only:
        return
    res = dict(what="row-list rounds against whole-bank rounds with dt < 0 for the others, host clock, MIXED storage, 8 anchors; "
                    "slots: per round of a back-to-back sequence over the three slots, KFPOS_SLOT_NO_POSE",
               reps=a.reps, results=results)
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
