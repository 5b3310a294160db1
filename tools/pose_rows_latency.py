"""Latency of a publish tick: kfpos_get_pose_rows for n rows against kfpos_get_pose_each for the whole bank (DESIGN.md
section 6 "Pose for a row list", profiles/HISTORY.md).

Bank: 65 536 tags x 8 anchors, 9-state, MIXED storage, stepped a few epochs. Host clock around each synchronous call
(both end in a device synchronise), after warm-up, through the C ABI with preallocated output arrays (so that neither
route pays for numpy allocations), the two routes ALTERNATING in one process: one whole-bank call, one row-list call, and
so on. n in {64, 655, 6 554, 65 536} = 0.1 %, 1 %, 10 %, 100 % of the bank; the rows are spread over the bank (a stride
that is odd, so they are distinct), not contiguous; dt_ahead is per entry on both routes.

    python tools/pose_rows_latency.py --out profiles/pose_rows_latency.json [--reps 200]

The JSON also records the crossover: the n / T at which the row-list call's median reaches the whole-bank call's,
interpolated (log n, log t) between the two measured n around it; null when the row-list call stays below (or above) the
whole-bank call at every measured n.
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

T, A, EPOCHS = 1 << 16, 8, 4
NS = (64, 655, 6554, 65536)


def stats(samples):
    a = np.asarray(samples) * 1e6
    return dict(n=int(a.size), median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)),
                p90_us=float(np.percentile(a, 90)), min_us=float(a.min()), max_us=float(a.max()))


def timed(fn):
    t0 = time.perf_counter()
    rc = fn()
    dt = time.perf_counter() - t0
    assert rc == 0, rc
    return dt


def crossover(per_n):
    """n / T where the row-list median meets the whole-bank median, or None"""
    pts = [(e["n"], e["rows"]["median_us"] - e["whole_bank"]["median_us"], e["rows"]["median_us"], e["whole_bank"]["median_us"])
           for e in per_n]
    for (n0, d0, r0, w0), (n1, d1, r1, w1) in zip(pts, pts[1:]):
        if d0 < 0 <= d1:
            # log-log line through the two row-list medians, against the (flat) whole-bank median between them
            slope = (np.log(r1) - np.log(r0)) / (np.log(n1) - np.log(n0))
            target = np.log(0.5 * (w0 + w1))
            n_x = float(np.exp(np.log(n0) + (target - np.log(r0)) / slope))
            return min(max(n_x, n0), n1) / T
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    a = ap.parse_args()
    w = Workload(T, A)
    real = np.float32
    b = capi.KfposBank(capi.MODEL_TOA_IMU, T, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions())
    for s in range(EPOCHS):
        b.step_toa_imu(w.ranges_mm(s), w.err_est(real), w.accel(s, real), w.accel_cov(real), w.dt_of(s))
    lib, h = b.lib, b._h
    ahead = np.full(T, 0.02)
    pos, cov, vel, st = np.zeros((T, 3)), np.zeros((T, 9)), np.zeros((T, 3)), np.zeros(T, dtype=np.uint32)
    rpos, rcov, rvel, rst = np.zeros((T, 3)), np.zeros((T, 9)), np.zeros((T, 3)), np.zeros(T, dtype=np.uint32)

    def whole():
        return lib.kfpos_get_pose_each(h, ahead.ctypes.data, pos.ctypes.data, cov.ctypes.data, vel.ctypes.data, st.ctypes.data)

    per_n = []
    for n in NS:
        rows = (np.arange(n, dtype=np.int64) * 16411 % T).astype(np.int32)  # 16411 is odd: n <= T distinct rows
        assert np.unique(rows).size == n
        d = np.ascontiguousarray(ahead[rows])

        def listed():
            return lib.kfpos_get_pose_rows(h, rows.ctypes.data, n, d.ctypes.data, n, rpos.ctypes.data, rcov.ctypes.data,
                                           rvel.ctypes.data, rst.ctypes.data)

        for _ in range(5):
            assert whole() == 0 and listed() == 0
        # the two routes agree before they are timed
        assert np.array_equal(rpos[:n], pos[rows], equal_nan=True) and np.array_equal(rcov[:n], cov[rows], equal_nan=True)
        assert np.array_equal(rvel[:n], vel[rows], equal_nan=True) and np.array_equal(rst[:n], st[rows])
        t_whole, t_rows = [], []
        for _ in range(a.reps):
            t_whole.append(timed(whole))
            t_rows.append(timed(listed))
        e = dict(n=n, fraction=n / T, rows=stats(t_rows), whole_bank=stats(t_whole))
        e["speedup_median"] = e["whole_bank"]["median_us"] / e["rows"]["median_us"]
        per_n.append(e)
        print(f"n={n:6d} ({100 * n / T:6.2f} %)  get_pose_rows median {e['rows']['median_us']:9.1f} us "
              f"[{e['rows']['p10_us']:.1f} .. {e['rows']['p90_us']:.1f}]   get_pose_each {e['whole_bank']['median_us']:9.1f} us "
              f"[{e['whole_bank']['p10_us']:.1f} .. {e['whole_bank']['p90_us']:.1f}]   x{e['speedup_median']:.2f}", flush=True)
    res = dict(what="kfpos_get_pose_rows (n rows spread over the bank, dt_ahead per entry) against kfpos_get_pose_each "
                    "(whole bank), host clock around the synchronous call, routes alternating",
               tags=T, anchors=A, model="9-state", storage="MIXED", epochs_before=EPOCHS, reps=a.reps, per_n=per_n,
               crossover_n_over_T=crossover(per_n))
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)
    b.close()


if __name__ == "__main__":
    main()
