"""Replaying an IMU-rate event schedule of the 9-state filter: single _dev calls against kfpos_run_events_dev
(profiles/HISTORY.md).

Bank: 65 536 tags x 8 anchors, KFPOS_STORE_MIXED, diagonal accelerometer covariance. A ranging period is K IMU events
(kfpos_step_imu_dev) followed by one ranging event (kfpos_step_toa_dev), every event at timeLag dt / (K + 1); K in
{0, 1, 4, 9}. 20 periods are timed with kfpos_timing_begin / _end after 5 periods of warm-up, and both routes replay the
same events from the same bank state (restored before each repetition, outside the timed span):
    route A  the single calls on one stream, K + 1 launches per period
    route B  kfpos_run_events_dev: one call for the warm-up periods, one for the timed ones
A and B alternate in one process, --rounds times each. Reported per K and route: median and 10th .. 90th percentile of
the time per ranging period, in microseconds; per route the cost of one IMU event, (period(K) - period(0)) / K.

    python tools/events_replay_latency.py --out profiles/events_replay_latency.json [--rounds 7] [--commit HASH]
    python tools/events_replay_latency.py --kernels-only      # one repetition of each, for a kernel trace
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roskfpos_amd import capi  # noqa: E402
from roskfpos_amd.synth import Workload  # noqa: E402
from replay_timing import alternate, commit_of, entry, finish  # noqa: E402

T, A = 1 << 16, 8
KS = (0, 1, 4, 9)
WARM, TIMED = 5, 20


class Replay:
    def __init__(self, tags=T):
        import torch
        self.torch = torch
        self.T = tags
        self.w = Workload(tags, A)
        self.bank = capi.KfposBank(capi.MODEL_TOA_IMU, tags, self.w.anchors, storage=capi.STORE_MIXED,
                                   init_pos=self.w.init_positions())
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
        self.up = up
        periods = WARM + TIMED
        # the first epoch (the reference's hard-coded 0.1 s step) is not part of the measurement
        self.bank.step_toa_imu(self.w.ranges_mm(0), self.w.err_est(np.float32), self.w.accel(0, np.float32),
                               self.w.accel_cov(np.float32), 0.1)
        self.start = self.bank.get_state() + (self.bank.get_latch(),)
        self.d_r = up(np.stack([self.w.ranges_mm(1 + p).T for p in range(periods)]))     # [periods][A][T]
        self.d_e = up(self.w.err_est(np.float32).T)
        self.d_c = up(self.w.accel_cov(np.float32).T)
        self.stream = torch.cuda.current_stream().cuda_stream

    def schedule(self, K):
        periods = WARM + TIMED
        acc = [self.w.accel_between(1 + p, i, K, np.float32).T for p in range(periods) for i in range(K)]
        d_a = self.up(np.stack(acc)) if K else None                                        # [periods * K][3][T]
        kinds = np.array(([capi.EVENT_IMU] * K + [capi.EVENT_TOA]) * periods, dtype=np.uint8)
        dts = np.full(kinds.size, self.w.dt_of(1) / (K + 1))
        return d_a, kinds, dts

    def restore(self):
        x, P, fl, latch = self.start
        self.bank.set_state(x, P, fl)
        self.bank.set_latch(latch)

    def route_a(self, K, d_a, dts, p0, p1):
        b = self.bank
        for p in range(p0, p1):
            for i in range(K):
                b.step_imu_dev(d_a[p * K + i], self.d_c, dts[0], stream=self.stream)
            b.step_toa_dev(self.d_r[p], self.d_e, dts[0], stream=self.stream)

    def route_b(self, K, d_a, kinds, dts, p0, p1):
        e0, e1 = p0 * (K + 1), p1 * (K + 1)
        self.bank.run_events_dev(kinds[e0:e1], dts[e0:e1], range_mm=self.d_r[p0], stride_ranges=A * self.T,
                                 err_est=self.d_e, stride_err=0, accel=d_a[p0 * K] if K else None,
                                 stride_accel=3 * self.T, cov=self.d_c if K else None, stream=self.stream)

    def once(self, route, K, sched):
        d_a, kinds, dts = sched
        self.restore()
        run = (lambda p0, p1: self.route_a(K, d_a, dts, p0, p1)) if route == "A" else \
              (lambda p0, p1: self.route_b(K, d_a, kinds, dts, p0, p1))
        run(0, WARM)
        self.bank.timing_begin(self.stream)
        run(WARM, WARM + TIMED)
        return self.bank.timing_end(self.stream) * 1e3 / TIMED      # microseconds per ranging period


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tags", type=int, default=T)
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    rp = Replay(a.tags)
    if a.kernels_only:
        for K in KS:
            sched = rp.schedule(K)
            rp.once("A", K, sched)
            rp.once("B", K, sched)
        return
    per_k = []
    for K in KS:
        sched = rp.schedule(K)
        # the two routes leave the same bank behind
        rp.once("A", K, sched)
        ref = rp.bank.get_state()
        rp.once("B", K, sched)
        got = rp.bank.get_state()
        same = all(np.array_equal(g, r, equal_nan=True) for g, r in zip(got, ref))
        us = alternate(("A", "B"), lambda route: rp.once(route, K, sched), a.rounds)
        e = entry(f"K={K}", "A", "B", us, K=K, events_per_period=K + 1, same_state=bool(same))
        del e["second_wholly_below_first"]           # not in this tool's record
        per_k.append(e)
    base = {r: per_k[0][r]["median_us"] for r in ("A", "B")}
    imu_event = {r: {str(e["K"]): (e[r]["median_us"] - base[r]) / e["K"] for e in per_k if e["K"]} for r in ("A", "B")}
    res = dict(what="9-state event replay: single _dev calls on one stream (A) against kfpos_run_events_dev (B), "
                    "microseconds per ranging period of K IMU events + 1 ranging event (kfpos_timing_begin / _end over "
                    f"{TIMED} periods after {WARM} of warm-up)",
               command="python tools/events_replay_latency.py " + " ".join(sys.argv[1:]),
               commit=a.commit or commit_of(ROOT), tags=a.tags, anchors=A, storage="MIXED", rounds=a.rounds, per_K=per_k, us_per_imu_event=imu_event)
    return finish(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
