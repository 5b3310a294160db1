"""Replaying a multi-sensor event schedule of the 8-state planar filter: single _dev calls against
kfpos_run_planar_events_dev (profiles/HISTORY.md).

Bank: 65 536 tags x 8 anchors, KFPOS_STORE_F64, fixed start. A ranging period is one of
    ranging   one ranging event
    imu1      1 IMU event + the ranging event
    full      10 IMU + 2 PX4Flow + 1 magnetometer event, interleaved as the sensors' rates would, + the ranging event
every event at timeLag dt / (events per period). 20 periods are timed with kfpos_timing_begin / _end after 5 periods of
warm-up, and both routes replay the same events from the same bank state (restored before each repetition, outside the
timed span):
    route A  the single calls (kfpos_step_sensor_dev / kfpos_step_toa_dev) on one stream, one launch per event
    route B  kfpos_run_planar_events_dev: one call for the warm-up periods, one for the timed ones
A and B alternate in one process, --rounds times each. Reported per period and route: median and 10th .. 90th percentile
of the time per ranging period, in microseconds, and the ratio of the medians.

    python tools/planar_events_replay_latency.py --out profiles/planar_events_replay_latency.json [--rounds 7]
    python tools/planar_events_replay_latency.py --kernels-only      # one repetition of each, for a kernel trace
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
TOA, PX4, IMU, MAG = capi.PLANAR_EVENT_TOA, capi.SENSOR_PX4FLOW, capi.SENSOR_IMU, capi.SENSOR_MAG
PERIODS = {"ranging": [TOA], "imu1": [IMU, TOA],
           "full": [IMU, IMU, PX4, IMU, IMU, IMU, MAG, IMU, IMU, PX4, IMU, IMU, IMU, TOA]}
WARM, TIMED = 5, 20
CFG = dict(use_fixed_height=1, fixed_height=1.0, init_angle=0.3, px4_height=Workload.PX4_HEIGHT, px4_arm_p1=0.05,
           px4_arm_p2=-0.02, px4_cov_velocity=0.002, px4_cov_gyro_z=0.001, imu_use_fixed_cov_acc=0, imu_cov_acc=0.02,
           imu_use_fixed_cov_ang_vel_z=1, imu_cov_ang_vel_z=0.0005, mag_angle_offset=0.1, mag_cov=0.01)


class Replay:
    """one bank and the inputs of WARM + TIMED periods of one kind"""

    def __init__(self, period, tags=T):
        import torch
        self.T, self.period = tags, list(period)
        w = self.w = Workload(tags, A)
        self.bank = capi.KfposBank(capi.MODEL_PLANAR, tags, w.anchors, init_pos=w.init_positions(), planar=CFG)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
        periods = WARM + TIMED
        # the first epoch (the reference's hard-coded 0.1 s step) is not part of the measurement
        self.bank.step_toa(w.ranges_mm(0), w.err_est(), 0.1)
        self.start = self.bank.get_state() + (self.bank.get_latch(), self.bank.get_height())
        self.kinds = np.array(self.period * periods, dtype=np.uint8)
        self.dts = np.full(self.kinds.size, w.dt_of(1) / len(self.period))
        count = {k: self.period.count(k) * periods for k in (TOA, PX4, IMU, MAG)}
        self.d_r = up(np.stack([w.ranges_mm(1 + p).T for p in range(count[TOA])]))       # [periods][A][T]
        self.d_e = up(w.err_est().T)
        cw, ca = np.tile(np.eye(3).ravel() * 1e-4, (tags, 1)), w.accel_cov()
        ca[:, 1] = ca[:, 3] = 0.002  # correlated accelerometer axes
        imu = [np.concatenate([wv, cw, la, ca], axis=1).T for wv, la in (w.planar_imu(i) for i in range(count[IMU]))]
        self.d_s = {IMU: up(np.stack(imu)) if imu else None,                              # [n][24][T]
                    PX4: up(np.stack([w.px4flow(i).T for i in range(count[PX4])])) if count[PX4] else None,
                    MAG: up(np.stack([w.mag(i).T for i in range(count[MAG])])) if count[MAG] else None}
        self.stream = torch.cuda.current_stream().cuda_stream

    def restore(self):
        x, P, fl, latch, z = self.start
        self.bank.set_state(x, P, fl)
        self.bank.set_latch(latch)
        self.bank.set_height(z)

    def ordinals(self, e0):
        """events of each kind ahead of event e0"""
        return {k: int((self.kinds[:e0] == k).sum()) for k in (TOA, PX4, IMU, MAG)}

    def route_a(self, e0, e1):
        b, n = self.bank, self.ordinals(e0)
        for e in range(e0, e1):
            kind = int(self.kinds[e])
            if kind == TOA:
                b.step_toa_dev(self.d_r[n[kind]], self.d_e, self.dts[e], stream=self.stream)
            else:
                b.step_sensor_dev(kind, self.d_s[kind][n[kind]], self.dts[e], stream=self.stream)
            n[kind] += 1

    def route_b(self, e0, e1):
        n, s = self.ordinals(e0), self.d_s
        at = lambda kind: None if s[kind] is None else s[kind][n[kind]]  # noqa: E731
        self.bank.run_planar_events_dev(self.kinds[e0:e1], self.dts[e0:e1], range_mm=self.d_r[n[TOA]],
                                        stride_ranges=A * self.T, err_est=self.d_e, stride_err=0,
                                        px4flow=at(PX4), stride_px4flow=5 * self.T, imu=at(IMU), stride_imu=24 * self.T,
                                        mag=at(MAG), stride_mag=3 * self.T, stream=self.stream)

    def once(self, route):
        self.restore()
        run = self.route_a if route == "A" else self.route_b
        ev = len(self.period)
        run(0, WARM * ev)
        self.bank.timing_begin(self.stream)
        run(WARM * ev, (WARM + TIMED) * ev)
        return self.bank.timing_end(self.stream) * 1e3 / TIMED      # microseconds per ranging period

    def final(self):
        return self.bank.get_state() + (self.bank.get_latch(), self.bank.get_height())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tags", type=int, default=T)
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    per_period = []
    for name, period in PERIODS.items():
        rp = Replay(period, a.tags)
        # the two routes leave the same bank behind
        rp.once("A")
        ref = rp.final()
        rp.once("B")
        got = rp.final()
        if a.kernels_only:
            rp.bank.close()
            continue
        same = all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        us = alternate(("A", "B"), rp.once, a.rounds)
        rp.bank.close()
        counts = {k: period.count(v) for k, v in (("ranging", TOA), ("imu", IMU), ("px4flow", PX4), ("mag", MAG))}
        e = entry(f"{name:8s}", "A", "B", us, period=name, events_per_period=len(period), events=counts,
                  same_state=bool(same))
        del e["second_wholly_below_first"]           # not in this tool's record
        e["A_over_B"] = e["A"]["median_us"] / e["B"]["median_us"]
        per_period.append(e)
    if a.kernels_only:
        return
    res = dict(what="planar event replay: single _dev calls on one stream (A) against kfpos_run_planar_events_dev (B), "
                    "microseconds per ranging period (kfpos_timing_begin / _end over "
                    f"{TIMED} periods after {WARM} of warm-up)",
               command="python tools/planar_events_replay_latency.py " + " ".join(sys.argv[1:]),
               commit=a.commit or commit_of(ROOT), tags=a.tags, anchors=A, storage="F64", rounds=a.rounds,
               per_period=per_period)
    return finish(res, a.out)


if __name__ == "__main__":
    sys.exit(main())
