"""Replaying a multi-sensor event schedule of the 8-state planar filter in which every tag has a timeline of its own: single
_dev calls with a per-tag dt array against kfpos_run_planar_events_each_dev (profiles/HISTORY.md).

Bank: 65 536 tags x 8 anchors, KFPOS_STORE_F64, fixed start. Every tag's ranging period is 10 IMU + 2 PX4Flow + 1
magnetometer sample, evenly spaced at their own rates (synth.planar_tag_timeline), + the ranging epoch: 14 events. The
tags fall into G = 4 phase groups, group g a fraction g / G of the IMU sample spacing behind group 0
(synth.merge_planar_timelines): a ranging period is 14 * G slots and every slot carries a quarter of the bank. Layouts:
    contiguous   groups in blocks of 64 tags ((t // 64) % G): whole wavefronts have nothing in three slots of four
    interleaved  group = t % G: every wavefront runs every slot, a quarter of its lanes at a time
Per layout both routes replay the same slots from the same bank state (restored before each repetition, outside the
timed span); 20 periods are timed with kfpos_timing_begin / _end after 5 periods of warm-up:
    route A  the single calls with dt_dev on one stream, 14 * G launches per period
    route B  kfpos_run_planar_events_each_dev: one call for the warm-up periods, one for the timed ones
and on a fully synchronous schedule (G = 1, every dt >= 0), the price of the per-tag form:
    route C  kfpos_run_planar_events_dev
    route D  kfpos_run_planar_events_each_dev
The routes of a comparison alternate in one process, --rounds times each, and must leave the same bytes behind
(asserted). Reported: median and 10th .. 90th percentile of the time per ranging period, in microseconds. Required: on
the contiguous layout B's range lies wholly below A's (exit status 1 otherwise); the other figures are reported as they
come out. Absent (tag, slot) pairs hold dt -1, NaN samples and -1 mm ranges.

    python tools/planar_events_each_latency.py --out profiles/planar_events_each_latency.json [--rounds 7] [--commit HASH]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roskfpos_amd import capi, synth  # noqa: E402
from roskfpos_amd.synth import Workload  # noqa: E402
from replay_timing import alternate, commit_of, entry, finish  # noqa: E402

T, A, G = 1 << 16, 8, 4
TOA, PX4, IMU, MAG = capi.PLANAR_EVENT_TOA, capi.SENSOR_PX4FLOW, capi.SENSOR_IMU, capi.SENSOR_MAG
PER_PERIOD = {IMU: 10, PX4: 2, MAG: 1, TOA: 1}
EVENTS = sum(PER_PERIOD.values())
WARM, TIMED = 5, 20
ABSENT_MM = -1
CFG = dict(use_fixed_height=1, fixed_height=1.0, init_angle=0.3, px4_height=Workload.PX4_HEIGHT, px4_arm_p1=0.05,
           px4_arm_p2=-0.02, px4_cov_velocity=0.002, px4_cov_gyro_z=0.001, imu_use_fixed_cov_acc=0, imu_cov_acc=0.02,
           imu_use_fixed_cov_ang_vel_z=1, imu_cov_ang_vel_z=0.0005, mag_angle_offset=0.1, mag_cov=0.01)


class Replay:
    def __init__(self, tags=T):
        import torch
        self.torch = torch
        self.T = tags
        w = self.w = Workload(tags, A)
        self.bank = capi.KfposBank(capi.MODEL_PLANAR, tags, w.anchors, init_pos=w.init_positions(), planar=CFG)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
        self.up = up
        periods = self.periods = WARM + TIMED
        # the first epoch (the reference's hard-coded 0.1 s step) is not part of the measurement
        self.bank.step_toa(w.ranges_mm(0), w.err_est(), 0.1)
        self.start = self.bank.get_state() + (self.bank.get_latch(), self.bank.get_height())
        # every tag's own samples by ordinal: what a slot holds for the tags that take part in it
        self.own = {TOA: up(np.stack([w.ranges_mm(1 + p).T for p in range(periods)]))}              # [n][A][T]
        for kind in (PX4, IMU, MAG):
            self.own[kind] = torch.stack([up(self.sample(kind, n).T)
                                          for n in range(periods * PER_PERIOD[kind])])              # [n][C][T]
        self.d_e = up(w.err_est().T)
        self.stream = torch.cuda.current_stream().cuda_stream

    def sample(self, kind, n):
        """synth.planar_sample with the correlated accelerometer axes of tools/planar_events_replay_latency.py"""
        a = synth.planar_sample(self.w, kind, n)
        if kind == IMU:
            a[:, 15 + 1] = a[:, 15 + 3] = 0.002
        return a

    def schedule(self, group_of_tag, n_groups):
        """the merged slots of a bank whose tag t is in phase group group_of_tag[t] -> dict(kinds, d_dt [E][T], inputs
        {kind: [n][C][T]} in slot order, share of (tag, slot) pairs that take part, dts of group 0)"""
        torch = self.torch
        spacing = synth.DT / (PER_PERIOD[IMU] + 1)
        lines = [synth.planar_tag_timeline(synth.DT, g * spacing / n_groups, self.periods, n_imu=PER_PERIOD[IMU],
                                           n_px4=PER_PERIOD[PX4], n_mag=PER_PERIOD[MAG]) for g in range(n_groups)]
        m = synth.merge_planar_timelines(lines)
        assert m.kinds.size == EVENTS * n_groups * self.periods and (m.present.sum(axis=1) == 1).all()
        grp = torch.from_numpy(np.asarray(group_of_tag, dtype=np.int64)).to("cuda:0")
        d_dt = self.up(m.dt)[:, grp].contiguous()                                                   # [E][T]
        nan = torch.tensor(float("nan"), dtype=torch.float64, device="cuda:0")
        absent = torch.tensor(ABSENT_MM, dtype=torch.int32, device="cuda:0")
        inputs = {k: [] for k in (TOA, PX4, IMU, MAG)}
        for e, kind in enumerate(m.kinds):
            kind = int(kind)
            n = int(m.ordinal[e][m.present[e]][0])       # the one group of this slot reads its own sample n
            present = (d_dt[e] >= 0)[None, :]
            inputs[kind].append(torch.where(present, self.own[kind][n], absent if kind == TOA else nan))
        inputs = {k: torch.stack(v) for k, v in inputs.items()}
        share = float(m.present[:, np.asarray(group_of_tag)].mean())
        return dict(kinds=m.kinds, d_dt=d_dt, inputs=inputs, share=share, dts=m.dt[:, 0].copy())

    def restore(self):
        x, P, fl, latch, z = self.start
        self.bank.set_state(x, P, fl)
        self.bank.set_latch(latch)
        self.bank.set_height(z)

    def final(self):
        return self.bank.get_state() + (self.bank.get_latch(), self.bank.get_height())

    @staticmethod
    def ordinals(kinds, e0):
        return {k: int((kinds[:e0] == k).sum()) for k in (TOA, PX4, IMU, MAG)}

    def single_calls(self, sched, e0, e1):
        kinds, d_dt, s = sched["kinds"], sched["d_dt"], sched["inputs"]
        b, n = self.bank, self.ordinals(kinds, e0)
        for e in range(e0, e1):
            kind = int(kinds[e])
            if kind == TOA:
                b.step_toa_dev(s[TOA][n[kind]], self.d_e, 0.0, stream=self.stream, dt_dev=d_dt[e])
            else:
                b.step_sensor_dev(kind, s[kind][n[kind]], 0.0, stream=self.stream, dt_dev=d_dt[e])
            n[kind] += 1

    def one_call(self, sched, e0, e1, shared=False):
        kinds, d_dt, s = sched["kinds"], sched["d_dt"], sched["inputs"]
        n = self.ordinals(kinds, e0)
        kw = dict(range_mm=s[TOA][n[TOA]], stride_ranges=A * self.T, err_est=self.d_e, stride_err=0,
                  px4flow=s[PX4][n[PX4]], stride_px4flow=5 * self.T, imu=s[IMU][n[IMU]], stride_imu=24 * self.T,
                  mag=s[MAG][n[MAG]], stride_mag=3 * self.T, stream=self.stream)
        if shared:   # kfpos_run_planar_events_dev: the schedule is synchronous, every tag has the slot's dt
            self.bank.run_planar_events_dev(kinds[e0:e1], sched["dts"][e0:e1], **kw)
        else:
            self.bank.run_planar_events_each_dev(kinds[e0:e1], d_dt[e0:e1], **kw)

    def once(self, route, sched):
        n = sched["kinds"].size // self.periods               # slots per ranging period
        self.restore()
        run = {"A": lambda e0, e1: self.single_calls(sched, e0, e1),
               "B": lambda e0, e1: self.one_call(sched, e0, e1),
               "C": lambda e0, e1: self.one_call(sched, e0, e1, shared=True),
               "D": lambda e0, e1: self.one_call(sched, e0, e1)}[route]
        run(0, WARM * n)
        self.bank.timing_begin(self.stream)
        run(WARM * n, (WARM + TIMED) * n)
        return self.bank.timing_end(self.stream) * 1e3 / TIMED      # microseconds per ranging period

    def measure(self, name, routes, sched, rounds):
        first, second = routes
        self.once(first, sched)
        ref = self.final()
        self.once(second, sched)
        got = self.final()
        same = all(g.tobytes() == r.tobytes() for g, r in zip(got, ref))
        assert same, f"{name}: routes {first} and {second} leave different bytes behind"
        assert np.isfinite(ref[0]).all()
        us = alternate(routes, lambda route: self.once(route, sched), rounds)
        e = entry(name, first, second, us, layout=name, slots_per_period=int(sched["kinds"].size // self.periods),
                  participation=sched["share"], same_state=bool(same))
        e["first_over_second"] = e[first]["median_us"] / e[second]["median_us"]
        return e


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tags", type=int, default=T)
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    a = ap.parse_args()
    rp = Replay(a.tags)
    t = np.arange(a.tags)
    layouts = []
    for name, grp in (("contiguous", (t // 64) % G), ("interleaved", t % G)):
        sched = rp.schedule(grp, G)
        layouts.append(rp.measure(name, ("A", "B"), sched, a.rounds))
        del sched
    sched = rp.schedule(np.zeros(a.tags, dtype=np.int64), 1)
    assert bool((sched["d_dt"] >= 0).all())
    sync = rp.measure("synchronous", ("C", "D"), sched, a.rounds)
    met = layouts[0]["second_wholly_below_first"] and layouts[0]["same_state"]
    res = dict(what="planar event replay with a timeline per tag: single _dev calls with dt_dev on one stream (A) against "
                    "kfpos_run_planar_events_each_dev (B), and kfpos_run_planar_events_dev (C) against "
                    "kfpos_run_planar_events_each_dev (D) on a synchronous schedule; microseconds per ranging period of "
                    "10 IMU + 2 PX4Flow + 1 magnetometer sample + 1 ranging epoch per tag, tags in "
                    f"G = {G} phase groups (kfpos_timing_begin / _end over {TIMED} periods after {WARM} of warm-up)",
               command="python tools/planar_events_each_latency.py " + " ".join(sys.argv[1:]),
               commit=a.commit or commit_of(ROOT), tags=a.tags, anchors=A, storage="F64", G=G, rounds=a.rounds,
               layouts=layouts, synchronous=sync,
               requirement="contiguous layout: B's 10th .. 90th percentile range lies wholly below A's",
               requirement_met=bool(met))
    return finish(res, a.out, met)


if __name__ == "__main__":
    sys.exit(main())
