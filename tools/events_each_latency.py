"""Replaying an event schedule of the 9-state filter in which every tag has a timeline of its own: single _dev calls with a
per-tag dt array against kfpos_run_events_each_dev (profiles/HISTORY.md).

Bank: 65 536 tags x 8 anchors, KFPOS_STORE_MIXED, diagonal accelerometer covariance, K = 4 IMU samples per ranging period.
The tags fall into G = 4 phase groups, group g a fraction g / G of the IMU sample spacing behind group 0
(synth.merge_timelines): a ranging period is (K + 1) * G slots and every slot carries a quarter of the bank. Two layouts:
    contiguous   groups in blocks of 64 tags ((t // 64) % G): whole wavefronts have nothing in three slots of four
    interleaved  group = t % G: every wavefront runs every slot, a quarter of its lanes at a time
Per layout both routes replay the same slots from the same bank state (restored before each repetition, outside the
timed span); 20 periods are timed with kfpos_timing_begin / _end after 5 periods of warm-up:
    route A  the single calls with dt_dev on one stream, (K + 1) * G launches per period
    route B  kfpos_run_events_each_dev: one call for the warm-up periods, one for the timed ones
and on a fully synchronous schedule (G = 1, every dt >= 0), the price of the per-tag form:
    route C  kfpos_run_events_dev
    route D  kfpos_run_events_each_dev
The routes of a comparison alternate in one process, --rounds times each. Reported: median and 10th .. 90th percentile
of the time per ranging period, in microseconds. Required: on the contiguous layout B's range lies wholly below A's
(exit status 1 otherwise); the other figures are reported as they come out.

    python tools/events_each_latency.py --out profiles/events_each_replay_latency.json [--rounds 7] [--commit HASH]
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

T, A, K, G = 1 << 16, 8, 4, 4
WARM, TIMED = 5, 20
ABSENT_MM = -1


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
        periods = self.periods = WARM + TIMED
        # the first epoch (the reference's hard-coded 0.1 s step) is not part of the measurement
        self.bank.step_toa_imu(self.w.ranges_mm(0), self.w.err_est(np.float32), self.w.accel(0, np.float32),
                               self.w.accel_cov(np.float32), 0.1)
        self.start = self.bank.get_state() + (self.bank.get_latch(),)
        # every tag's own samples, by ranging period: what a slot holds for the tags that take part in it
        self.r_all = up(np.stack([self.w.ranges_mm(1 + p).T for p in range(periods)]))          # [periods][A][T]
        self.a_all = up(np.stack([self.w.accel_between(1 + p, i, K, np.float32).T
                                  for p in range(periods) for i in range(K)]))                  # [periods * K][3][T]
        self.d_e = up(self.w.err_est(np.float32).T)
        self.d_c = up(self.w.accel_cov(np.float32).T)
        self.stream = torch.cuda.current_stream().cuda_stream

    def schedule(self, group_of_tag, n_groups):
        """the merged slots of a bank whose tag t is in phase group group_of_tag[t] -> (kinds, d_dt [E][T], d_r
        [J][A][T], d_a [I][3][T], share of (tag, slot) pairs that take part); absent entries: dt -1, ranges
        ABSENT_MM, accel NaN"""
        torch = self.torch
        spacing = synth.DT / (K + 1)
        g = synth.merge_timelines(synth.DT, K, np.arange(n_groups) * spacing / n_groups, self.periods)
        grp = torch.from_numpy(np.asarray(group_of_tag, dtype=np.int64)).to("cuda:0")
        d_dt = self.up(g.dt)[:, grp].contiguous()                                               # [E][T]
        r, a = [], []
        nan = torch.tensor(float("nan"), dtype=torch.float32, device="cuda:0")
        absent = torch.tensor(ABSENT_MM, dtype=torch.int32, device="cuda:0")
        for e, kind in enumerate(g.kinds):
            here = g.step[e] >= 0
            steps, subs = set(g.step[e][here].tolist()), set(g.sub[e][here].tolist())
            assert len(steps) == 1 and len(subs) == 1   # the groups of a slot are in the same period and sub-sample
            p, i = steps.pop(), subs.pop()
            present = (d_dt[e] >= 0)[None, :]
            if kind == capi.EVENT_TOA:
                r.append(torch.where(present, self.r_all[p], absent))
            else:
                a.append(torch.where(present, self.a_all[p * K + i], nan))
        share = float((g.dt >= 0)[:, np.asarray(group_of_tag)].mean())
        return g.kinds, d_dt, torch.stack(r), torch.stack(a), share

    def restore(self):
        x, P, fl, latch = self.start
        self.bank.set_state(x, P, fl)
        self.bank.set_latch(latch)

    def single_calls(self, sched, e0, e1):
        kinds, d_dt, d_r, d_a = sched[:4]
        b = self.bank
        j, i = int((kinds[:e0] == capi.EVENT_TOA).sum()), int((kinds[:e0] == capi.EVENT_IMU).sum())
        for e in range(e0, e1):
            if kinds[e] == capi.EVENT_TOA:
                b.step_toa_dev(d_r[j], self.d_e, 0.0, stream=self.stream, dt_dev=d_dt[e])
                j += 1
            else:
                b.step_imu_dev(d_a[i], self.d_c, 0.0, stream=self.stream, dt_dev=d_dt[e])
                i += 1

    def one_call(self, sched, e0, e1, shared=False):
        kinds, d_dt, d_r, d_a = sched[:4]
        j, i = int((kinds[:e0] == capi.EVENT_TOA).sum()), int((kinds[:e0] == capi.EVENT_IMU).sum())
        kw = dict(range_mm=d_r[j], stride_ranges=A * self.T, err_est=self.d_e, stride_err=0, accel=d_a[i],
                  stride_accel=3 * self.T, cov=self.d_c, stream=self.stream)
        if shared:   # kfpos_run_events_dev: the schedule is synchronous, every tag has the slot's dt
            self.bank.run_events_dev(kinds[e0:e1], sched[5][e0:e1], **kw)
        else:
            self.bank.run_events_each_dev(kinds[e0:e1], d_dt[e0:e1], **kw)

    def once(self, route, sched):
        n = sched[0].size // self.periods               # slots per ranging period
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
        ref = self.bank.get_state() + (self.bank.get_latch(),)
        self.once(second, sched)
        got = self.bank.get_state() + (self.bank.get_latch(),)
        same = all(np.array_equal(g, r, equal_nan=True) for g, r in zip(got, ref))
        us = alternate(routes, lambda route: self.once(route, sched), rounds)
        return entry(name, first, second, us, layout=name, slots_per_period=int(sched[0].size // self.periods),
                     participation=sched[4], same_state=bool(same))


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
    assert bool((sched[1] >= 0).all())
    sched = sched + (sched[1][:, 0].cpu().numpy(),)       # the slots' shared dts, for kfpos_run_events_dev
    sync = rp.measure("synchronous", ("C", "D"), sched, a.rounds)
    met = layouts[0]["second_wholly_below_first"] and layouts[0]["same_state"]
    res = dict(what="9-state event replay with a timeline per tag: single _dev calls with dt_dev on one stream (A) against "
                    "kfpos_run_events_each_dev (B), and kfpos_run_events_dev (C) against kfpos_run_events_each_dev (D) "
                    f"on a synchronous schedule; microseconds per ranging period of K = {K} IMU samples + 1 ranging "
                    f"epoch per tag, tags in G = {G} phase groups (kfpos_timing_begin / _end over {TIMED} periods "
                    f"after {WARM} of warm-up)",
               command="python tools/events_each_latency.py " + " ".join(sys.argv[1:]), commit=a.commit or commit_of(ROOT),
               tags=a.tags, anchors=A, storage="MIXED", K=K, G=G, rounds=a.rounds, layouts=layouts, synchronous=sync,
               requirement="contiguous layout: B's 10th .. 90th percentile range lies wholly below A's",
               requirement_met=bool(met))
    return finish(res, a.out, met)


if __name__ == "__main__":
    sys.exit(main())
