"""Replaying ranging rounds of the 6-state filter in which every tag has a timeline of its own: single kfpos_step_toa_dev
calls with a per-tag dt array against kfpos_run_trace_each_dev (profiles/HISTORY.md).

Bank: 65 536 tags x 8 anchors, KFPOS_STORE_MIXED, fixed start -- and the same at 131 072 tags, where the single calls run
the two-wavefront build and the one call holds the bank to one wavefront per SIMD. The tags range in G TDMA phase groups,
group g a fraction g / G of the ranging period behind group 0 (synth.merge_timelines with no IMU samples): a period is G
slots and every slot carries 1 / G of the bank. G = 1, 2, 10: participation 100 %, 50 %, 10 %. Two layouts where G > 1:
    contiguous   groups in blocks of 64 tags ((t // 64) % G): whole wavefronts have nothing in G - 1 slots of G
    interleaved  group = t % G: every wavefront runs every slot, 1 / G of its lanes at a time
Every route replays the same slots from the same bank state (restored before each repetition, outside the timed span);
TIMED slots are timed with kfpos_timing_begin / _end after WARM slots of warm-up:
    route A  the single calls with dt_dev on one stream, one launch per slot
    route B  kfpos_run_trace_each_dev: one call for the warm-up slots, one for the timed ones
    route C  (G = 1 only) kfpos_run_trace_dev with the slots' shared dt: the floor, no per-lane dt and no mask
The routes of a comparison alternate in one process, --rounds times each. Reported: median and 10th .. 90th percentile
of the time per SLOT, in microseconds, the spread of A (p90 - p10), and whether B's median is above A's by more than that
spread (exit status 1 if it is at any participation of the 65 536-tag bank; the 131 072-tag figures are reported only).

    python tools/trace_each_latency.py --out profiles/trace_each_latency.json [--rounds 7] [--commit HASH]
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roskfpos_amd import capi, synth  # noqa: E402
from roskfpos_amd.synth import Workload  # noqa: E402
from replay_timing import alternate, commit_of, finish, stats  # noqa: E402

T, A = 1 << 16, 8
GROUPS = (1, 2, 10)
WARM, TIMED = 40, 400       # slots; both are multiples of every G
ABSENT_MM = -1


class Replay:
    def __init__(self, tags):
        import torch
        self.torch = torch
        self.T = tags
        self.w = Workload(tags, A)
        self.bank = capi.KfposBank(capi.MODEL_TOA, tags, self.w.anchors, storage=capi.STORE_MIXED,
                                   init_pos=self.w.init_positions())
        self.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
        # the first epoch (the reference's hard-coded 0.1 s step) is not part of the measurement
        self.bank.step_toa(self.w.ranges_mm(0), self.w.err_est(np.float32), 0.1)
        self.start = self.bank.get_state()
        self.d_e = self.up(self.w.err_est(np.float32).T)
        self.stream = torch.cuda.current_stream().cuda_stream
        self.r_all = None

    def periods_data(self, periods):
        """every tag's own ranges by ranging period, [periods][A][T] on the device (grown on demand)"""
        have = 0 if self.r_all is None else self.r_all.shape[0]
        if have < periods:
            more = self.up(np.stack([self.w.ranges_mm(1 + p).T for p in range(have, periods)]))
            self.r_all = more if self.r_all is None else self.torch.cat([self.r_all, more])
        return self.r_all

    def schedule(self, group_of_tag, n_groups):
        """the merged slots of a bank whose tag t is in phase group group_of_tag[t] -> (d_dt [E][T], d_r [E][A][T],
        share of (tag, slot) pairs that take part, the slots' dt where all tags share it); absent entries: dt -1,
        ranges ABSENT_MM"""
        torch = self.torch
        periods = (WARM + TIMED) // n_groups
        g = synth.merge_timelines(synth.DT, 0, np.arange(n_groups) * synth.DT / n_groups, periods)
        assert g.kinds.size == WARM + TIMED and (g.kinds == 1).all()
        grp = torch.from_numpy(np.asarray(group_of_tag, dtype=np.int64)).to("cuda:0")
        d_dt = self.up(g.dt)[:, grp].contiguous()                                               # [E][T]
        r_all = self.periods_data(periods)
        absent = torch.tensor(ABSENT_MM, dtype=torch.int32, device="cuda:0")
        r = []
        for e in range(g.kinds.size):
            steps = set(g.step[e][g.step[e] >= 0].tolist())
            assert len(steps) == 1                       # the groups of a slot are in the same period
            r.append(torch.where((d_dt[e] >= 0)[None, :], r_all[steps.pop()], absent))
        share = float((g.dt >= 0)[:, np.asarray(group_of_tag)].mean())
        return d_dt, torch.stack(r), share, (g.dt[:, 0] if n_groups == 1 else None)

    def once(self, route, sched):
        d_dt, d_r, _, shared = sched
        b, nt = self.bank, self.T
        b.set_state(*self.start)

        def run(e0, e1):
            if route == "A":
                for e in range(e0, e1):
                    b.step_toa_dev(d_r[e], self.d_e, 0.0, stream=self.stream, dt_dev=d_dt[e])
            elif route == "B":
                b.run_trace_each_dev(d_dt[e0:e1], d_r[e0], A * nt, self.d_e, 0, stream=self.stream)
            else:
                b.run_trace_dev(e1 - e0, d_r[e0], A * nt, self.d_e, 0, shared[e0:e1], stream=self.stream)

        run(0, WARM)
        b.timing_begin(self.stream)
        run(WARM, WARM + TIMED)
        return b.timing_end(self.stream) * 1e3 / TIMED      # microseconds per slot

    def measure(self, name, routes, sched, rounds):
        states = []
        for route in routes:
            self.once(route, sched)
            states.append(self.bank.get_state())
        same = all(g.tobytes() == r.tobytes() for st in states[1:] for g, r in zip(st, states[0]))
        us = alternate(routes, lambda route: self.once(route, sched), rounds)
        entry = dict(layout=name, tags=self.T, participation=sched[2], same_state=bool(same))
        for route in routes:
            entry[route] = stats(us[route])
        a, b = entry["A"], entry["B"]
        entry["A_spread_us"] = a["p90_us"] - a["p10_us"]
        entry["B_minus_A_us"] = b["median_us"] - a["median_us"]
        entry["B_no_slower_than_A_within_its_spread"] = bool(entry["B_minus_A_us"] <= entry["A_spread_us"])
        if "C" in entry:
            entry["B_over_C"] = b["median_us"] / entry["C"]["median_us"]
        print(f"{self.T} tags, {name}: " + "   ".join(
            f"{r} {entry[r]['median_us']:7.2f} us [{entry[r]['p10_us']:.2f} .. {entry[r]['p90_us']:.2f}]" for r in routes) +
            f"   per slot; same state: {same}", flush=True)
        return entry


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--tags", type=int, nargs="+", default=[T, 2 * T])
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    a = ap.parse_args()
    runs = []
    for tags in a.tags:
        rp = Replay(tags)
        t = np.arange(tags)
        for G in GROUPS:
            layouts = (("synchronous", np.zeros(tags, dtype=np.int64)),) if G == 1 else \
                      (("contiguous", (t // 64) % G), ("interleaved", t % G))
            for name, grp in layouts:
                sched = rp.schedule(grp, G)
                entry = rp.measure(name, ("A", "B", "C") if G == 1 else ("A", "B"), sched, a.rounds)
                entry["groups"] = G
                runs.append(entry)
                del sched
        rp.bank.close()
        del rp
    judged = [r for r in runs if r["tags"] == a.tags[0]]
    met = all(r["B_no_slower_than_A_within_its_spread"] and r["same_state"] for r in judged)
    res = dict(what="6-state ranging rounds with a timeline per tag: single kfpos_step_toa_dev calls with dt_dev on one "
                    "stream (A) against kfpos_run_trace_each_dev (B), and at full participation kfpos_run_trace_dev "
                    "with a shared dt (C); microseconds per slot, tags in G TDMA phase groups of one ranging period "
                    f"(kfpos_timing_begin / _end over {TIMED} slots after {WARM} of warm-up)",
               command="python tools/trace_each_latency.py " + " ".join(sys.argv[1:]), commit=a.commit or commit_of(ROOT),
               anchors=A, storage="MIXED", rounds=a.rounds, warm_slots=WARM, timed_slots=TIMED, runs=runs,
               claim=f"{a.tags[0]} tags, every participation and layout: B's median is not above A's by more than A's "
                     "own 10th .. 90th percentile spread",
               claim_holds=bool(met))
    return finish(res, a.out, met)


if __name__ == "__main__":
    sys.exit(main())
