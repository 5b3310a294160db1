"""Latency of the per-tag lifecycle calls against the whole-bank accessors (profiles/HISTORY.md).

Host clock around each synchronous call (every one ends in a device synchronise), after warm-up, alternating in one
process the per-tag call of n rows with the only route to the same end the whole-bank accessors offer:
    get_tags   vs  kfpos_get_state + kfpos_get_latch
    set_tags   vs  kfpos_set_state + kfpos_set_latch
    reset_tags vs  kfpos_set_state + kfpos_set_latch   (get everything once, patch on the host, set everything)
for n in {1, 64, 4096, 65536} on (a) 1 048 576 tags, 6-state, F64 and (b) 65 536 tags, 9-state, MIXED.

    python tools/tag_lifecycle_latency.py --out profiles/tag_lifecycle_latency.json [--reps 200] [--full-reps 5]
    python tools/tag_lifecycle_latency.py --kernels-only     # a few calls of each kind, for a kernel trace

The whole-bank calls take 0.1 - 1 s each on the large bank, so they are repeated --full-reps times per n (they do not
depend on n) while the per-tag calls run --reps times; the two are interleaved: one whole-bank call after every
reps / full-reps per-tag calls.
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
    dict(name="toa6_f64_1048576", model=capi.MODEL_TOA, T=1 << 20, storage=capi.STORE_F64),
    dict(name="imu9_mixed_65536", model=capi.MODEL_TOA_IMU, T=1 << 16, storage=capi.STORE_MIXED),
]
NS = (1, 64, 4096, 65536)


def stats(samples):
    a = np.asarray(samples) * 1e6
    return dict(n=int(a.size), median_us=float(np.median(a)), p10_us=float(np.percentile(a, 10)),
                p90_us=float(np.percentile(a, 90)), min_us=float(a.min()), max_us=float(a.max()))


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def bank_of(cfg):
    w = Workload(cfg["T"], 8)
    real = np.float64 if cfg["storage"] == capi.STORE_F64 else np.float32
    b = capi.KfposBank(cfg["model"], cfg["T"], w.anchors, storage=cfg["storage"], init_pos=w.init_positions())
    if cfg["model"] == capi.MODEL_TOA_IMU:
        b.step_toa_imu(w.ranges_mm(0), w.err_est(real), w.accel(0, real), w.accel_cov(real), 0.1)
    else:
        b.step_toa(w.ranges_mm(0), w.err_est(real), 0.1)
    return b, w


def measure(cfg, reps, full_reps):
    b, w = bank_of(cfg)
    T = cfg["T"]
    out = dict(config=cfg["name"], tags=T, state_dim=b.n, storage=cfg["storage"], per_n=[])
    x, P, fl = b.get_state()
    latch = b.get_latch()
    for n in NS:
        rows = (np.arange(n, dtype=np.int64) * 16411 % T).astype(np.int32)  # 16411 is odd: n <= T distinct rows
        assert np.unique(rows).size == n
        part = b.get_tags(rows)
        init = w.init_positions()[rows]
        calls = {
            "get_tags": lambda: b.get_tags(rows),
            "set_tags": lambda: b.set_tags(rows, part[0], part[1], part[2], part[3]),
            "reset_tags": lambda: b.reset_tags(rows, init),
        }
        fulls = {
            "get_state+get_latch": lambda: (b.get_state(), b.get_latch()),
            "set_state+set_latch": lambda: (b.set_state(x, P, fl), b.set_latch(latch)),
        }
        rival = {"get_tags": "get_state+get_latch", "set_tags": "set_state+set_latch",
                 "reset_tags": "set_state+set_latch"}
        entry = dict(n=n)
        for name, fn in calls.items():
            for _ in range(5):
                fn()
            fulls[rival[name]]()
            t_tag, t_full = [], []
            every = max(1, reps // full_reps)
            for k in range(reps):
                t_tag.append(timed(fn))
                if k % every == every - 1:
                    t_full.append(timed(fulls[rival[name]]))
            entry[name] = stats(t_tag)
            entry[name]["whole_bank_route"] = rival[name]
            entry[name]["whole_bank"] = stats(t_full)
            print(f"{cfg['name']} n={n:6d} {name:10s} median {entry[name]['median_us']:10.1f} us  "
                  f"[{entry[name]['p10_us']:.1f} .. {entry[name]['p90_us']:.1f}]   {rival[name]} "
                  f"{entry[name]['whole_bank']['median_us'] / 1e3:9.1f} ms", flush=True)
        out["per_n"].append(entry)
        b.set_state(x, P, fl)  # the bank as it was, for the next n
        b.set_latch(latch)
    return out


def kernels_only():
    for cfg in CONFIGS:
        b, w = bank_of(cfg)
        for n in NS:
            rows = (np.arange(n, dtype=np.int64) * 16411 % cfg["T"]).astype(np.int32)
            for _ in range(10):
                part = b.get_tags(rows)
                b.set_tags(rows, part[0], part[1], part[2], part[3])
                b.reset_tags(rows, w.init_positions()[rows])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--full-reps", type=int, default=5)
    ap.add_argument("--kernels-only", action="store_true")
    a = ap.parse_args()
    if a.kernels_only:
        kernels_only()
        return
    res = dict(what="per-tag lifecycle calls against the whole-bank accessors, host clock around the synchronous call",
               reps=a.reps, whole_bank_reps_per_n=a.full_reps, results=[measure(c, a.reps, a.full_reps) for c in CONFIGS])
    text = json.dumps(res, indent=1)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    else:
        print(text)


if __name__ == "__main__":
    main()
