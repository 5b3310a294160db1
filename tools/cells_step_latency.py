"""What an anchor cell costs: a ranging epoch of a bank with ONE anchor table (the existing step kernels) against the same
bank with anchor cells (kfpos_set_anchor_cells: the cells kernels, the plain forms), DESIGN.md section 6.

Banks: 65 536 tags x 8 anchors, KFPOS_STORE_MIXED, fixed start; the 9-state filter with a fresh sample per epoch (fused
rounds) and the 6-state filter. Three banks per filter, fed the same epochs from the same state (restored before every
repetition, outside the timed span):
    single      kfpos_set_anchors: k_step_imu9 (the bench kernel) / k_step_toa6
    cells1      kfpos_set_anchor_cells with 1 cell
    cells1024   kfpos_set_anchor_cells with 1 024 cells, every block of 64 rows its own (all cells hold the same
                coordinates, so the three banks must end in the same bytes: recorded as same_state)
Two ways to run the TIMED epochs, after WARM epochs of warm-up, timed with kfpos_timing_begin / _end:
    launches    one kfpos_step_toa_imu_dev / kfpos_step_toa_dev call per epoch
    trace       one kfpos_run_trace_dev call
The routes take turns in one process, --rounds times each. Reported: median and 10th .. 90th percentile of the time per
epoch in microseconds and the ratios of the medians against `single`. No bar is set: the record is what a cell costs.

The measurement runs in ONE child process under a time limit of its own (--limit seconds); the parent opens no GPU.

    python tools/cells_step_latency.py --out profiles/anchor_cells_latency.json [--rounds 7] [--commit HASH]
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from roskfpos_amd import capi  # noqa: E402
from roskfpos_amd.synth import Workload  # noqa: E402
from replay_timing import alternate, commit_of, finish, stats  # noqa: E402

T, A = 1 << 16, 8
WARM, TIMED = 8, 64
ROUTES = ("single", "cells1", "cells1024")
MODES = ("launches", "trace")


class Filter:
    def __init__(self, model):
        import torch
        self.torch, self.model, self.fused = torch, model, model == capi.MODEL_TOA_IMU
        w = self.w = Workload(T, A)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")  # noqa: E731
        n = 1 + WARM + TIMED
        self.d_r = up(np.stack([w.ranges_mm(s).T for s in range(n)]))                       # [n][A][T]
        self.d_e = up(w.err_est(np.float32).T)
        self.d_a = up(np.stack([w.accel(s, np.float32).T for s in range(n)]))               # [n][3][T]
        self.d_c = up(w.accel_cov(np.float32).T)
        self.dts = np.array([w.dt_of(s) for s in range(n)])
        self.stream = torch.cuda.current_stream().cuda_stream
        n_blocks = (T + capi.CELL_TAGS - 1) // capi.CELL_TAGS
        self.banks = {}
        for route in ROUTES:
            b = capi.KfposBank(model, T, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions())
            if route == "cells1":
                b.set_anchor_cells(w.anchors[None], np.zeros(n_blocks, dtype=np.int32))
            elif route == "cells1024":
                b.set_anchor_cells(np.repeat(w.anchors[None], n_blocks, axis=0), np.arange(n_blocks, dtype=np.int32))
            assert b.anchor_cells == {"single": 0, "cells1": 1, "cells1024": n_blocks}[route]
            self.banks[route] = b
        # the first epoch (the reference's hard-coded 0.1 s step) is not part of the measurement
        for b in self.banks.values():
            self.epochs(b, "launches", 0, 1)
        torch.cuda.synchronize()
        self.start = {r: (b.get_state(), b.get_latch()) for r, b in self.banks.items()}

    def epochs(self, b, mode, s0, s1):
        if mode == "trace":
            kw = dict(accel=self.d_a[s0], stride_accel=3 * T, cov=self.d_c, stride_cov=0) if self.fused else {}
            b.run_trace_dev(s1 - s0, self.d_r[s0], A * T, self.d_e, 0, self.dts[s0:s1], stream=self.stream, **kw)
            return
        for s in range(s0, s1):
            if self.fused:
                b.step_toa_imu_dev(self.d_r[s], self.d_e, self.d_a[s], self.d_c, self.dts[s], stream=self.stream)
            else:
                b.step_toa_dev(self.d_r[s], self.d_e, self.dts[s], stream=self.stream)

    def once(self, route, mode):
        b = self.banks[route]
        (x, P, fl), latch = self.start[route]
        b.set_state(x, P, fl)
        b.set_latch(latch)
        self.epochs(b, mode, 1, 1 + WARM)
        b.timing_begin(self.stream)
        self.epochs(b, mode, 1 + WARM, 1 + WARM + TIMED)
        return b.timing_end(self.stream) * 1e3 / TIMED      # microseconds per epoch

    def measure(self, mode, rounds):
        left = {}
        for route in ROUTES:
            self.once(route, mode)
            left[route] = list(self.banks[route].get_state()) + [self.banks[route].get_latch()]
        same = all(g.tobytes() == r.tobytes() for route in ROUTES[1:] for g, r in zip(left[route], left["single"]))
        us = alternate(ROUTES, lambda route: self.once(route, mode), rounds)
        entry = dict(filter="9-state, fused rounds" if self.fused else "6-state", mode=mode, same_state=bool(same))
        for route in ROUTES:
            entry[route] = stats(us[route])
        for route in ROUTES[1:]:
            entry[route + "_over_single"] = entry[route]["median_us"] / entry["single"]["median_us"]
        print(f"{entry['filter']}, {mode}: " + "   ".join(
            f"{r} {entry[r]['median_us']:7.2f} us [{entry[r]['p10_us']:.2f} .. {entry[r]['p90_us']:.2f}]" for r in ROUTES) +
            f"   per epoch; cells1 / single {entry['cells1_over_single']:.3f}, cells1024 / single "
            f"{entry['cells1024_over_single']:.3f}; same state: {same}", flush=True)
        return entry

    def close(self):
        for b in self.banks.values():
            b.close()


def child(a):
    runs = []
    for model in (capi.MODEL_TOA_IMU, capi.MODEL_TOA):
        f = Filter(model)
        for mode in MODES:
            runs.append(f.measure(mode, a.rounds))
        f.close()
        del f
    res = dict(what="a ranging epoch of 65 536 tags x 8 anchors, KFPOS_STORE_MIXED: one anchor table (single: the existing "
                    "step kernels) against anchor cells (cells1: 1 cell; cells1024: every block of 64 rows its own cell); "
                    f"microseconds per epoch (kfpos_timing_begin / _end over {TIMED} epochs after {WARM} of warm-up), as "
                    "one launch per epoch (launches) and as one kfpos_run_trace_dev call (trace)",
               command="python tools/cells_step_latency.py " + " ".join(x for x in sys.argv[1:] if x != "--child"),
               commit=a.commit or commit_of(ROOT), tags=T, anchors=A, storage="MIXED", rounds=a.rounds, warm_epochs=WARM,
               timed_epochs=TIMED, runs=runs, same_state=all(r["same_state"] for r in runs))
    return finish(res, a.out, res["same_state"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--limit", type=int, default=420, help="seconds the one GPU run may take")
    ap.add_argument("--commit", default=None, help="recorded in the output (default: git rev-parse HEAD)")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    try:
        return subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + sys.argv[1:], timeout=a.limit).returncode
    except subprocess.TimeoutExpired:
        print(f"the GPU run did not end within {a.limit} s", file=sys.stderr)
        return 124


if __name__ == "__main__":
    sys.exit(main())
