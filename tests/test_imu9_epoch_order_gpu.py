"""The order of an epoch's phases in k_step_imu9 must stay invisible. In the 8-anchor MIXED kernel (the bench kernel)
the covariance lives in the LDS park between two epochs: the head of epoch e + 1's covariance work (prediction, B, B^-1)
runs behind epoch e's update -- for the lanes that will run the prediction; a lane that waits for its ML initialisation
parks its covariance as it is -- a step that ends early reads P back from the park, and the measurements are unpacked at
the top of the body. A launch of one epoch is prologue + body + epilogue, the order it always had; so K epochs as one
launch, as 3 + 4 and as K launches of one must leave the same bytes: the pose of every epoch, x, P, flags, status words
and latch are compared as bit patterns. The same runs are held against the oracle with the tolerances of
tests/test_gpu_parity.py (F64 / MIXED 1e-9 m RMS and 1e-8 m max with equal status words, P48 1e-7 / 1e-6 with equal
flags, F32 5e-6 m RMS).

P48, F32 and F64 keep the old order (as do the generic anchor loop and the IMU-only kernel, which are not here for that
reason): for them this is one more check that nothing moved, and the cases are there for the day one of them is rotated.

Every scenario is chosen on the CPU with the oracle and asserted on the status words of the kernel: a scenario that does
not occur fails. T = 37 is a partly filled wavefront, T = 101 two wavefronts, the second ragged; 8 anchors."""
import functools

import numpy as np
import pytest

import step_checks as steps
from conftest import has_gpu
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

A, K = 8, 7
UPDATE_SKIPPED, FEW_RANGES, ML_INIT, NONFINITE = (capi.ST_UPDATE_SKIPPED, capi.ST_FEW_RANGES, capi.ST_ML_INIT,
                                                    capi.ST_NONFINITE)
E9 = [0, 1, 2, 6, 7, 8]
# (RMS, max) in metres against the oracle, status words compared: tests/test_gpu_parity.py
TOL = {0: (1e-9, 1e-8, "words"), 2: (1e-9, 1e-8, "words"), 3: (1e-7, 1e-6, "flags"), 1: (5e-6, None, None)}
SCENARIOS = ("started", "nan_starts", "fixed_start", "err_zero", "latched_replay", "nan_state")
NEVER, ZERO_ERR, BAD = 5, 3, 9     # the tag that never starts / whose errorEstimation is 0 / whose state is NaN


class Scenario:
    """what a scenario runs: `pre` epochs one launch each (fused steps), an edit of the state, then K epochs from s0"""
    def __init__(self, name, T):
        self.name, self.T = name, T
        self.w = Workload(T, A)
        self.pre = {"started": 6, "nan_state": 6, "latched_replay": 1}.get(name, 0)
        self.S = self.pre + K
        self.dts = steps.dts(self.S)
        self.init = name != "nan_starts"
        self.accel = name != "latched_replay"     # False: MODE_TOA epochs that re-fuse the latched sample
        self.r = np.stack([self.w.ranges_mm(s) for s in range(self.S)])
        self.err = self.w.err_est(np.float64).copy()
        self.bare = np.arange(T) % 3 == 1 if name == "latched_replay" else np.zeros(T, dtype=bool)
        if name == "nan_starts":          # tag t starts in epoch 2 * (t % 3): fewer than four ranges until then
            for t in range(T):
                self.r[:2 * (t % 3), t, 3:] = 0
            self.r[:, NEVER, 2:] = 0
        if name == "err_zero":
            self.err[ZERO_ERR] = 0.0

    def trace(self, storage, dev):
        return steps.Trace(self.w, self.S, storage, dev, r=self.r, err=self.err)

    def edit(self, x, P, fl):
        if self.name == "latched_replay":
            assert (fl & steps.FL_HAS_IMU).all()
            fl[self.bare] &= ~steps.FL_HAS_IMU
        if self.name == "nan_state":
            x[BAD, :3] = np.nan
        return x, P, fl


def _invertible(P, dt):
    """sym6_inverse's verdict on B = (F P F' + Q)_ee, per tag: every LDL' pivot above 1e-7 of its diagonal entry"""
    import oracle_py
    F, Q = oracle_py.predict_matrices(1, dt)
    ok = np.zeros(len(P), dtype=bool)
    for t, p in enumerate(P):
        B = (F @ p @ F.T + Q)[np.ix_(E9, E9)]
        L, d, good = np.eye(6), np.zeros(6), True
        for j in range(6):
            d[j] = B[j, j] - (L[j, :j] ** 2 * d[:j]).sum()
            good = good and d[j] > 1e-7 * B[j, j]
            dj = d[j] if d[j] > 0 else 1.0
            for i in range(j + 1, 6):
                L[i, j] = (B[i, j] - (L[i, :j] * L[j, :j] * d[:j]).sum()) / dj
        ok[t] = good
    return ok


@functools.lru_cache(maxsize=None)
def _oracle(name, T, f32):
    """the scenario on the CPU, once per (scenario, T, measurement width): poses [K][T][3] and status words [K][T] of
    the K epochs, and whether B was invertible at the head of each of them [K][T]"""
    sn = Scenario(name, T)
    inv = []

    def edit(o, s):
        if s == sn.pre and name == "nan_state":
            x, P = o.get_state()
            x[BAD, :3] = np.nan
            o.set_state(x, P)
        if s >= sn.pre:
            inv.append(_invertible(o.get_state()[1], sn.dts[s]))

    poses, stats = steps.oracle_run(sn.w, sn.r, sn.err, sn.dts, real=np.float32 if f32 else np.float64,
                                 init=sn.w.init_positions() if sn.init else None,
                                 accel=[s < sn.pre or sn.accel for s in range(sn.S)], edit=edit)[:2]
    return poses[sn.pre:], stats[sn.pre:], np.stack(inv)


def _start(sc, tr, storage, chunk):
    b = steps.bank(sc.w, sc.T, storage, chunk=chunk, init=sc.init)
    if sc.pre:
        steps.single_calls(b, tr, sc.dts, sc.pre, poses=False)
    b.set_state(*sc.edit(*b.get_state()))     # (every scenario goes through the same round trip)
    return b


def _occurs(sc, st, poses, inv):
    """the scenario really happened: st = the kernel's status words of the K epochs [K][T], poses [K][3][T]"""
    T, fl, name = sc.T, capi.st_flags(st), sc.name
    if name == "started":
        assert (fl == 0).all() and np.isfinite(poses).all()
    elif name == "nan_starts":
        lanes = np.array([t for t in range(T) if t != NEVER])
        for t in lanes:
            e0 = 2 * (t % 3)
            assert (fl[:e0, t] == FEW_RANGES).all() and fl[e0, t] == ML_INIT, (t, fl[:, t])
            assert not (fl[e0 + 1:, t] & (FEW_RANGES | ML_INIT)).any(), (t, fl[:, t])      # ... and steps from then on
            assert np.isnan(poses[:e0, 0, t]).all() and np.isfinite(poses[e0:, :, t]).all()
        assert (fl[:, NEVER] == FEW_RANGES).all() and np.isnan(poses[:, 0, NEVER]).all()
        assert len({2 * (t % 3) for t in range(min(T, 64))}) == 3      # wave-mates run normal steps meanwhile
    elif name == "fixed_start":
        assert (fl == 0).all()
        # B is singular at the fixed start: the (I + M B) form; tags change to the information form within the launch
        assert not inv[0].any() and (inv[-1] & ~inv[0]).any() and (np.diff(inv.sum(1)) >= 0).all(), inv.sum(1)
    elif name == "err_zero":
        others = np.arange(T) != ZERO_ERR
        assert (fl[:, ZERO_ERR] == UPDATE_SKIPPED).all() and (fl[:, others] == 0).all()
    elif name == "latched_replay":
        assert (fl == 0).all() and sc.bare[:min(T, 64)].any() and not sc.bare[:min(T, 64)].all()
    elif name == "nan_state":
        others = np.arange(T) != BAD
        assert np.isnan(poses[:, :, BAD]).all() and np.isfinite(poses[:, :, others]).all()


@pytest.mark.parametrize("name", SCENARIOS)
@pytest.mark.parametrize("storage", [2, 3, 1, 0])   # mixed, p48, f32, f64
@pytest.mark.parametrize("T", [37, 101])
def test_one_launch_equals_three_plus_four_equals_seven_and_the_oracle(T, storage, name):
    if not has_gpu():
        pytest.skip("no GPU")
    sc = Scenario(name, T)
    tr = sc.trace(storage, "cuda:0")
    s0, dts = sc.pre, sc.dts

    # seven launches of one epoch through the single-epoch entry points: the status words of every epoch
    b = _start(sc, tr, storage, None)
    ref = steps.single_calls(b, tr, dts, K, s0, sc.accel, poses=False)
    if name == "err_zero":
        assert not np.array_equal(ref.P[ZERO_ERR], np.zeros((9, 9)))     # its covariance is predicted all the same
    b.close()
    # ... and through the trace entry point, which also writes the poses
    b = _start(sc, tr, storage, 1)
    single = steps.fused(b, tr, dts, K, s0, sc.accel)
    b.close()
    steps.same(single, ref.last(single.poses), "seven launches of one epoch")
    # one launch of seven
    b = _start(sc, tr, storage, 25)
    one = steps.fused(b, tr, dts, K, s0, sc.accel)
    b.close()
    steps.same(one, single, "one launch of seven epochs")
    # 3 + 4
    b = _start(sc, tr, storage, 25)
    first = steps.fused(b, tr, dts, 3, s0, sc.accel)
    assert np.array_equal(first.status, ref.status[2]), "status words after three epochs"
    second = steps.fused(b, tr, dts, 4, s0 + 3, sc.accel)
    b.close()
    steps.same(second._replace(poses=np.concatenate([first.poses, second.poses])), single,
               "launches of three and four epochs")

    poses_o, stats_o, inv = _oracle(name, T, storage != 0)
    _occurs(sc, ref.status, single.poses, inv)
    if name == "nan_state":      # its bytes do not reach anybody else: the same run without it
        plain = Scenario("started", T)
        b = _start(plain, tr, storage, 25)
        clean = steps.fused(b, tr, dts, K, s0)
        b.close()
        keep = np.arange(T) != BAD
        steps.same(one.only(keep), clean.only(keep), "the tags next to the NaN one")
        assert one.status[BAD] & NONFINITE

    # the oracle: the poses of the K epochs (latched_replay: the oracle has a sample on every tag -- the latched ones)
    rms_bar, max_bar, words = TOL[storage]
    keep = ~sc.bare & ((np.arange(T) != BAD) | (name != "nan_state"))
    got, want = single.poses.transpose(0, 2, 1)[:, keep], poses_o[:, keep]
    assert np.array_equal(np.isnan(got), np.isnan(want))
    d = np.nan_to_num(got - want)
    n = max(1, int(np.isfinite(want).all(axis=2).sum()))
    rms, mx = float(np.sqrt((d ** 2).sum() / n)), float(np.abs(d).max())
    print(f"{name} T={T} storage={storage}: {rms:.3e} m RMS, {mx:.3e} m max against the oracle over {K} epochs")
    assert rms <= rms_bar and (max_bar is None or mx <= max_bar), (rms, mx)
    if words == "words":
        assert np.array_equal(ref.status[:, keep], stats_o[:, keep])
    elif words == "flags":
        assert np.array_equal(capi.st_flags(ref.status[:, keep]), capi.st_flags(stats_o[:, keep]))
