"""The epoch loop of the 9-state kernel (k_step_imu9): what it reads ahead and what it stores early must stay invisible.
In a multi-epoch launch the kernel reads the next epoch's dt (scalar, from the kernel arguments) and accelerometer
sample one epoch ahead, stores the pose before the covariance update, and runs the diagonal form of the gain iteration
in wavefronts whose accelerometer covariances are all diagonal. Every comparison here is bit for bit (step_checks.same):
the pose of every epoch, x, P, flags, status words and latch.

The synthetic trace has the same dt in every epoch after the first, which would hide an off-by-one in the dt that is read
ahead: these tests give every epoch its own."""

import numpy as np
import pytest

import step_checks as sc
from conftest import has_gpu
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("A", [8, 5])               # the 8-anchor kernel (epoch in registers), the run-time-loop kernel
@pytest.mark.parametrize("storage", [0, 1, 2, 3])   # f64, f32, mixed, p48
@pytest.mark.parametrize("T", [64, 130])            # one wavefront; two full ones and one of two lanes
def test_fused_launches_equal_single_epoch_launches_with_a_dt_per_epoch(T, storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    S = 7
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    b = sc.bank(w, T, storage)
    ref = sc.single_calls(b, tr, dts, S, poses=False)
    b.close()
    st = capi.st_flags(ref.status)
    assert (st[4, 1::9] != 0).all() and (st == 0).mean() > 0.5   # the few-ranges path ran, most steps are plain
    poses = None
    for chunk in (1, 2, 3, 7, 25):      # 1: one launch per epoch through the trace entry point; its poses are the reference
        b = sc.bank(w, T, storage, chunk=chunk)
        got = sc.fused(b, tr, dts, S)
        b.close()
        poses = got.poses if poses is None else poses
        sc.same(got, ref.last(poses), f"chunk {chunk}")
        if chunk == 7:
            b = sc.bank(w, T, storage, chunk=chunk)
            bare = sc.fused(b, tr, dts, S, with_traj=False)
            b.close()
            sc.same(bare, got, "trajectory=None", sc.Run._fields[1:])


@pytest.mark.parametrize("storage", [0, 2])
def test_ml_initialisation_inside_a_fused_launch(storage):
    """no start position: every tag initialises from its first ML solve (a step that leaves early), some of them late"""
    if not has_gpu():
        pytest.skip("no GPU")
    T, A, S = 130, 8, 7
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    tr.r[0, 2:, 3::5] = 0             # too few ranges in epoch 0 for every fifth tag: it initialises one epoch later
    b = sc.bank(w, T, storage, init=False)
    ref = sc.single_calls(b, tr, dts, S, poses=False)
    b.close()
    poses = None
    for chunk in (1, 3, 7):
        b = sc.bank(w, T, storage, chunk=chunk, init=False)
        got = sc.fused(b, tr, dts, S)
        b.close()
        poses = got.poses if poses is None else poses
        sc.same(got, ref.last(poses), f"chunk {chunk}")
    assert np.isnan(poses[0, 0, 3::5]).all() and np.isfinite(poses[1]).all()   # late starters waited one epoch
    st = capi.st_flags(ref.status)      # few ranges, then ML init
    assert (st[0, 3::5] == capi.ST_FEW_RANGES).all() and (st[1, 3::5] & capi.ST_ML_INIT != 0).all()


@pytest.mark.parametrize("storage,A", [(2, 8), (0, 8), (3, 5)])
def test_refuse_of_the_latched_sample(storage, A):
    """ranging-only epochs on a 9-state bank re-fuse the sample the last fused step latched"""
    if not has_gpu():
        pytest.skip("no GPU")
    T, S = 130, 7
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    b = sc.bank(w, T, storage)
    sc.single_calls(b, tr, dts, 1, poses=False)
    ref = sc.single_calls(b, tr, dts, S - 1, s0=1, accel=False, poses=False)
    b.close()
    poses = None
    for chunk in (1, 2, 25):
        b = sc.bank(w, T, storage, chunk=chunk)
        sc.fused(b, tr, dts, 1)
        got = sc.fused(b, tr, dts, S - 1, s0=1, accel=False)
        b.close()
        poses = got.poses if poses is None else poses
        sc.same(got, ref.last(poses), f"chunk {chunk}")


def test_the_diagonal_form_is_invisible():
    if not has_gpu():
        pytest.skip("no GPU")
    T, A, S, storage = 192, 8, 30, capi.STORE_MIXED
    w = Workload(T, A)
    dts = np.array([w.dt_of(s) for s in range(S)])
    tr_a = sc.Trace(w, S, storage, gaps=True)
    cov_b = w.accel_cov().copy()
    cov_b[5::64, 1] = cov_b[5::64, 3] = 1e-3      # lane 5 of every wavefront: an off-diagonal of 1e-3 m^2/s^4
    tr_b = sc.Trace(w, S, storage, cov=cov_b, gaps=True)
    out = {}
    for name, tr, diag in (("A", tr_a, None), ("A full", tr_a, 0), ("B", tr_b, None), ("B full", tr_b, 0)):
        b = sc.bank(w, T, storage, diag=diag)
        out[name] = sc.fused(b, tr, dts, S)
        b.close()
    b = sc.bank(w, T, storage)
    per_epoch = sc.single_calls(b, tr_a, dts, S, poses=False)
    b.close()
    assert (capi.st_gain_iters(per_epoch.status) == 20).any()         # capped steps are in it
    sc.same(out["A"], per_epoch.last(), "fused against per-epoch launches", sc.Run._fields[1:])
    sc.same(out["A"], out["A full"], "all diagonal: default against KFPOS_IMU9_DIAG=0")
    sc.same(out["B"], out["B full"], "one lane per wavefront not diagonal: default against KFPOS_IMU9_DIAG=0")
    others = np.ones(T, dtype=bool)
    others[5::64] = False
    a_, b_ = out["A"].only(others), out["B"].only(others)
    assert np.array_equal(a_.poses, b_.poses), "poses of the other tags"
    assert np.array_equal(a_.status, b_.status), "status words of the other tags"
    assert np.array_equal(a_.x, b_.x) and np.array_equal(a_.P, b_.P) and np.array_equal(a_.flags, b_.flags)
    assert not np.array_equal(out["A"].x[~others], out["B"].x[~others])  # (the off-diagonal does reach the filter)


def test_fused_launches_with_a_dt_per_epoch_match_the_oracle():
    if not has_gpu():
        pytest.skip("no GPU")
    T, A, S, storage = 128, 8, 40, capi.STORE_MIXED
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    b = sc.bank(w, T, storage)
    got = sc.fused(b, tr, dts, S)
    b.close()
    xo = sc.oracle_run(w, tr.r_host, w.err_est(), dts, real=np.float32, init=w.init_positions())[2]
    rms = float(np.sqrt(((got.x[:, :3] - xo[:, :3]) ** 2).sum(1).mean()))
    print(f"RMS position difference vs oracle over {S} epochs with a dt per epoch: {rms:.3e} m")
    assert rms <= 1e-6, rms
