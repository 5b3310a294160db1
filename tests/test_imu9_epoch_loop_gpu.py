"""The epoch loop of the 9-state kernel (k_step_imu9): what it reads ahead and what it stores early must stay invisible.
In a multi-epoch launch the kernel reads the next epoch's dt (scalar, from the kernel arguments) and accelerometer
sample one epoch ahead, stores the pose before the covariance update, and runs the diagonal form of the gain iteration
in wavefronts whose accelerometer covariances are all diagonal. Every comparison here is bit for bit: the pose of every
epoch, x, P, flags and status words.

The synthetic trace has the same dt in every epoch after the first, which would hide an off-by-one in the dt that is read
ahead: these tests give every epoch its own."""

import numpy as np
import pytest

import replay_checks as rc
from conftest import has_gpu
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu


def _dts(S):
    return np.array([0.03 + 0.01 * (s % 5) for s in range(S)])


def _trace(w, S, storage, dev, cov=None):
    import torch
    from roskfpos_amd import capi
    real = np.float64 if storage == capi.STORE_F64 else np.float32
    r = np.stack([w.ranges_mm(s) for s in range(S)])
    if S > 4:
        r[2, ::7, 1] = -1      # an absent range
        r[4, 1::9, 2:] = 0     # fewer than four ranges: no update for these tags in this epoch
    cov = w.accel_cov(real) if cov is None else cov.astype(real)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return dict(r=up(r.transpose(0, 2, 1)), e=up(w.err_est(real).T), c=up(cov.T),
                a=up(np.stack([w.accel(s, real) for s in range(S)]).transpose(0, 2, 1)), r_host=r, cov_host=cov)


def _bank(w, T, storage, chunk=None, diag=None, init=True):
    from roskfpos_amd import capi
    with rc.env(KFPOS_TRACE_CHUNK_STEPS=chunk, KFPOS_IMU9_DIAG=diag):
        return capi.KfposBank(capi.MODEL_TOA_IMU, T, w.anchors, storage=storage,
                              init_pos=w.init_positions() if init else None)


def _fused(b, tr, S, dts, T, A, with_traj=True, accel=True, s0=0):
    """kfpos_run_trace_dev over epochs s0 .. s0 + S - 1 -> (trajectory, status, x, P, flags, latch)"""
    import torch
    dev = tr["r"].device
    traj = torch.zeros(S, 3, T, dtype=torch.float64, device=dev) if with_traj else None
    st = torch.zeros(T, dtype=torch.int32, device=dev)
    kw = dict(accel=tr["a"][s0], stride_accel=3 * T, cov=tr["c"], stride_cov=0) if accel else {}
    b.run_trace_dev(S, tr["r"][s0], A * T, tr["e"], 0, dts[s0:s0 + S], trajectory=traj, status=st,
                    stream=torch.cuda.current_stream().cuda_stream, **kw)
    torch.cuda.synchronize()
    x, P, fl = b.get_state()
    return (traj.cpu().numpy() if with_traj else None, st.cpu().numpy(), x, P, fl, b.get_latch())


def _per_epoch(b, tr, S, dts, T, accel=True, s0=0):
    """the single-epoch entry points, one launch per epoch -> (None, status of every epoch, x, P, flags, latch)"""
    import torch
    st = torch.zeros(T, dtype=torch.int32, device=tr["r"].device)
    stream = torch.cuda.current_stream().cuda_stream
    stats = []
    for s in range(s0, s0 + S):
        if accel:
            b.step_toa_imu_dev(tr["r"][s], tr["e"], tr["a"][s], tr["c"], dts[s], status=st, stream=stream)
        else:
            b.step_toa_dev(tr["r"][s], tr["e"], dts[s], status=st, stream=stream)
        stats.append(st.cpu().numpy().copy())
    x, P, fl = b.get_state()
    return (None, np.stack(stats), x, P, fl, b.get_latch())


def _same(got, ref, what, traj=True):
    if traj:
        assert np.array_equal(got[0], ref[0], equal_nan=True), (what, "pose of every epoch")
    assert np.array_equal(got[1], ref[1]), (what, "status")
    assert np.array_equal(got[2], ref[2], equal_nan=True), (what, "x")
    assert np.array_equal(got[3], ref[3], equal_nan=True), (what, "P")
    assert np.array_equal(got[4], ref[4]), (what, "flags")
    assert np.array_equal(got[5], ref[5], equal_nan=True), (what, "latch")


@pytest.mark.parametrize("A", [8, 5])               # the 8-anchor kernel (epoch in registers), the run-time-loop kernel
@pytest.mark.parametrize("storage", [0, 1, 2, 3])   # f64, f32, mixed, p48
@pytest.mark.parametrize("T", [64, 130])            # one wavefront; two full ones and one of two lanes
def test_fused_launches_equal_single_epoch_launches_with_a_dt_per_epoch(T, storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    S = 7
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    b = _bank(w, T, storage)
    ref = _per_epoch(b, tr, S, dts, T)
    b.close()
    st = (ref[1] & 0xFF)
    assert (ref[1][4, 1::9] & 0xFF != 0).all() and (st == 0).mean() > 0.5   # the few-ranges path ran, most steps are plain
    poses = None
    for chunk in (1, 2, 3, 7, 25):      # 1: one launch per epoch through the trace entry point; its poses are the reference
        b = _bank(w, T, storage, chunk=chunk)
        got = _fused(b, tr, S, dts, T, A)
        b.close()
        poses = got[0] if poses is None else poses
        _same(got, (poses, ref[1][-1]) + ref[2:], f"chunk {chunk}")
        if chunk == 7:
            b = _bank(w, T, storage, chunk=chunk)
            bare = _fused(b, tr, S, dts, T, A, with_traj=False)
            b.close()
            _same(bare, got, "trajectory=None", traj=False)


@pytest.mark.parametrize("storage", [0, 2])
def test_ml_initialisation_inside_a_fused_launch(storage):
    """no start position: every tag initialises from its first ML solve (a step that leaves early), some of them late"""
    if not has_gpu():
        pytest.skip("no GPU")
    T, A, S = 130, 8, 7
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    tr["r"][0, 2:, 3::5] = 0          # too few ranges in epoch 0 for every fifth tag: it initialises one epoch later
    b = _bank(w, T, storage, init=False)
    ref = _per_epoch(b, tr, S, dts, T)
    b.close()
    poses = None
    for chunk in (1, 3, 7):
        b = _bank(w, T, storage, chunk=chunk, init=False)
        got = _fused(b, tr, S, dts, T, A)
        b.close()
        poses = got[0] if poses is None else poses
        _same(got, (poses, ref[1][-1]) + ref[2:], f"chunk {chunk}")
    assert np.isnan(poses[0, 0, 3::5]).all() and np.isfinite(poses[1]).all()   # late starters waited one epoch
    assert (ref[1][0, 3::5] & 0xFF == 0x04).all() and (ref[1][1, 3::5] & 0x08 != 0).all()   # few ranges, then ML init


@pytest.mark.parametrize("storage,A", [(2, 8), (0, 8), (3, 5)])
def test_refuse_of_the_latched_sample(storage, A):
    """ranging-only epochs on a 9-state bank re-fuse the sample the last fused step latched"""
    if not has_gpu():
        pytest.skip("no GPU")
    T, S = 130, 7
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    b = _bank(w, T, storage)
    _per_epoch(b, tr, 1, dts, T)
    ref = _per_epoch(b, tr, S - 1, dts, T, accel=False, s0=1)
    b.close()
    poses = None
    for chunk in (1, 2, 25):
        b = _bank(w, T, storage, chunk=chunk)
        _fused(b, tr, 1, dts, T, A)
        got = _fused(b, tr, S - 1, dts, T, A, accel=False, s0=1)
        b.close()
        poses = got[0] if poses is None else poses
        _same(got, (poses, ref[1][-1]) + ref[2:], f"chunk {chunk}")


def test_the_diagonal_form_is_invisible():
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    T, A, S, storage = 192, 8, 30, capi.STORE_MIXED
    w = Workload(T, A)
    dts = np.array([w.dt_of(s) for s in range(S)])
    tr_a = _trace(w, S, storage, "cuda:0")
    cov_b = w.accel_cov().copy()
    cov_b[5::64, 1] = cov_b[5::64, 3] = 1e-3      # lane 5 of every wavefront: an off-diagonal of 1e-3 m^2/s^4
    tr_b = _trace(w, S, storage, "cuda:0", cov=cov_b)
    out = {}
    for name, tr, diag in (("A", tr_a, None), ("A full", tr_a, 0), ("B", tr_b, None), ("B full", tr_b, 0)):
        b = _bank(w, T, storage, diag=diag)
        out[name] = _fused(b, tr, S, dts, T, A)
        b.close()
    b = _bank(w, T, storage)
    per_epoch = _per_epoch(b, tr_a, S, dts, T)
    b.close()
    assert (((per_epoch[1] >> 8) & 0xFF) == 20).any()         # capped steps are in it
    _same(out["A"], (None, per_epoch[1][-1]) + per_epoch[2:], "fused against per-epoch launches", traj=False)
    _same(out["A"], out["A full"], "all diagonal: default against KFPOS_IMU9_DIAG=0")
    _same(out["B"], out["B full"], "one lane per wavefront not diagonal: default against KFPOS_IMU9_DIAG=0")
    others = np.ones(T, dtype=bool)
    others[5::64] = False
    a_, b_ = out["A"], out["B"]
    assert np.array_equal(a_[0][:, :, others], b_[0][:, :, others]), "poses of the other tags"
    assert np.array_equal(a_[1][others], b_[1][others]), "status words of the other tags"
    assert np.array_equal(a_[2][others], b_[2][others]) and np.array_equal(a_[3][others], b_[3][others])
    assert np.array_equal(a_[4][others], b_[4][others])
    assert not np.array_equal(a_[2][~others], b_[2][~others])  # (the off-diagonal does reach the filter)


def test_fused_launches_with_a_dt_per_epoch_match_the_oracle():
    if not has_gpu():
        pytest.skip("no GPU")
    import oracle_py
    from roskfpos_amd import capi
    T, A, S, storage = 128, 8, 40, capi.STORE_MIXED
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    b = _bank(w, T, storage)
    got = _fused(b, tr, S, dts, T, A)
    b.close()
    o = oracle_py.OracleBank(1, T, w.anchors, init_pos=w.init_positions(), n_threads=8)
    err, cov = w.err_est(np.float32).astype(np.float64), tr["cov_host"].astype(np.float64)
    for s in range(S):
        o.step_imu(w.accel(s, np.float32).astype(np.float64), cov, 0.0)
        o.step_toa(tr["r_host"][s], err, dts[s])
    xo, _ = o.get_state()
    rms = float(np.sqrt(((got[2][:, :3] - xo[:, :3]) ** 2).sum(1).mean()))
    print(f"RMS position difference vs oracle over {S} epochs with a dt per epoch: {rms:.3e} m")
    assert rms <= 1e-6, rms
