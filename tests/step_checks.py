"""What the tests of the step side of the filters share (the 9-state kernel's forms above all): a trace on the device,
a bank created under chosen KFPOS_* variables, the trace's epochs as single _dev calls, as one kfpos_run_trace_dev call
and as two, the byte comparison of what they leave, and the same trace through the oracle. The step-side sibling of
replay_checks.py. A test file keeps its scenarios, shapes, tolerances and "this really occurred" assertions.

Nothing here needs a GPU: with dev="cpu" and a stand-in bank (tests/test_step_checks.py) every function runs on the CPU.
torch is imported where a tensor is made."""
import collections

import numpy as np

from replay_checks import env, same_bytes, up
from roskfpos_amd import capi

FL_STARTED, FL_HAS_IMU = np.uint32(1), np.uint32(2)     # the flags word of get_state(): kfpos_core.h
UNSET = None                                            # bank(pairs=UNSET): KFPOS_PAIR9 unset, the library's default


def dts(S):
    """a dt of its own for every epoch (the synthetic trace's is the same from the second on)"""
    return np.array([0.03 + 0.01 * (s % 5) for s in range(S)])


def real_of(storage):
    """the element type of a bank's measurements"""
    return np.float64 if storage == capi.STORE_F64 else np.float32


class Trace:
    """S epochs of measurements as the _dev calls take them, component-major on `dev`: r [S][A][T] int32, err [A][T],
    accel [S][3][T], cov [9][T]; and the host copies r_host [S][T][A], cov_host [T][9]. What is not given comes from
    the workload w: r [S][T][A], err [T][A], accel [S][T][3], cov [T][9].
    gaps: an absent range in epoch 2 (every 7th tag) and fewer than four ranges in epoch 4 (every 9th from the second:
    no update for these tags in this epoch)"""

    def __init__(self, w, S, storage, dev="cuda:0", *, r=None, err=None, accel=None, cov=None, gaps=False):
        real = real_of(storage)
        r = np.stack([w.ranges_mm(s) for s in range(S)]) if r is None else r
        if gaps:
            r[2, ::7, 1] = -1
            r[4, 1::9, 2:] = 0
        err = (w.err_est() if err is None else err).astype(real)
        accel = (np.stack([w.accel(s) for s in range(S)]) if accel is None else accel).astype(real)
        cov = (w.accel_cov() if cov is None else cov).astype(real)
        self.S, self.T, self.A = r.shape
        self.r, self.err = up(r.transpose(0, 2, 1), dev), up(err.T, dev)
        self.accel, self.cov = up(accel.transpose(0, 2, 1), dev), up(cov.T, dev)
        self.r_host, self.cov_host = r, cov

    def stream(self):
        """-> (the current stream's handle, a function that waits for it); (None, nothing) for a trace on the CPU"""
        if self.r.device.type != "cuda":
            return None, lambda: None
        import torch
        return torch.cuda.current_stream().cuda_stream, torch.cuda.synchronize


def bank(w, T, storage, *, model=capi.MODEL_TOA_IMU, init=True, chunk=None, diag=None, pairs=UNSET, meet=None,
         no_coop=None):
    """a capi.KfposBank created under exactly these variables (None: unset). init: True = the workload's fixed starts,
    False = none (every tag starts from its first ML solve), or an array [T][3]"""
    init = w.init_positions() if init is True else None if init is False else init
    with env(KFPOS_TRACE_CHUNK_STEPS=chunk, KFPOS_IMU9_DIAG=diag, KFPOS_PAIR9=pairs, KFPOS_PAIR9_MEET=meet,
             KFPOS_NO_COOP=no_coop):
        return capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=init)


class Run(collections.namedtuple("Run", "poses status x P flags latch")):
    """what a run leaves: the pose after every epoch [n][3][T] (or None), the status words (of every epoch [n][T] from
    single calls, of the last epoch [T] from a launch), and the bank's state, covariance, flags and latch"""
    __slots__ = ()

    def only(self, keep):
        """the entries of the tags in the mask `keep`"""
        return Run(None if self.poses is None else self.poses[:, :, keep], self.status[..., keep],
                   *(v[keep] for v in self[2:]))

    def last(self, poses=None):
        """single calls as a launch over the same epochs reports them: the last epoch's status words (and these poses)"""
        return self._replace(status=self.status[-1], poses=self.poses if poses is None else poses)


def _left(b, poses, status):
    x, P, fl = b.get_state()
    return Run(poses, status, x, P, fl, b.get_latch())


def single_calls(b, tr, dts, n, s0=0, accel=True, poses=True):
    """epochs s0 .. s0 + n - 1 as n single-epoch _dev calls (accel=False: ranging-only calls) -> Run with the status
    words of every epoch; poses: read the pose after every call (else None)"""
    import torch
    st = torch.zeros(tr.T, dtype=torch.int32, device=tr.r.device)
    stream, _ = tr.stream()
    seen, stats = [], []
    for s in range(s0, s0 + n):
        if accel:
            b.step_toa_imu_dev(tr.r[s], tr.err, tr.accel[s], tr.cov, dts[s], status=st, stream=stream)
        else:
            b.step_toa_dev(tr.r[s], tr.err, dts[s], status=st, stream=stream)
        stats.append(st.cpu().numpy().copy())
        if poses:
            seen.append(b.get_state()[0][:, :3].T.copy())
    return _left(b, np.stack(seen) if poses else None, np.stack(stats))


def fused(b, tr, dts, n, s0=0, accel=True, with_traj=True):
    """the same epochs as one kfpos_run_trace_dev call -> Run with the last epoch's status words"""
    import torch
    dev = tr.r.device
    traj = torch.zeros(n, 3, tr.T, dtype=torch.float64, device=dev) if with_traj else None
    st = torch.zeros(tr.T, dtype=torch.int32, device=dev)
    kw = dict(accel=tr.accel[s0], stride_accel=3 * tr.T, cov=tr.cov, stride_cov=0) if accel else {}
    stream, wait = tr.stream()
    b.run_trace_dev(n, tr.r[s0], tr.A * tr.T, tr.err, 0, dts[s0:s0 + n], trajectory=traj, status=st, stream=stream, **kw)
    wait()
    return _left(b, traj.cpu().numpy() if with_traj else None, st.cpu().numpy())


def fused_split(b, tr, dts, n, s0=0, accel=True, *, split):
    """the same epochs as two calls, of split and n - split epochs, their poses concatenated"""
    first = fused(b, tr, dts, split, s0, accel)
    second = fused(b, tr, dts, n - split, s0 + split, accel)
    return second._replace(poses=np.concatenate([first.poses, second.poses]))


def same(got, ref, what, fields=Run._fields):
    """shape, dtype and bytes of the named fields of two Runs: the sign of a zero and a NaN's payload count"""
    same_bytes([getattr(got, f) for f in fields], [getattr(ref, f) for f in fields], fields, what)


def oracle_run(w, r, err, dts, *, model=1, real, init, accel=True, cov=None, edit=None):
    """r [S][T][A] and err [T][A] through the oracle, with the workload's accelerometer samples (of its first T tags)
    rounded to `real` as the bank holds them; accel: one flag, or one per epoch, whether the epoch fuses a sample;
    edit(oracle, s) runs before epoch s -> (poses [S][T][3], status [S][T] uint32, final x, final P)"""
    import oracle_py
    S, T = r.shape[:2]
    o = oracle_py.OracleBank(model, T, w.anchors, init_pos=init, n_threads=8)
    err = np.asarray(err).astype(real).astype(np.float64)
    cov = (w.accel_cov() if cov is None else cov).astype(real).astype(np.float64)[:T]
    poses, stats = [], []
    for s in range(S):
        if edit:
            edit(o, s)
        if model == capi.MODEL_TOA_IMU and np.broadcast_to(accel, S)[s]:
            o.step_imu(w.accel(s, real).astype(np.float64)[:T], cov, 0.0)
        stats.append(np.asarray(o.step_toa(r[s], err, dts[s])).astype(np.uint32))
        poses.append(o.get_state()[0][:, :3].copy())
    return (np.stack(poses), np.stack(stats)) + tuple(o.get_state())


def first_seed(seeds, occurs, what):
    """the first workload seed for which occurs(seed) holds: how a test chooses, with the oracle on the CPU, a trace in
    which its scenario `what` occurs"""
    for seed in seeds:
        if occurs(seed):
            return seed
    raise AssertionError(f"no seed in {seeds[0]} .. {seeds[-1]} for which the oracle sees {what}")
