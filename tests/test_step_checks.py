"""tests/step_checks.py judged on the CPU: a stand-in bank whose state is a running digest of exactly the bytes it was
handed, epoch by epoch, takes the place of capi.KfposBank, and the trace lives in host memory. So single_calls, fused and
fused_split leave the same Run exactly when they hand over the same epochs in the same order; same() has to see what
value equality does not; bank() has to create under the variables it was asked for and no others."""
import hashlib
import os

import numpy as np
import pytest
import torch

import step_checks as sc
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload

T, A, S = 11, 4, 9
VARS = ("KFPOS_TRACE_CHUNK_STEPS", "KFPOS_IMU9_DIAG", "KFPOS_PAIR9", "KFPOS_PAIR9_MEET", "KFPOS_NO_COOP")


def _bytes(*arrays):
    return b"".join(b"-" if a is None else np.ascontiguousarray(a).tobytes() for a in arrays)


class StandIn:
    """the calls of capi.KfposBank the harness makes. Everything it reports is spread from its digest."""

    def __init__(self):
        self.digest, self.epochs = b"", []

    def _spread(self, shape, dtype, salt):
        n = int(np.prod(shape))
        raw = np.frombuffer(hashlib.sha256(self.digest + salt).digest(), dtype=np.uint8)
        return (np.resize(raw, n).astype(np.int64) * 131 + np.arange(n)).astype(dtype).reshape(shape)

    def _epoch(self, r, err, accel, cov, dt, status, stream):
        assert stream is None                            # a trace on the CPU asks for no stream
        handed = _bytes(*(None if a is None else a.numpy() for a in (r, err, accel, cov)), np.float64(dt))
        self.epochs.append(handed)
        self.digest = hashlib.sha256(self.digest + handed).digest()
        status.copy_(torch.from_numpy(self._spread((T,), np.int32, b"status")))

    def step_toa_imu_dev(self, r, err, accel, cov, dt, status=None, stream=None):
        self._epoch(r, err, accel, cov, dt, status, stream)

    def step_toa_dev(self, r, err, dt, status=None, stream=None):
        self._epoch(r, err, None, None, dt, status, stream)

    def run_trace_dev(self, n, r, stride_r, err, stride_err, dts, accel=None, stride_accel=0, cov=None, stride_cov=0,
                      trajectory=None, status=None, stream=None):
        def at(a, e, stride):       # the tensor `stride` elements times e further on, as the library's pointer sum
            return None if a is None else torch.as_strided(a, a.shape, a.stride(), a.storage_offset() + e * stride)

        assert len(dts) == n
        for e in range(n):
            self._epoch(at(r, e, stride_r), at(err, e, stride_err), at(accel, e, stride_accel), at(cov, e, stride_cov),
                        dts[e], status, stream)
            if trajectory is not None:
                trajectory[e] = torch.from_numpy(self.get_state()[0][:, :3].T.copy())

    def get_state(self):
        return self._spread((T, 9), np.float64, b"x"), self._spread((T, 9, 9), np.float64, b"P"), \
            self._spread((T,), np.uint32, b"flags")

    def set_state(self, x, P, flags=None):
        self.digest = hashlib.sha256(self.digest + _bytes(x, P, flags)).digest()

    def get_latch(self):
        return self._spread((T, 3), np.float64, b"latch")

    def close(self):
        pass


@pytest.fixture(scope="module")
def trace():
    rng = np.random.default_rng(5)
    return sc.Trace(None, S, capi.STORE_MIXED, "cpu", r=rng.integers(-1, 9000, (S, T, A), dtype=np.int32),
                    err=rng.random((T, A)), accel=rng.standard_normal((S, T, 3)), cov=rng.random((T, 9)))


def test_a_trace_holds_what_it_was_given_component_major_and_the_gaps_are_an_option(trace):
    assert (trace.S, trace.T, trace.A) == (S, T, A) and trace.r.dtype == torch.int32 and trace.err.dtype == torch.float32
    assert np.array_equal(trace.r.numpy(), trace.r_host.transpose(0, 2, 1))
    assert np.array_equal(trace.cov.numpy(), trace.cov_host.T) and trace.accel.shape == (S, 3, T)
    w = Workload(20, A)
    plain, gaps = sc.Trace(w, 5, capi.STORE_F64, "cpu"), sc.Trace(w, 5, capi.STORE_F64, "cpu", gaps=True)
    assert plain.err.dtype == torch.float64 and np.array_equal(plain.r_host[3], w.ranges_mm(3)) and (plain.r_host > 0).all()
    changed = plain.r_host != gaps.r_host
    assert (gaps.r_host[2, ::7, 1] == -1).all() and (gaps.r_host[4, 1::9, 2:] == 0).all()
    assert changed.sum() == changed[2, ::7, 1].sum() + changed[4, 1::9, 2:].sum() == 3 + 3 * (A - 2)
    assert np.array_equal(sc.dts(7), [0.03, 0.04, 0.05, 0.06, 0.07, 0.03, 0.04])


@pytest.mark.parametrize("accel", [True, False])
@pytest.mark.parametrize("s0", [0, 3])
def test_the_three_ways_hand_over_the_same_epochs_in_the_same_order(trace, s0, accel):
    n, dts = 5, sc.dts(S)
    banks = [StandIn(), StandIn(), StandIn(), StandIn()]
    single = sc.single_calls(banks[0], trace, dts, n, s0, accel)
    fused = sc.fused(banks[1], trace, dts, n, s0, accel)
    split = sc.fused_split(banks[2], trace, dts, n, s0, accel, split=2)
    bare = sc.fused(banks[3], trace, dts, n, s0, accel, with_traj=False)
    real = np.float32
    want = [_bytes(trace.r_host[s].T, trace.err.numpy(), trace.accel.numpy()[s] if accel else None,
                   trace.cov_host.T.astype(real) if accel else None, np.float64(dts[s])) for s in range(s0, s0 + n)]
    for b in banks:
        assert b.epochs == want
    assert single.status.shape == (n, T) and fused.status.shape == (T,) and single.poses.shape == (n, 3, T)
    sc.same(fused, single.last(), "one call against single calls")
    sc.same(split, fused, "two calls against one")
    assert bare.poses is None
    sc.same(bare, fused, "without a trajectory", sc.Run._fields[1:])
    assert sc.single_calls(StandIn(), trace, dts, n, s0, accel, poses=False).poses is None
    # another epoch, another order, another dt: another Run
    other = sc.fused(StandIn(), trace, dts, n, s0 + 1, accel)
    with pytest.raises(AssertionError):
        sc.same(other, fused, "the epochs one further on")


def _differs(run, field, how):
    a = getattr(run, field).copy()
    if how == "the sign of a zero":
        a.flat[0] = -0.0
    elif how == "a NaN payload":
        a.view(np.uint64).flat[0] ^= 1
    elif how == "a dtype":
        a = a.view(np.int32)
    else:
        a.flat[3] ^= 1 << 8
    return run._replace(**{field: a})


@pytest.mark.parametrize("field,how", [("x", "the sign of a zero"), ("poses", "a NaN payload"), ("P", "a NaN payload"),
                                       ("flags", "a dtype"), ("status", "one status word"),
                                       ("latch", "the sign of a zero")])
def test_same_fails_on_one_difference_value_equality_may_miss_and_names_the_field(trace, field, how):
    ref = sc.fused(StandIn(), trace, sc.dts(S), 4)
    ref.x.flat[0] = ref.latch.flat[0] = 0.0
    ref.poses.flat[0] = ref.P.flat[0] = np.nan
    sc.same(ref, ref._replace(x=ref.x.copy()), "a copy")
    got = _differs(ref, field, how)
    if how != "one status word":
        assert np.array_equal(getattr(got, field), getattr(ref, field), equal_nan=True)     # ... to value equality
    with pytest.raises(AssertionError) as failure:
        sc.same(got, ref, "one difference")
    assert failure.value.args[0] == ("one difference", field)
    sc.same(got, ref, "the other fields", [f for f in sc.Run._fields if f != field])


def test_only_and_last():
    run = sc.Run(np.arange(24.).reshape(2, 3, 4), np.arange(8).reshape(2, 4), np.arange(36.).reshape(4, 9),
                 np.zeros((4, 9, 9)), np.arange(4, dtype=np.uint32), np.zeros((4, 3)))
    keep = np.array([True, False, True, True])
    part = run.only(keep)
    assert part.poses.shape == (2, 3, 3) and part.status.shape == (2, 3) and part.x.shape == (3, 9)
    assert np.array_equal(part.flags, [0, 2, 3]) and part.P.shape == (3, 9, 9) and part.latch.shape == (3, 3)
    assert np.array_equal(run.last().status, [4, 5, 6, 7]) and run.last().poses is run.poses
    assert run.last(run.poses[:1]).poses.shape == (1, 3, 4) and run.last().only(keep).status.shape == (3,)


def test_bank_creates_under_exactly_the_requested_variables_and_restores_the_environment(monkeypatch):
    seen = []

    def recorder(model, n_tags, anchors, storage=None, init_pos=None):
        seen.append(({k: os.environ.get(k) for k in VARS}, model, n_tags, storage, init_pos))
        return "a bank"

    monkeypatch.setattr(capi, "KfposBank", recorder)
    monkeypatch.setenv("KFPOS_PAIR9", "1")
    monkeypatch.setenv("KFPOS_NO_COOP", "1")
    monkeypatch.delenv("KFPOS_TRACE_CHUNK_STEPS", raising=False)
    before = dict(os.environ)
    w = Workload(T, A)
    unset = dict.fromkeys(VARS)
    assert sc.bank(w, T, 2) == "a bank"
    assert seen[-1][0] == unset and seen[-1][1:4] == (capi.MODEL_TOA_IMU, T, 2)
    assert np.array_equal(seen[-1][4], w.init_positions())
    sc.bank(w, T, 3, chunk=7, pairs=0, init=False)
    assert seen[-1][0] == dict(unset, KFPOS_TRACE_CHUNK_STEPS="7", KFPOS_PAIR9="0") and seen[-1][4] is None
    start = np.ones((T, 3))
    sc.bank(w, T, 0, model=capi.MODEL_TOA, init=start, diag=0, pairs=sc.UNSET, meet="7,10", no_coop=1)
    assert seen[-1][0] == dict(unset, KFPOS_IMU9_DIAG="0", KFPOS_PAIR9_MEET="7,10", KFPOS_NO_COOP="1")
    assert seen[-1][1] == capi.MODEL_TOA and seen[-1][4] is start
    assert dict(os.environ) == before

    def refuses(*a, **kw):
        raise capi.KfposError("no")

    monkeypatch.setattr(capi, "KfposBank", refuses)
    with pytest.raises(capi.KfposError):
        sc.bank(w, T, 2, chunk=3, pairs=0)
    assert dict(os.environ) == before


def test_first_seed_takes_the_first_that_qualifies_and_names_the_scenario_when_none_does():
    asked = []
    assert sc.first_seed(range(1, 9), lambda seed: asked.append(seed) or seed % 3 == 0, "a multiple of three") == 3
    assert asked == [1, 2, 3]
    with pytest.raises(AssertionError, match="no seed in 1 .. 8 .* a multiple of eleven"):
        sc.first_seed(range(1, 9), lambda seed: seed % 11 == 0, "a multiple of eleven")


def test_oracle_run_edits_before_each_epoch_and_fuses_a_sample_where_asked():
    w = Workload(4, 8)
    r = np.stack([w.ranges_mm(s) for s in range(3)])
    seen = []
    poses, status, x, P = sc.oracle_run(w, r, w.err_est(), sc.dts(3), real=np.float32, init=w.init_positions(),
                                        edit=lambda o, s: seen.append((s, o.get_state()[0].copy())))
    assert [s for s, _ in seen] == [0, 1, 2] and np.array_equal(seen[0][1][:, :3], w.init_positions())
    assert poses.shape == (3, 4, 3) and status.shape == (3, 4) and status.dtype == np.uint32
    assert np.array_equal(poses[1], seen[2][1][:, :3]) and np.array_equal(poses[2], x[:, :3]) and P.shape == (4, 9, 9)
    ranging_only = sc.oracle_run(w, r, w.err_est(), sc.dts(3), real=np.float32, init=w.init_positions(), accel=False)
    late = sc.oracle_run(w, r, w.err_est(), sc.dts(3), real=np.float32, init=w.init_positions(),
                         accel=[True, True, False])
    assert not np.array_equal(ranging_only[2], x)
    assert np.array_equal(late[0][:2], poses[:2]) and not np.array_equal(late[2], x)
    assert sc.oracle_run(w, r, w.err_est(), sc.dts(3), model=0, real=np.float64, init=w.init_positions())[2].shape == (4, 6)
