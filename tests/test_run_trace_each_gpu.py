"""kfpos_run_trace_each_dev: ranging slots of the 6-state filter in which every tag has a timeline of its own, in one
launch, compute bit for bit what the same slots give as single kfpos_step_toa_dev calls with a per-tag dt array -- state,
covariance as stored, flags, the status word and the position of every slot -- and stay with the oracle after every slot.

One schedule serves every test: SLOTS ranging slots from cases.Case.epoch (dropout rows inside) and an explicit
participation mask over 130 tags whose properties the first test asserts. The single-call reference of a configuration
is computed once and shared by the launch sizes compared against it (tests/replay_checks.py)."""
import ctypes
import functools
import types

import numpy as np
import pytest

import replay_checks as rc
from cases import Case, rms_and_max
from conftest import has_gpu
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

T = 130                                       # two full wavefronts and one of two lanes
SLOTS = 37
DT_ZERO = 10                                  # a slot in which every participant has dt = 0
WAVE_OUT = (9, 17)                            # slots nobody of tags 64..127 takes part in
LATE, LATE_FIRST = 7, 5                       # tag 7 first takes part in slot 5
ABSENT_MM = 1999999999                        # what the ranges of an absent (tag, slot) pair hold
ST_SKIPPED, ST_ML_INIT = 64, 8
FL_STARTED = 1
ERR_ARG, ERR_MODEL, ERR_STATE = 1, 4, 5
F64, F32, MIXED, P48 = 0, 1, 2, 3
NO_COOP = {"KFPOS_NO_COOP": 1}


def _mask(slots=SLOTS):
    """who takes part in which slot: (slots, T) bool"""
    m = np.random.default_rng(20261018).random((slots, T)) < 0.65
    m[:, 0] = True
    m[:, 5] = False
    for e in WAVE_OUT:
        m[e, 64:128] = False
    m[-1, 128] = False
    m[:LATE_FIRST, LATE] = False
    m[LATE_FIRST, LATE] = True
    return m


def test_the_schedule_holds_what_it_is_meant_to_hold():
    m = _mask()
    assert 35 <= SLOTS <= 39 and m.shape == (SLOTS, T) and T == 2 * 64 + 2
    assert m[:, 0].all() and not m[:, 5].any()
    assert len(WAVE_OUT) == 2 and not m[list(WAVE_OUT), 64:128].any()
    assert m[list(WAVE_OUT), :64].any(axis=1).all()             # while the first wavefront runs those slots
    assert not m[-1, 128] and m[:-1, 128].any()
    assert int(np.flatnonzero(m[:, LATE])[0]) == LATE_FIRST > 0
    assert 0.40 <= m.mean() <= 0.80
    assert (m.all(axis=0).sum(), (~m).all(axis=0).sum()) == (1, 1)   # only tag 0 is everywhere, only tag 5 nowhere
    assert m[DT_ZERO].sum() > 1 and DT_ZERO not in WAVE_OUT
    # the dropout rows of cases.Case.epoch fall among the slots, and tags take part in them
    for mod, rem in ((7, 3), (11, 5), (23, 9)):
        assert any(s % mod == rem and m[s].sum() > 1 for s in range(SLOTS))
    assert SLOTS % 7 != 0                                       # launches of 7 slots: the last one is a short one
    long = _mask(130)                                           # the schedule that crosses the 128-slot launch boundary
    assert long.shape == (130, T) and long[127].any() and long[128].any() and long[129].any()


class Inputs:
    """the schedule's inputs in HBM (component-major), and on the host in the (T, A) form the oracle takes"""

    def __init__(self, A, storage, fixed=True, ignore_worst=False, top_n=0, slots=SLOTS, env=None, tags=T, dev="cuda:0"):
        """tags: the bank holds the first `tags` columns of the 130-tag schedule"""
        n = self.T = tags
        self.A, self.storage, self.fixed = A, storage, fixed
        self.ignore_worst, self.top_n, self.env = ignore_worst, top_n, dict(env or {})
        real = self.real = np.float64 if storage == F64 else np.float32
        case = Case("each", 0, A, fixed=fixed, T=T, outlier=bool(ignore_worst or top_n))
        w = Workload(T, A)
        self.anchors, self.init = w.anchors, w.init_positions()[:n]
        self.slots, self.kinds = slots, np.zeros(slots, dtype=np.uint8)   # ranging slots only
        self.mask = _mask(slots)[:, :n]
        base = np.round(np.random.default_rng(20261017).uniform(0.02, 0.12, slots), 4)
        base[DT_ZERO] = 0.0
        self.dt = np.where(self.mask, base[:, None], -1.0)                        # (S, T)
        self.ranges = np.stack([case.epoch(w, s) for s in range(slots)])[:, :n]    # (S, T, A), dropout rows kept
        self.ranges[~self.mask] = ABSENT_MM
        self.err = w.err_est(real)[:n]
        up = lambda a: rc.up(a, dev)  # noqa: E731
        self.d_r, self.d_e, self.d_dt = up(self.ranges.transpose(0, 2, 1)), up(self.err.T), up(self.dt)
        assert n == self.d_dt.shape[1]

    def bank(self, chunk=None):
        from roskfpos_amd import capi
        with rc.env(KFPOS_TRACE_CHUNK_STEPS=chunk, **self.env):
            return capi.KfposBank(capi.MODEL_TOA, self.T, self.anchors, storage=self.storage,
                                  ignore_worst=self.ignore_worst, top_n=self.top_n,
                                  init_pos=self.init if self.fixed else None)


def _single(b, inp, e, kind, i, status, stream, dt):
    b.step_toa_dev(inp.d_r[e], inp.d_e, 0.0, status=status, stream=stream, dt_dev=dt)


def _call(b, inp, n, dts, traj, sts, st, stream):
    b.run_trace_each_dev(dts, inp.d_r, inp.A * inp.T, inp.d_e, 0, trajectory=traj, status_steps=sts, status=st,
                         stream=stream)


NAMES = ("position after every slot", "status of every slot", "x", "P", "flags")
FAM = rc.Family(names=NAMES, n_kinds=1, dts=lambda inp: inp.d_dt, final=lambda b: b.get_state(),
                position=lambda b: b.get_state()[0][:, :3].T, single=_single, call=_call)


CONFIGS = {
    # A = 8, fixed start, no heuristic: the epoch in registers
    "A8 fixed f64": dict(A=8, storage=F64, env=NO_COOP),
    "A8 fixed mixed": dict(A=8, storage=MIXED, env=NO_COOP),
    "A8 fixed p48": dict(A=8, storage=P48, env=NO_COOP),
    "A8 fixed f32": dict(A=8, storage=F32, env=NO_COOP),
    # ML start: the full covariance layout, compile-time loops over the LDS-resident epoch
    "A8 ml f64": dict(A=8, storage=F64, fixed=False),
    "A8 ml mixed": dict(A=8, storage=MIXED, fixed=False),
    "A8 ml p48": dict(A=8, storage=P48, fixed=False),
    "A8 fixed ignore_worst mixed": dict(A=8, storage=MIXED, ignore_worst=True),
    "A16 fixed top3 mixed": dict(A=16, storage=MIXED, top_n=3),
    "A16 fixed top3 p48": dict(A=16, storage=P48, top_n=3),
    "A16 ml ignore_worst mixed": dict(A=16, storage=MIXED, fixed=False, ignore_worst=True),
    # run-time anchor loop
    "A5 fixed mixed": dict(A=5, storage=MIXED, env=NO_COOP),
    "A5 ml mixed": dict(A=5, storage=MIXED, fixed=False),
    "A8 fixed mixed generic": dict(A=8, storage=MIXED, env={"KFPOS_GENERIC_KERNEL": 1}),
    # no environment: the handle runs the 8-lanes-per-tag kernel, the call one launch per slot
    "A8 fixed mixed coop": dict(A=8, storage=MIXED),
    # more than 64 KB of LDS, so k_trace_toa6_each runs behind a raised hipFuncAttributeMaxDynamicSharedMemorySize: the
    # run-time loop's epoch alone from 43 anchors (66 048 bytes; 42: 64 512), with Pinv6 of the ML start behind it from 31
    # (66 048; 30: 64 512). 65 tags: a full wavefront, whose lane 63 reaches the end of the block, and a ragged one
    "A43 fixed f64 T65": dict(A=43, storage=F64, tags=65),
    "A43 fixed mixed T65": dict(A=43, storage=MIXED, tags=65),
    "A31 ml f64 T65": dict(A=31, storage=F64, fixed=False, tags=65),
    "A31 ml mixed T65": dict(A=31, storage=MIXED, fixed=False, tags=65),
}


@functools.lru_cache(maxsize=None)
def _inputs(name, slots=SLOTS):
    """the inputs of a configuration; read-only"""
    return Inputs(slots=slots, **CONFIGS[name])


@pytest.mark.parametrize("name", list(CONFIGS))
def test_one_call_equals_the_single_calls_bit_for_bit(name):
    if not has_gpu():
        pytest.skip("no GPU")
    inp = _inputs(name)
    ref = rc.check_one_call(FAM, inp, name, chunks=(1, None, 7))
    words = ref[1]
    assert ((words == ST_SKIPPED) == ~inp.mask).all()            # the reference run itself skips where the mask says
    low = words[inp.mask] & 0xFF
    assert (low == 0).any() and (low != 0).any()                 # plain slots, and the dropout paths ran
    if not inp.fixed:
        assert (low & ST_ML_INIT).any()                          # ML initialisations happened


def test_a_schedule_that_crosses_the_launch_boundary():
    """130 slots at the default launch size: 128 in the first launch, 2 in the second"""
    if not has_gpu():
        pytest.skip("no GPU")
    inp = _inputs("A8 fixed mixed", 130)
    assert inp.d_dt.shape[0] == 130
    out = []
    for run in (rc.single_calls, rc.one_call):
        b = inp.bank()
        out.append(run(FAM, b, inp))
        b.close()
    rc.same_bytes(out[1], out[0], NAMES, "130 slots")


def test_a_bank_with_more_wavefronts_than_simds():
    """65 600 tags: the single calls run the two-wavefront build, the one call k_trace_toa6_each"""
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    n, A, S = 65600, 8, 3
    w = Workload(n, A)
    mask = np.random.default_rng(3).random((S, n)) < 0.5
    mask[1, 64 * 500:64 * 520] = False                          # whole wavefronts pass a slot here as well
    assert 0.45 < mask.mean() < 0.55
    dt = np.where(mask, np.array([0.1, 0.05, 0.07])[:, None], -1.0)
    ranges = np.stack([w.ranges_mm(s) for s in range(S)])
    ranges[~mask] = ABSENT_MM
    inp = types.SimpleNamespace(T=n, A=A, kinds=np.zeros(S, dtype=np.uint8), d_r=rc.up(ranges.transpose(0, 2, 1)),
                                d_e=rc.up(w.err_est(np.float32).T), d_dt=rc.up(dt))
    out = []
    for run in (rc.single_calls, rc.one_call):
        b = capi.KfposBank(capi.MODEL_TOA, n, w.anchors, storage=MIXED, init_pos=w.init_positions())
        out.append(run(FAM, b, inp))
        b.close()
    assert ((out[0][1] == ST_SKIPPED) == ~mask).all()
    rc.same_bytes(out[1], out[0], NAMES, "65 600 tags")


@pytest.mark.parametrize("name", ["A8 fixed p48", "A8 fixed f32", "A8 ml p48", "A5 ml mixed", "A8 fixed mixed coop"])
def test_a_tag_that_runs_nothing_keeps_every_stored_byte(name):
    """on a bank that has been stepped before the call (every tag, tag 5 included) and on a fresh one"""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    inp = _inputs(name)
    assert not inp.mask[:, 5].any()
    for chunk in (None, 7):
        b = inp.bank(chunk)
        before = b.get_tags([5])
        assert before[2][0] == 0                                 # fresh: not started
        rc.one_call(FAM, b, inp)
        after = b.get_tags([5])
        for x, y, what in zip(before[:3], after[:3], ("x", "P", "flags")):
            assert x.tobytes() == y.tobytes(), (what, chunk)
        assert after[2][0] & FL_STARTED == 0
        assert (b.get_state()[2][np.arange(T) != 5] & FL_STARTED).all()   # everyone else ran something
        b.close()
        # stepped before: two full epochs for every tag, then the call
        b = inp.bank(chunk)
        for s in (0, 1):
            every = torch.from_numpy(Case("each", 0, inp.A, T=T).epoch(Workload(T, inp.A), s).T.copy()).to(inp.d_r.device)
            b.step_toa_dev(every, inp.d_e, 0.1, stream=torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        before = b.get_tags([5])
        assert before[2][0] & FL_STARTED and np.isfinite(before[0]).all() and before[1].any()
        rc.one_call(FAM, b, inp)
        after = b.get_tags([5])
        for x, y, what in zip(before[:3], after[:3], ("x", "P", "flags")):
            assert x.tobytes() == y.tobytes(), (what, chunk, "stepped before")
        b.close()


ORACLE = {
    "A8 fixed": dict(A=8, storage=F64, env=NO_COOP),
    "A8 ml": dict(A=8, storage=F64, fixed=False),
    "A5 fixed": dict(A=5, storage=F64, env=NO_COOP),
    "A5 ml": dict(A=5, storage=F64, fixed=False),
    "A8 fixed ignore_worst": dict(A=8, storage=F64, ignore_worst=True),
    "A16 fixed top3": dict(A=16, storage=F64, top_n=3),
    "A43 fixed T65": dict(A=43, storage=F64, tags=65),
    "A31 ml T65": dict(A=31, storage=F64, fixed=False, tags=65),
}


@pytest.mark.parametrize("name", list(ORACLE))
def test_f64_storage_matches_the_oracle_after_every_slot_a_tag_ran(name):
    """position RMS <= 1e-9 m (the bound of test_run_events_each_gpu.py for this comparison) over the tags that ran the
    slot, every status word equal to the oracle's, absent tags' rows equal to the previous slot's. Measured on an MI355X,
    worst slot of the 37: 1.5e-15 m RMS (8.9e-15 m max) from a fixed start -- leave-one-out and top-N included --, 3.7e-15 m
    RMS (1.3e-14 m max) from an ML start."""
    if not has_gpu():
        pytest.skip("no GPU")
    import oracle_py
    inp = Inputs(**ORACLE[name])
    T = inp.T
    b = inp.bank()
    got = rc.one_call(FAM, b, inp)
    b.close()
    o = oracle_py.OracleBank(0, T, inp.anchors, ignore_worst=inp.ignore_worst, top_n=inp.top_n,
                             init_pos=inp.init if inp.fixed else None, n_threads=8)
    worst = [0.0, 0.0]
    for e in range(inp.slots):
        so = o.step_toa(inp.ranges[e], inp.err, inp.dt[e])
        ran = inp.mask[e]
        po = o.get_state()[0][:, :3]
        pg = got[0][e].T
        assert pg.shape == po.shape == (T, 3)
        rms, mx, same_nan = rms_and_max(pg[ran], po[ran])
        print(f"slot {e}: {int(ran.sum())} tags, RMS {rms:.3e} m, max {mx:.3e} m")
        worst = [max(worst[0], rms), max(worst[1], mx)]
        assert same_nan, e
        assert rms <= 1e-9, (e, rms, mx)
        assert np.array_equal(so, got[1][e].astype(np.uint32)), (e, "status words")
        if e:   # a tag that sat the slot out reports its untouched position
            assert got[0][e].T[~ran].tobytes() == got[0][e - 1].T[~ran].tobytes(), e
    print(f"{name}: worst RMS {worst[0]:.3e} m, worst max {worst[1]:.3e} m against the oracle over {inp.slots} slots")
    started = np.isfinite(got[0][-1]).all(axis=0)
    assert started[np.arange(T) != 5].all()    # every tag but the absent one has started by the end
    if not inp.fixed:
        assert np.isnan(got[0][:, :, 5]).all()  # a tag waiting for its ML initialisation reports NaN


def _raw_call(b, n, d_dt, r, e, A, nt):
    p = lambda x: None if x is None else x.data_ptr()  # noqa: E731
    return b.lib.kfpos_run_trace_each_dev(b._h, n, p(d_dt), p(r), A * nt, p(e), 0, None, None, None, None)


def _snapshot(b):
    parts = list(b.get_state())
    if b.lib.kfpos_latch_dim(b._h):
        parts.append(b.get_latch())
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_argument_errors_are_decided_before_anything_runs():
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    A = 8
    inp = Inputs(A, MIXED, env=NO_COOP)
    b = inp.bank()
    rc.one_call(FAM, b, inp)                 # a bank with something in it
    before = _snapshot(b)
    d, r, e = inp.d_dt, inp.d_r, inp.d_e
    refused = {"n_steps < 0": (-1, d, r, e), "dt_steps_dev missing": (9, None, r, e),
               "range_mm missing": (9, d, None, e), "err_est missing": (9, d, r, None)}
    for what, args in refused.items():
        assert _raw_call(b, *args, A, T) == ERR_ARG, what
        assert _snapshot(b) == before, what
    assert b.lib.kfpos_run_trace_each_dev(None, 0, None, None, 0, None, 0, None, None, None, None) == ERR_ARG
    assert _raw_call(b, 0, None, None, None, A, T) == 0     # n_steps == 0 comes ahead of the NULL arrays
    assert _raw_call(b, 0, d, r, e, A, T) == 0
    assert _snapshot(b) == before, "n_steps == 0"
    assert _raw_call(b, 3, d, r, e, A, T) == 0
    assert _snapshot(b) != before
    b.close()

    # handles of the other models: refused, NULL arrays first (the order of kfpos_run_events_each_dev)
    planar = dict(use_fixed_height=1, fixed_height=1.0)
    for model, kw in ((capi.MODEL_TOA_IMU, {}), (capi.MODEL_ML, {}), (capi.MODEL_PLANAR, {"planar": planar})):
        o = capi.KfposBank(model, T, inp.anchors, storage=MIXED, init_pos=inp.init, **kw)
        o.step_toa_dev(r[0], e, 0.1)
        before = _snapshot(o)
        assert _raw_call(o, 9, d, r, e, A, T) == ERR_MODEL, model
        assert _raw_call(o, 9, None, r, e, A, T) == ERR_ARG, model
        assert _raw_call(o, 0, None, None, None, A, T) == 0, model
        assert _snapshot(o) == before, model
        o.close()

    # a 6-state handle whose anchors are not set
    lib = capi.load()
    cfg = capi._Config()
    cfg.model, cfg.n_tags, cfg.max_anchors, cfg.storage = capi.MODEL_TOA, T, A, MIXED
    cfg.accel_noise, cfg.jolt, cfg.cost_threshold, cfg.use_init_pos = 0.5, 0.5, 0.5, 1
    cfg.init_pos = (ctypes.c_double * 3)(5.0, 5.0, 1.0)
    h = ctypes.c_void_p()
    assert lib.kfpos_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    bare = capi.KfposBank.__new__(capi.KfposBank)
    bare.lib, bare._h, bare.T, bare.A, bare.model, bare.storage = lib, h, T, A, capi.MODEL_TOA, MIXED
    bare.n = lib.kfpos_state_dim(h)
    assert lib.kfpos_init(h) == 0
    before = _snapshot(bare)
    assert _raw_call(bare, 9, d, r, e, A, T) == ERR_STATE
    assert _raw_call(bare, 9, d, None, e, A, T) == ERR_ARG
    assert _snapshot(bare) == before
    bare.close()
