"""kfpos_run_events_each_dev: an event schedule in which every tag has a timeline of its own, in one launch, computes bit
for bit what the same slots give as single kfpos_step_imu_dev / kfpos_step_toa_dev calls with a per-tag dt array --
state, covariance as stored, flags, latch, the status word and the position of every slot -- and stays with the oracle
after every slot.

One schedule serves every test: the kinds pattern RUNS + TAIL below (39 slots) and an explicit participation mask over
130 tags whose properties the first test asserts."""
import ctypes

import numpy as np
import pytest

import replay_checks as rc
from cases import Case, rms_and_max
from conftest import has_gpu
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

IMU, TOA = 0, 1
RUNS = (0, 4, 1, 4, 4, 0, 1, 4, 0, 1, 4, 1)   # IMU slots ahead of each ranging slot
TAIL = 3                                      # IMU slots behind the last ranging slot
T = 130                                       # two full wavefronts and one of two lanes
DT_ZERO = 10                                  # a slot in which every participant has dt = 0 (inside an IMU run)
WAVE_OUT = (9, 17)                            # an IMU and a TOA slot nobody of tags 64..127 takes part in
LATE, LATE_FIRST = 7, 5                       # tag 7 first takes part in slot 5, a TOA slot behind four IMU slots
ABSENT_MM = 1999999999                        # what the ranges of an absent (tag, slot) pair hold
ST_SKIPPED, ST_ML_INIT = 64, 8
FL_STARTED, FL_HAS_IMU = 1, 2
ERR_ARG, ERR_MODEL, ERR_STATE = 1, 4, 5


def _kinds():
    kinds = []
    for k in RUNS:
        kinds += [IMU] * k + [TOA]
    return np.array(kinds + [IMU] * TAIL, dtype=np.uint8)


def _mask():
    """who takes part in which slot: (E, T) bool"""
    E = _kinds().size
    m = np.random.default_rng(20261018).random((E, T)) < 0.65
    m[:, 0] = True
    m[:, 5] = False
    for e in WAVE_OUT:
        m[e, 64:128] = False
    m[-1, 128] = False
    m[:LATE_FIRST, LATE] = False
    m[LATE_FIRST, LATE] = True
    return m


def test_the_schedule_holds_what_it_is_meant_to_hold():
    k, m = _kinds(), _mask()
    E = k.size
    assert 36 <= E <= 40 and m.shape == (E, T) and T == 2 * 64 + 2
    assert {0, 1, 4} <= set(RUNS) and any(k[e] == TOA and k[e + 1] == TOA for e in range(E - 1))
    assert m[:, 0].all() and not m[:, 5].any()
    assert k[WAVE_OUT[0]] == IMU and k[WAVE_OUT[1]] == TOA and not m[list(WAVE_OUT), 64:128].any()
    assert m[list(WAVE_OUT), :64].any(axis=1).all()             # while the first wavefront runs those slots
    assert not m[-1, 128] and m[:-1, 128].any()
    first = int(np.flatnonzero(m[:, LATE])[0])
    assert first == LATE_FIRST and k[first] == TOA and (k[:first] == IMU).sum() >= 1
    assert 0.40 <= m.mean() <= 0.80
    every = m.all(axis=0).sum(), (~m).all(axis=0).sum()
    assert every == (1, 1)                                      # only tag 0 is everywhere, only tag 5 nowhere
    # launches of 7 slots: a boundary inside a run of IMU slots, another directly before a ranging slot
    starts = list(range(7, E, 7))
    assert any(k[s - 1] == IMU and k[s] == IMU for s in starts), "no boundary inside an IMU run"
    assert any(k[s] == TOA for s in starts), "no boundary directly before a ranging slot"
    assert k[DT_ZERO] == IMU and m[DT_ZERO].sum() > 1
    # the dropout rows of cases.Case.epoch fall among the ranging slots
    eps = range(len(RUNS))
    assert any(s % 7 == 3 for s in eps) and any(s % 11 == 5 for s in eps) and any(s % 23 == 9 for s in eps)
    # the single-tag schedule: tag 0 of a mask cut to one column would never skip, so that test takes column 1
    assert 0 < m[:, 1].sum() < E


class Inputs:
    """the schedule's inputs in HBM (component-major), and on the host in the (T, ...) form the oracle takes"""

    def __init__(self, A, storage, fixed, cov_full, tags=None, fill=True, dev="cuda:0"):
        """fill: the input entries of absent (tag, slot) pairs hold NaN (accel) / ABSENT_MM (ranges)"""
        from roskfpos_amd import capi
        tags = np.arange(T) if tags is None else np.asarray(tags)
        n = self.T = tags.size
        self.A, self.storage, self.fixed = A, storage, fixed
        real = self.real = np.float64 if storage == capi.STORE_F64 else np.float32
        case = Case("each", 1, A, fixed=fixed, T=T, cov_full=cov_full)
        w = Workload(T, A)
        self.anchors, self.init = w.anchors, w.init_positions()[tags]
        self.kinds = _kinds()
        self.mask = _mask()[:, tags]
        base = np.round(np.random.default_rng(20261017).uniform(0.004, 0.03, self.kinds.size), 4)
        base[DT_ZERO] = 0.0
        self.base = base
        self.dt = np.where(self.mask, base[:, None], -1.0)                                # (E, T)
        toa, imu = np.flatnonzero(self.kinds == TOA), np.flatnonzero(self.kinds == IMU)
        self.ranges = np.stack([case.epoch(w, s) for s in range(len(RUNS))])[:, tags]     # (J, T, A), dropout rows kept
        if fill:
            self.ranges[~self.mask[toa]] = ABSENT_MM
        acc = [w.accel_between(s, i, k, real) for s, k in enumerate(RUNS) for i in range(k)]
        acc += [w.accel_between(len(RUNS), i, TAIL, real) for i in range(TAIL)]
        self.accel = np.stack(acc)[:, tags]                                               # (I, T, 3)
        if fill:
            self.accel[~self.mask[imu]] = np.nan
        self.accel_full = w.accel(0, real)[tags]                                          # an earlier sample for every tag
        self.err = w.err_est(real)[tags]
        self.cov = case.accel_cov(w).astype(real)[tags]
        self.cov_other = Case("other", 1, A, T=T, cov_full=not cov_full).accel_cov(w).astype(real)[tags]
        up = lambda a: rc.up(a, dev)  # noqa: E731
        self.d_r, self.d_e = up(self.ranges.transpose(0, 2, 1)), up(self.err.T)
        self.d_a, self.d_c, self.d_c_other = up(self.accel.transpose(0, 2, 1)), up(self.cov.T), up(self.cov_other.T)
        self.d_a_full, self.d_dt = up(self.accel_full.T), up(self.dt)
        assert n == self.d_dt.shape[1]

    def bank(self, chunk=None):
        from roskfpos_amd import capi
        with rc.env(KFPOS_TRACE_CHUNK_STEPS=chunk):
            return capi.KfposBank(capi.MODEL_TOA_IMU, self.T, self.anchors, storage=self.storage,
                                  init_pos=self.init if self.fixed else None)


def _final(b):
    x, P, fl = b.get_state()
    return x, P, fl, b.get_latch()


def _single(b, inp, e, kind, i, status, stream, dt):
    if kind == TOA:
        b.step_toa_dev(inp.d_r[i], inp.d_e, 0.0, status=status, stream=stream, dt_dev=dt)
    else:
        b.step_imu_dev(inp.d_a[i], inp.d_c, 0.0, status=status, stream=stream, dt_dev=dt)


def _call(method):
    def call(b, inp, n, dts, traj, ste, st, stream):
        nt, A = inp.T, inp.A
        getattr(b, method)(inp.kinds[:n], dts, range_mm=inp.d_r, stride_ranges=A * nt, err_est=inp.d_e, stride_err=0,
                           accel=inp.d_a, stride_accel=3 * nt, cov=inp.d_c, trajectory=traj, status_events=ste,
                           status=st, stream=stream)
    return call


NAMES = ("position after every slot", "status of every slot", "x", "P", "flags", "latch")
EACH = rc.Family(names=NAMES, n_kinds=2, dts=lambda inp: inp.d_dt, final=_final,
                 position=lambda b: b.get_state()[0][:, :3].T, single=_single, call=_call("run_events_each_dev"))
# the shared-timeline entry point over the same inputs; its dts: one scalar per slot
SHARED = rc.Family(**{**vars(EACH), "call": _call("run_events_dev")})


def _bit_identity(A, storage, combos, tags=None):
    for fixed, cov_full in combos:
        inp = Inputs(A, storage, fixed, cov_full, tags)
        ref = rc.check_one_call(EACH, inp, f"fixed={fixed} cov_full={cov_full}")
        words = ref[1]
        assert ((words == ST_SKIPPED) == ~inp.mask).all()        # the reference run itself skips where the mask says
        low = words[inp.mask] & 0xFF
        if inp.T > 1:
            assert (low == 0).mean() > 0.5 and (low != 0).any()  # most events are plain, the dropout paths ran
            if not fixed:
                assert (words[inp.mask] & ST_ML_INIT).any()      # ML initialisations happened


EVERY = [(f, c) for f in (True, False) for c in (False, True)]


@pytest.mark.parametrize("A", [8, 5])               # epoch in registers; run-time anchor loop
@pytest.mark.parametrize("storage", [0, 1, 2, 3])   # f64, f32, mixed, p48
def test_one_call_equals_the_single_calls_bit_for_bit(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(A, storage, EVERY)


@pytest.mark.parametrize("storage,A", [(2, 8), (3, 5)])
def test_one_call_equals_the_single_calls_for_a_single_tag(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(A, storage, [(True, False), (False, True)], tags=[1])   # tag 1 skips slots (asserted above)


OVER_64K = [(True, False), (False, True)]            # (fixed, cov_full)


@pytest.mark.parametrize("storage", [0, 2])         # f64; mixed: 4-byte measurements
def test_one_call_equals_the_single_calls_behind_a_raised_lds_limit(storage):
    """17 anchors: the run-time loop's epoch and CovPark9 take 66 240 bytes of LDS, the smallest count over 64 KB (16:
    64 704), so k_events_imu9_each runs behind a raised hipFuncAttributeMaxDynamicSharedMemorySize. Tags 0..64: a full
    wavefront, whose lane 63 reaches the end of the block, and a ragged one"""
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(17, storage, OVER_64K, tags=np.arange(65))


def test_a_schedule_that_crosses_the_launch_boundary():
    """the schedule four times over, 156 slots: a launch of 128 slots -- both words of its `kinds` in use, slots of
    either kind at 64 or later in it -- and a second one for the rest"""
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    reps = 4
    inp = Inputs(8, capi.STORE_MIXED, True, False)                  # the register-resident kernel
    inp.kinds, inp.mask = np.tile(inp.kinds, reps), np.tile(inp.mask, (reps, 1))
    inp.d_r, inp.d_a, inp.d_dt = inp.d_r.repeat(reps, 1, 1), inp.d_a.repeat(reps, 1, 1), inp.d_dt.repeat(reps, 1)
    assert inp.kinds.size >= 130 and inp.kinds.size > 128
    assert set(inp.kinds[64:128].tolist()) == {IMU, TOA}
    b = inp.bank()
    ref = rc.single_calls(EACH, b, inp)
    b.close()
    assert ((ref[1] == ST_SKIPPED) == ~inp.mask).all()
    low = ref[1][inp.mask] & 0xFF
    assert (low == 0).mean() > 0.5 and (low != 0).any() and np.isfinite(ref[0][-1]).all()
    b = inp.bank()
    got = rc.one_call(EACH, b, inp)
    b.close()
    rc.same_bytes(got, ref, NAMES, "four times the schedule")


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 5), (2, 8), (3, 5), (2, 5)])
def test_slots_ahead_of_a_tags_first_sample_fuse_its_earlier_latch_with_its_own_covariance(storage, A):
    """On a bank that has run the schedule once (from a fixed start with P = 0 the sample's covariance leaves no trace in
    the first events), three populations meet in every launch: odd tags latch a sample with ANOTHER covariance than the
    call's; tags 2, 6, 10, ... sat every IMU slot of that first run out and have nothing latched; tags 0, 4, 8, ... carry
    the call's own covariance."""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    for cov_full in (False, True):
        inp = Inputs(A, storage, True, cov_full)
        tags = np.arange(T)
        early = torch.from_numpy(np.where(tags % 2 == 1, 0.02, -1.0)).to(inp.d_r.device)
        pre = inp.dt.copy()
        pre[np.ix_(inp.kinds == IMU, tags % 4 == 2)] = -1.0           # the first run without a sample for these tags
        d_pre = torch.from_numpy(pre).to(inp.d_r.device)
        nothing = (tags % 4 == 2)
        first = np.array([inp.kinds[np.flatnonzero(inp.mask[:, t])[0]] for t in tags[nothing]])
        assert (first == TOA).any() and (first == IMU).any()          # ranging slots ahead of the first sample, or not

        def bank(chunk=None, cov=None):
            b = inp.bank(chunk)
            rc.single_calls(EACH, b, inp, dts=d_pre)
            b.step_imu_dev(inp.d_a_full, inp.d_c_other if cov is None else cov, 0.0, dt_dev=early,
                           stream=torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            return b

        b = bank()
        latched = b.get_latch()[:, 3:]
        other = (latched == inp.cov_other.astype(np.float64)).all(axis=1)
        assert other.tolist() == (tags % 2 == 1).tolist()             # who carries which covariance into the call
        assert (latched[tags % 4 == 0] == inp.cov.astype(np.float64)[0]).all()
        has = (b.get_state()[2] & FL_HAS_IMU) != 0
        assert has.tolist() == (~nothing).tolist() and (b.get_state()[2][nothing] & FL_STARTED).all()
        ref = rc.single_calls(EACH, b, inp)
        b.close()
        for chunk in (None, 3):
            b = bank(chunk)
            got = rc.one_call(EACH, b, inp)
            b.close()
            rc.same_bytes(got, ref, NAMES, f"cov_full={cov_full} chunk={chunk}")
        # the comparison has teeth: tag 7 (odd) runs a TOA slot ahead of its own first sample; had that slot fused the
        # latched sample with the CALL's covariance, its covariance would have come out of that slot differently (the
        # acceleration block, which the tag's next own sample overwrites: hence the comparison right behind the slot)
        behind = []
        for cov in (None, inp.d_c):
            b = bank(cov=cov)
            behind.append(rc.single_calls(EACH, b, inp, n_slots=LATE_FIRST + 1))
            b.close()
        assert LATE % 2 == 1 and behind[0][3].tobytes() != behind[1][3].tobytes()
        if storage != 1:   # (a difference of 1.4e-7 of the entry: below what 24 mantissa bits keep)
            assert behind[0][3][LATE].tobytes() != behind[1][3][LATE].tobytes()
        # ... and the call that ends right behind that slot leaves exactly the bytes of the single calls
        for chunk in (None, 3):
            b = bank(chunk)
            got = rc.one_call(EACH, b, inp, n_slots=LATE_FIRST + 1)
            b.close()
            rc.same_bytes(got, behind[0], NAMES, f"cov_full={cov_full} chunk={chunk}, {LATE_FIRST + 1} slots")


@pytest.mark.parametrize("storage,A", [(2, 8), (0, 5)])
def test_a_nan_dt_runs_the_event_as_the_single_call_does(storage, A):
    """the predicate is dt < 0.0: a NaN dt takes part. Tags 3 and 70 get one in an IMU slot, tags 9 and 129 in a ranging
    slot; what comes out is what the single calls leave -- status words and flags equal, every number equal or NaN in the
    same places (which NaN an operation hands on is the one thing two builds of the same arithmetic may differ in)."""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    inp = Inputs(A, storage, True, False, fill=False)
    e_imu, e_toa = 14, 18
    assert inp.kinds[e_imu] == IMU and inp.kinds[e_toa] == TOA
    dt = inp.dt.copy()
    dt[e_imu, [3, 70]] = np.nan
    dt[e_toa, [9, 129]] = np.nan
    d_dt = torch.from_numpy(dt).to(inp.d_r.device)
    b = inp.bank()
    ref = rc.single_calls(EACH, b, inp, dts=d_dt)
    b.close()
    assert not (ref[1][e_imu, [3, 70]] == ST_SKIPPED).any() and not (ref[1][e_toa, [9, 129]] == ST_SKIPPED).any()
    assert (ref[1][e_imu, [3, 70]] & 32).all() and (ref[1][e_toa, [9, 129]] & 32).all()   # ... and KFPOS_ST_NONFINITE
    for chunk in (None, 7):
        b = inp.bank(chunk)
        got = rc.one_call(EACH, b, inp, dts=d_dt)
        b.close()
        for g, r, name in zip(got, ref, NAMES):
            assert g.shape == r.shape and g.dtype == r.dtype, name
            assert np.array_equal(g, r, equal_nan=g.dtype.kind == "f"), (name, chunk)
        clean = np.setdiff1d(np.arange(T), [3, 70, 9, 129])
        assert got[3][clean].tobytes() == ref[3][clean].tobytes()


@pytest.mark.parametrize("storage,A,fixed", [(3, 8, True), (1, 5, False), (3, 5, False), (1, 8, True)])
def test_a_tag_that_runs_nothing_keeps_every_stored_byte(storage, A, fixed):
    if not has_gpu():
        pytest.skip("no GPU")
    inp = Inputs(A, storage, fixed, True)
    assert not inp.mask[:, 5].any()
    rng = np.random.default_rng(5)
    m = rng.normal(size=(9, 9))
    P5 = (m @ m.T * 1.234567890123e-2)[None]          # not representable in 24 or 39 mantissa bits
    latch5 = rng.normal(size=(1, 12)) * 0.123456789
    for chunk in (None, 7):
        b = inp.bank(chunk)
        b.set_tags([5], P=P5, latch=latch5)           # no flags: the tag stays as fresh as the handle made it
        before = b.get_tags([5])
        assert before[2][0] == 0 and not np.array_equal(before[1], P5)   # not started, nothing latched; P was rounded
        rc.one_call(EACH, b, inp)
        after = b.get_tags([5])
        for x, y, name in zip(before[:4], after[:4], ("x", "P", "flags", "latch")):
            assert x.tobytes() == y.tobytes(), (name, chunk)
        assert after[2][0] & FL_STARTED == 0
        others = b.get_state()[2]
        assert (others[np.arange(T) != 5] & FL_STARTED).all()            # everyone else ran something
        assert ((others & FL_HAS_IMU) != 0).tolist() == inp.mask[inp.kinds == IMU].any(axis=0).tolist()
        b.close()


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 8), (2, 8), (3, 8), (2, 5), (3, 5)])
def test_an_all_synchronous_schedule_equals_run_events_dev(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    for fixed, cov_full in ((True, False), (False, True)):
        inp = Inputs(A, storage, fixed, cov_full, fill=False)   # every tag takes part: every input entry is read
        base = inp.base                                          # every tag at the slot's shared dt
        d_dt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(base[:, None], inp.dt.shape))).to(inp.d_r.device)
        out = []
        for chunk in (None, 7):
            b = inp.bank(chunk)
            ref = rc.one_call(SHARED, b, inp, dts=base)
            b.close()
            b = inp.bank(chunk)
            got = rc.one_call(EACH, b, inp, dts=d_dt)
            b.close()
            rc.same_bytes(got, ref, NAMES, f"fixed={fixed} cov_full={cov_full} chunk={chunk}")
            out.append(ref)
        assert not (out[0][1] == ST_SKIPPED).any()


@pytest.mark.parametrize("A", [8, 5])
@pytest.mark.parametrize("fixed", [True, False])
@pytest.mark.parametrize("cov_full", [False, True])
def test_f64_storage_matches_the_oracle_after_every_event_a_tag_ran(cov_full, fixed, A, T=T):
    """position RMS <= 1e-9 m (the bound of test_run_events_gpu.py for this comparison) over the tags that ran the slot,
    every status word equal to the oracle's. Measured on an MI355X: worst RMS 2.4e-16 m from a fixed start, 3.9e-15 m (max
    1.2e-14 m) from an ML start."""
    if not has_gpu():
        pytest.skip("no GPU")
    import oracle_py
    inp = Inputs(A, 0, fixed, cov_full, tags=np.arange(T))
    b = inp.bank()
    got = rc.one_call(EACH, b, inp)
    b.close()
    o = oracle_py.OracleBank(1, T, inp.anchors, init_pos=inp.init if fixed else None, n_threads=8)
    j = i = 0
    worst = [0.0, 0.0]
    for e, kind in enumerate(inp.kinds):
        if kind == TOA:
            so = o.step_toa(inp.ranges[j], inp.err, inp.dt[e])
            j += 1
        else:
            so = o.step_imu(np.nan_to_num(inp.accel[i], nan=0.0), inp.cov, inp.dt[e])   # never read: zeros for tidiness
            i += 1
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
        # a tag that sat the slot out reports its untouched position
        if e:
            assert got[0][e].T[~ran].tobytes() == got[0][e - 1].T[~ran].tobytes(), e
    print(f"A={A} fixed={fixed} cov_full={cov_full}: worst RMS {worst[0]:.3e} m, worst max {worst[1]:.3e} m "
          f"against the oracle over {inp.kinds.size} slots")
    started = np.isfinite(got[0][-1]).all(axis=0)
    assert started[np.arange(T) != 5].all()    # every tag but the absent one has started by the end


@pytest.mark.parametrize("cov_full", [False, True])
def test_f64_storage_matches_the_oracle_behind_a_raised_lds_limit(cov_full):
    """the same bound at 17 anchors and tags 0..64 (more than 64 KB of LDS), from a fixed start: an ML start stays with the
    bit-identity test above. Beyond a dozen anchors the Gauss-Newton walk of a few tags' ML initialisation is chaotic
    (cases.py, "No 16-anchor ML-init case"): on the CPU alone the host emulation of the kernel arithmetic and the oracle
    then part by 1e-7 ... 3e-2 m on 2 to 4 of 130 tags and count different gain iterations. Measured with the library
    before launch selection moved into kfpos_launch_plan.h, ML start, full covariance: the status words of slot 25 differ from the oracle's."""
    test_f64_storage_matches_the_oracle_after_every_event_a_tag_ran(cov_full, True, 17, T=65)


def _raw_call(b, n, kinds, d_dt, r, e, a, c, A, nt):
    p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())  # noqa: E731
    return b.lib.kfpos_run_events_each_dev(b._h, n, p(kinds), p(d_dt), p(r), A * nt, p(e), 0, p(a), 3 * nt, p(c),
                                           None, None, None, None)


def _snapshot(b):
    x, P, fl = b.get_state()
    parts = [x, P, fl]
    if b.model == 1:
        parts.append(b.get_latch())
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_argument_errors_are_decided_before_anything_runs():
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    A = 8
    inp = Inputs(A, capi.STORE_MIXED, True, False, fill=False)
    b = inp.bank()
    rc.one_call(EACH, b, inp)                                        # a bank with something in it
    before = _snapshot(b)
    k, d = inp.kinds[:9].copy(), inp.d_dt
    only_imu, only_toa = np.zeros(3, dtype=np.uint8), np.ones(3, dtype=np.uint8)
    bad = k.copy()
    bad[4] = 2
    r, e, a, c = inp.d_r, inp.d_e, inp.d_a, inp.d_c
    refused = {
        "n_events < 0": (-1, k, d, r, e, a, c),
        "a kind other than 0 or 1": (9, bad, d, r, e, a, c),
        "kinds missing": (9, None, d, r, e, a, c),
        "dt_events_dev missing": (9, k, None, r, e, a, c),
        "range_mm missing, TOA slots": (9, k, d, None, e, a, c),
        "err_est missing, TOA slots": (3, only_toa, d, r, None, a, c),
        "accel missing, IMU slots": (9, k, d, r, e, None, c),
        "cov missing, IMU slots": (3, only_imu, d, r, e, a, None),
    }
    for what, args in refused.items():
        assert _raw_call(b, *args, A, T) == ERR_ARG, what
        assert _snapshot(b) == before, what
    assert _raw_call(b, 9, bad, d, r, e, a, c, A, T) == ERR_ARG
    assert b"kinds[4]" in b.lib.kfpos_last_error()           # the message names the event
    # arrays of a kind that does not occur may be missing; n_events == 0 touches nothing
    assert _raw_call(b, 0, None, None, None, None, None, None, A, T) == 0
    assert _raw_call(b, 0, k, d, r, e, a, c, A, T) == 0
    assert _snapshot(b) == before, "n_events == 0"
    assert _raw_call(b, 3, only_toa, d, r, e, None, None, A, T) == 0
    assert _raw_call(b, 3, only_imu, d, None, None, a, c, A, T) == 0
    assert _snapshot(b) != before
    b.close()

    # another model
    b6 = capi.KfposBank(capi.MODEL_TOA, T, inp.anchors, storage=capi.STORE_MIXED, init_pos=inp.init)
    b6.step_toa_dev(r[0], e, 0.1)
    before = _snapshot(b6)
    assert _raw_call(b6, 9, k, d, r, e, a, c, A, T) == ERR_MODEL
    assert _raw_call(b6, 3, only_toa, d, r, e, None, None, A, T) == ERR_MODEL
    assert _snapshot(b6) == before
    b6.close()

    # a 9-state handle whose anchors are not set: ranging slots are refused, IMU slots run
    lib = capi.load()
    cfg = capi._Config()
    cfg.model, cfg.n_tags, cfg.max_anchors, cfg.storage = capi.MODEL_TOA_IMU, T, A, capi.STORE_MIXED
    cfg.accel_noise, cfg.jolt, cfg.cost_threshold, cfg.use_init_pos = 0.5, 0.5, 0.5, 1
    cfg.init_pos = (ctypes.c_double * 3)(5.0, 5.0, 1.0)
    h = ctypes.c_void_p()
    assert lib.kfpos_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    bare = capi.KfposBank.__new__(capi.KfposBank)
    bare.lib, bare._h, bare.T, bare.A, bare.model, bare.storage = lib, h, T, A, capi.MODEL_TOA_IMU, capi.STORE_MIXED
    bare.n = lib.kfpos_state_dim(h)
    assert lib.kfpos_init(h) == 0
    before = _snapshot(bare)
    assert _raw_call(bare, 9, k, d, r, e, a, c, A, T) == ERR_STATE
    assert _snapshot(bare) == before
    assert _raw_call(bare, 3, only_imu, d, None, None, a, c, A, T) == 0
    assert _snapshot(bare) != before
    bare.close()
