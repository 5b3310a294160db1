"""kfpos_run_planar_events_each_dev: a multi-sensor event schedule of the 8-state planar filter in which every tag has a
timeline of its own, in one call, computes bit for bit what the same slots give as single kfpos_step_toa_dev /
kfpos_step_sensor_dev calls with the slot's per-tag dt array -- state, height, covariance as stored, flags, all 15 latch
rows, the status word and the position of every slot -- and stays with the oracle after every slot.

One schedule serves every test (tests/planar_events_each.py; tests/test_planar_events_each_schedule.py asserts on the
CPU that it holds what it is meant to hold): the kinds of tests/planar_events.py and an explicit participation mask over
130 tags. Absent (tag, slot) pairs and dropped PX4Flow samples carry NaN / a sentinel range in the inputs."""
import ctypes

import numpy as np
import pytest

import planar_events as pe
import planar_events_each as pee
import replay_checks as rc
from conftest import has_gpu

pytestmark = pytest.mark.gpu

T = pee.T
ERR_ARG, ERR_MODEL, ERR_STATE = 1, 4, 5
FL_STARTED = 1
HAS_PX4, HAS_IMU, HAS_MAG = 1 << 5, 1 << 6, 1 << 7      # planar flags word: what a tag has latched
ST_SKIPPED = pee.ST_SKIPPED
SENTINEL = -12345.6789


class Inputs:
    """a schedule's inputs in HBM, component-major; tags: the columns of the 130-tag schedule the bank holds"""

    def __init__(self, A, storage, start, end_on_sensor=True, waiting=False, kinds=None, tags=None, fill=True,
                 dev="cuda:0"):
        from roskfpos_amd import capi
        tags = np.arange(T) if tags is None else np.asarray(tags)
        self.T, self.A, self.storage, self.start = tags.size, A, storage, start
        real = np.float64 if storage == capi.STORE_F64 else np.float32
        es = self.es = pee.EachSchedule(A, end_on_sensor, waiting, real, kinds, fill)
        self.kinds, self.base = es.kinds, es.base
        self.mask, self.ran, self.dt = es.mask[:, tags], es.ran[:, tags], es.dt[:, tags]
        init = pe.init_of(es.sch, start)
        self.init = None if init is None else init[tags]
        up = lambda a: rc.up(a, dev)  # noqa: E731
        self.d_r = up(es.ranges[:, tags].transpose(0, 2, 1))
        self.d_e = up(es.sch.err[tags].T)
        self.d_s = {kind: up(es.samples[kind][:, tags].transpose(0, 2, 1)) for kind in pe.WIDTH}     # (n, C, T)
        self.d_dt = up(self.dt)

    def bank(self, chunk=None):
        from roskfpos_amd import capi
        with rc.env(KFPOS_TRACE_CHUNK_STEPS=chunk):
            return capi.KfposBank(capi.MODEL_PLANAR, self.T, self.es.sch.w.anchors, storage=self.storage,
                                  init_pos=self.init, planar=pe.cfg_of(self.start))


def _final(b):
    x, P, fl = b.get_state()
    return x, P, fl, b.get_latch(), b.get_height()


def _single(b, inp, e, kind, i, status, stream, dt):
    if kind == pe.TOA:
        b.step_toa_dev(inp.d_r[i], inp.d_e, 0.0, status=status, stream=stream, dt_dev=dt)
    else:
        b.step_sensor_dev(kind, inp.d_s[kind][i], 0.0, status=status, stream=stream, dt_dev=dt)


def _call(method):
    def call(b, inp, n, dts, traj, ste, st, stream):
        nt, A, s = inp.T, inp.A, inp.d_s
        getattr(b, method)(inp.kinds[:n], dts, range_mm=inp.d_r, stride_ranges=A * nt, err_est=inp.d_e, stride_err=0,
                           px4flow=s[pe.PX4], stride_px4flow=5 * nt, imu=s[pe.IMU], stride_imu=24 * nt,
                           mag=s[pe.MAG], stride_mag=3 * nt, compass=s[pe.COMPASS], stride_compass=nt,
                           trajectory=traj, status_events=ste, status=st, stream=stream)
    return call


NAMES = ("position after every slot", "status of every slot", "x", "P", "flags", "latch", "height")
EACH = rc.Family(names=NAMES, n_kinds=5, dts=lambda inp: inp.d_dt, final=_final,
                 position=lambda b: np.vstack([b.get_state()[0][:, :2].T, b.get_height()]),
                 single=_single, call=_call("run_planar_events_each_dev"))
# the shared-timeline entry point over the same inputs; its dts: one scalar per slot
SHARED = rc.Family(**{**vars(EACH), "call": _call("run_planar_events_dev")})


def _bit_identity(A, storage, combos, tags=None):
    for start, end_on_sensor, waiting in combos:
        inp = Inputs(A, storage, start, end_on_sensor, waiting, tags=tags)
        what = f"start={start} end_on_sensor={end_on_sensor} waiting={waiting}"
        ref = rc.check_one_call(EACH, inp, what)
        words = ref[1]
        assert np.array_equal(words == ST_SKIPPED, ~inp.ran), what   # the reference run skips where the schedule says
        if inp.T > 1:
            low = words[inp.ran] & 0xFF
            assert (low == 0).mean() > 0.5 and (low & 0x04).any(), what      # most are plain; too few ranges happened
            if not pe.STARTS[start][0]:
                assert (low & 0x08).any(), what                              # ML initialisations happened
            started = np.isfinite(ref[0][-1]).all(axis=0)
            assert started[(np.arange(T) if tags is None else np.asarray(tags)) != pee.NOWHERE].all(), what


@pytest.mark.parametrize("A", [8, 5])               # compile-time anchor loops; run-time anchor loop
@pytest.mark.parametrize("storage", [0, 1, 2, 3])   # f64, f32, mixed, p48
def test_one_call_equals_the_single_calls_bit_for_bit(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(A, storage, [("fixed", True, False), ("ml3d", False, False)])


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 5), (2, 5), (3, 8)])
def test_one_call_equals_the_single_calls_for_a_single_tag(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(A, storage, [("fixed", True, False), ("ml2d", False, True)], tags=[1])   # tag 1 skips slots


OVER_64K = [("fixed", True, False), ("ml3d", False, False)]   # (start, end_on_sensor, waiting)


@pytest.mark.parametrize("storage", [0, 2])         # f64; mixed: 4-byte measurements
def test_one_call_equals_the_single_calls_behind_a_raised_lds_limit(storage):
    """31 anchors: the run-time loop's epoch and CovSpill8 take 66 048 bytes of LDS, the smallest count over 64 KB (30:
    64 512), so k_events_planar_each runs behind a raised hipFuncAttributeMaxDynamicSharedMemorySize. Tags 0..64: a full
    wavefront, whose lane 63 reaches the end of the block, and a ragged one"""
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(31, storage, OVER_64K, tags=np.arange(65))


def test_a_schedule_that_crosses_the_launch_boundary():
    """the schedule four times over, 160 slots: behind the leading ranging slot of a fresh handle a launch of 128 slots
    -- all 16 words of its `kinds` in use, slots of every kind at 64 or later in it -- and a second one for the rest"""
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    reps = 4
    inp = Inputs(8, capi.STORE_F64, "fixed")
    inp.kinds, inp.ran = np.tile(inp.kinds, reps), np.tile(inp.ran, (reps, 1))
    inp.d_r, inp.d_dt = inp.d_r.repeat(reps, 1, 1), inp.d_dt.repeat(reps, 1)
    inp.d_s = {kind: s.repeat(reps, 1, 1) for kind, s in inp.d_s.items()}
    lead = pe.launch_starts(inp.kinds, 128)[0]
    assert inp.kinds.size >= 130 and lead == 1 and len(pe.launch_starts(inp.kinds, 128)) == 2
    assert set(inp.kinds[lead + 64:lead + 128].tolist()) == {0, 1, 2, 3, 4}
    b = inp.bank()
    ref = rc.single_calls(EACH, b, inp)
    b.close()
    assert np.array_equal(ref[1] == ST_SKIPPED, ~inp.ran)
    low = ref[1][inp.ran] & 0xFF
    assert (low == 0).mean() > 0.5 and (low != 0).any() and np.isfinite(ref[0][-1]).all()
    b = inp.bank()
    got = rc.one_call(EACH, b, inp)
    b.close()
    rc.same_bytes(got, ref, NAMES, "four times the schedule")


@pytest.mark.parametrize("start,waiting,storage,A", [("fixed", False, 2, 5), ("fixed_free", False, 3, 8),
                                                     ("ml3d", True, 1, 8), ("ml2d", True, 0, 5),
                                                     ("ml3d", False, 3, 5), ("ml2d", False, 2, 8)])
def test_the_four_starts_and_the_waiting_prefix(start, waiting, storage, A):
    """waiting: two sensor slots ahead of every tag's first ranging -- tags run events while they wait for their ML
    start, and the call has no leading ranging slot"""
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(A, storage, [(start, True, waiting)])


LEAD = np.array([0, 0, 0, 2, 0, 1, 4, 0, 3, 0, 2], dtype=np.uint8)


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 5), (3, 8), (2, 5)])
def test_leading_ranging_slots_on_a_fresh_handle_and_on_one_with_latches(storage, A):
    """On a handle that never had a sample the ranging slots ahead of the call's first sensor slot run the ranging-only
    kernel, as single calls do, tags absent from them included; on a handle that has latches from earlier single calls
    the same schedule carries them in those slots. A call of leading ranging slots only reports the last one's status."""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    inp = Inputs(A, storage, "fixed", kinds=LEAD)
    lead = inp.mask[:3]
    assert (~lead).any(axis=1).all() and lead.any(axis=1).all() and not lead[:, 64:128].all(axis=0).all()
    ref = rc.check_one_call(EACH, inp, "fresh handle", chunks=(None, 3))
    assert (ref[4][np.arange(T) != pee.NOWHERE] & FL_STARTED).all()
    rc.check_one_call(EACH, inp, "fresh handle, ranging slots only", chunks=(None, 2), n_slots=3)

    def prepare(b):
        stream = torch.cuda.current_stream().cuda_stream
        for kind in (pe.IMU, pe.PX4, pe.MAG):
            b.step_sensor_dev(kind, inp.d_s[kind][-1], 0.01, stream=stream, dt_dev=inp.d_dt[-1])
        torch.cuda.synchronize()

    latched = rc.check_one_call(EACH, inp, "latched before the call", prepare, chunks=(None, 3))
    assert latched[3].tobytes() != ref[3].tobytes()               # the leading slots carried the latches
    rc.check_one_call(EACH, inp, "latched before the call, ranging slots only", prepare, chunks=(None, 2), n_slots=3)


@pytest.mark.parametrize("storage,A,start", [(3, 8, "fixed"), (1, 5, "ml3d"), (3, 5, "ml2d"), (1, 8, "fixed")])
def test_a_tag_that_runs_nothing_keeps_every_stored_byte(storage, A, start):
    """(What this can and cannot see: the record is read back through get_tags, decoded. A lane that ran nothing and
    stored its record all the same would rewrite state and covariance with the values it loaded -- the same bytes -- so
    it shows in the flags word of the fresh tag, which would come back started, and in latch rows, which are only ever
    written for kinds a lane sampled.)
    tag 5 is in no slot: state, covariance planes, latch rows, height and the flags word stay as set_tags left them
    -- the tag stays not started; tag 6 is taken out of every slot as well and holds a started record with latches. In
    every other tag the latch rows of kinds it never sampled (thirty tags are kept away from one kind each) keep the
    sentinel they were given."""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    inp = Inputs(A, storage, start)
    quiet = [pee.NOWHERE, 6]
    mask = inp.mask.copy()
    mask[:, 6] = False
    # tags 10..19 sit every PX4Flow slot out, 20..29 every IMU slot, 30..39 every magnetometer and compass slot
    mask[np.ix_(inp.kinds == pe.PX4, np.arange(10, 20))] = False
    mask[np.ix_(inp.kinds == pe.IMU, np.arange(20, 30))] = False
    mask[np.ix_(np.isin(inp.kinds, [pe.MAG, pe.COMPASS]), np.arange(30, 40))] = False
    d_dt = torch.from_numpy(np.where(mask, inp.dt, -1.0)).to(inp.d_r.device)
    ran = mask & ~inp.es.dropped
    rng = np.random.default_rng(5)
    m = rng.normal(size=(2, 8, 8))
    P = m @ m.transpose(0, 2, 1) * 1.234567890123e-2       # not representable in 24 or 39 mantissa bits
    x = rng.normal(size=(2, 8)) * 1.23456789
    latch = rng.normal(size=(2, 15)) * 0.123456789
    height = np.array([1.0123456789, 0.987654321])
    for chunk in (None, 7):
        b = inp.bank(chunk)
        b.set_latch(np.full((T, 15), SENTINEL))
        b.set_tags(quiet, x=x, P=P, latch=latch, height=height)
        b.set_tags([6], flags=np.array([FL_STARTED | HAS_PX4 | HAS_MAG], dtype=np.uint32))
        before = b.get_tags(quiet)
        assert before[2].tolist() == [0, FL_STARTED | HAS_PX4 | HAS_MAG] and not np.array_equal(before[1], P)
        got = rc.one_call(EACH, b, inp, dts=d_dt)
        after = b.get_tags(quiet)
        for u, v, name in zip(before, after, ("x", "P", "flags", "latch", "height")):
            assert u.tobytes() == v.tobytes(), (name, chunk)
        assert (got[1][:, quiet] == ST_SKIPPED).all()
        flags, rows = got[4], got[5]
        others = np.setdiff1d(np.arange(T), quiet)
        assert (flags[others] & FL_STARTED).all()
        for kinds, bit, cols in (([pe.PX4], HAS_PX4, slice(0, 5)), ([pe.IMU], HAS_IMU, slice(5, 13)),
                                 ([pe.MAG, pe.COMPASS], HAS_MAG, slice(13, 15))):
            sampled = ran[np.isin(inp.kinds, kinds)].any(axis=0)[others]
            assert sampled.any() and not sampled.all()
            assert ((flags[others] & bit) != 0).tolist() == sampled.tolist(), (kinds, chunk)
            assert (rows[others][:, cols] == SENTINEL).all(axis=1).tolist() == (~sampled).tolist(), (kinds, chunk)
            assert (rows[others][:, cols] != SENTINEL).all(axis=1).tolist() == sampled.tolist(), (kinds, chunk)
        b.close()


@pytest.mark.parametrize("storage,A", [(2, 8), (0, 5)])
def test_a_nan_dt_runs_the_event_as_the_single_call_does(storage, A):
    """the predicate is dt < 0.0: a NaN dt takes part. Tags 3 and 70 get one in an IMU slot, tags 9 and 129 in a ranging
    slot, whether the mask has them there or not; what comes out are the bytes the single calls leave."""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    inp = Inputs(A, storage, "fixed", fill=False)
    e_imu, e_toa = 18, 21
    assert inp.kinds[e_imu] == pe.IMU and inp.kinds[e_toa] == pe.TOA
    dt = inp.dt.copy()
    dt[e_imu, [3, 70]] = np.nan
    dt[e_toa, [9, 129]] = np.nan
    d_dt = torch.from_numpy(dt).to(inp.d_r.device)
    ref = rc.check_one_call(EACH, inp, "NaN dt", dts=d_dt)
    assert not (ref[1][e_imu, [3, 70]] == ST_SKIPPED).any() and not (ref[1][e_toa, [9, 129]] == ST_SKIPPED).any()
    assert (ref[1][e_imu, [3, 70]] & 32).all() and (ref[1][e_toa, [9, 129]] & 32).all()   # ... and KFPOS_ST_NONFINITE


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 8), (2, 8), (3, 8), (2, 5), (3, 5)])
def test_an_all_present_schedule_equals_run_planar_events_dev(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    for start, end_on_sensor, waiting in (("fixed", True, False), ("ml2d", False, True)):
        inp = Inputs(A, storage, start, end_on_sensor, waiting, fill=False)   # everybody takes part: every entry is read
        d_dt = torch.from_numpy(np.ascontiguousarray(np.broadcast_to(inp.base[:, None], inp.dt.shape))).to(inp.d_r.device)
        for chunk in (None, 7):
            b = inp.bank(chunk)
            ref = rc.one_call(SHARED, b, inp, dts=inp.base)
            b.close()
            b = inp.bank(chunk)
            got = rc.one_call(EACH, b, inp, dts=d_dt)
            b.close()
            rc.same_bytes(got, ref, NAMES, f"start={start} chunk={chunk}")
        assert np.array_equal(ref[1] == ST_SKIPPED, inp.es.dropped)


@pytest.mark.parametrize("A", [8, 5])
@pytest.mark.parametrize("start", ["fixed", "fixed_free", "ml3d", "ml2d"])
def test_f64_storage_matches_the_oracle_after_every_slot(start, A, T=T):
    """position RMS <= 1e-9 m and max <= 1e-8 m after every slot over the tags that ran it (the bounds of
    tests/test_planar_events_gpu.py for the same comparison), every status word equal to the oracle's, a tag that sat
    the slot out reports the bytes of its previous row. Measured on an MI355X, worst over the slots, A = 8 / A = 5:
    fixed and fixed_free start RMS 1.8e-16 / 1.7e-16 m (max 8.9e-16 m); ml3d RMS 1.6e-15 / 4.2e-15 m (max 5.8e-15 /
    1.3e-14 m); ml2d RMS 4.0e-10 / 7.7e-10 m (max 3.4e-9 / 5.3e-9 m)."""
    if not has_gpu():
        pytest.skip("no GPU")
    from planar import PlanarOracle
    inp = Inputs(A, 0, start, True, waiting=not pe.STARTS[start][0], tags=np.arange(T))   # (the oracle: all 130)
    assert (inp.dt[inp.mask] > 0).all()           # dt = 0 stays out of this leg
    b = inp.bank()
    got = rc.one_call(EACH, b, inp)
    b.close()
    sch = inp.es.sch
    po, so = pee.replay(PlanarOracle(sch.w, pe.cfg_of(start), pe.init_of(sch, start)), inp.es)
    po, so = po[:, :T], so[:, :T]
    worst = [0.0, 0.0]
    for e in range(inp.kinds.size):
        ran = inp.ran[e]
        assert ran.any()
        pg = got[0][e].T
        assert pg.shape == po[e].shape == (T, 3)
        rms, mx, same_waiting = pe.distance(pg[ran], po[e][ran])
        worst = [max(worst[0], rms), max(worst[1], mx)]
        print(f"slot {e} kind {inp.kinds[e]}: {int(ran.sum())} tags, RMS {rms:.3e} m, max {mx:.3e} m")
        assert same_waiting, e                   # no tag left out of the comparison on one side only
        assert rms <= 1e-9 and mx <= 1e-8, (e, rms, mx)
        assert np.array_equal(so[e], got[1][e].astype(np.uint32)), (e, "status words")
        if e:
            assert got[0][e].T[~ran].tobytes() == got[0][e - 1].T[~ran].tobytes(), e
    print(f"A={A} start={start}: worst RMS {worst[0]:.3e} m, worst max {worst[1]:.3e} m against the oracle over "
          f"{inp.kinds.size} slots")
    started = np.isfinite(got[0][-1]).all(axis=0)
    assert started[np.arange(T) != pee.NOWHERE].all() and np.isfinite(po[-1][np.arange(T) != pee.NOWHERE]).all()


@pytest.mark.parametrize("start", ["fixed", "fixed_free"])
def test_f64_storage_matches_the_oracle_behind_a_raised_lds_limit(start):
    """the same bounds at 31 anchors and tags 0..64 (more than 64 KB of LDS), from a fixed start: an ML start stays with the
    bit-identity test above. Beyond a dozen anchors the Gauss-Newton walk of a few tags' ML initialisation is chaotic
    (cases.py, "No 16-anchor ML-init case"): on the CPU alone the host emulation of the kernel arithmetic and the oracle
    then part by 1e-7 ... 3e-2 m on 2 to 4 of 130 tags and count different gain iterations. Measured with the library
    before launch selection moved into kfpos_launch_plan.h, the 9-state replays at 17 anchors miss the bound from an ML start (tests/test_run_events_gpu.py)."""
    test_f64_storage_matches_the_oracle_after_every_slot(start, 31, T=65)


def _raw_call(b, n, kinds, d_dt, inputs):
    p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())  # noqa: E731
    return b.lib.kfpos_run_planar_events_each_dev(b._h, n, p(kinds), p(d_dt),
                                                  None if inputs is None else ctypes.byref(inputs), None, None, None,
                                                  None)


def _snapshot(b):
    from roskfpos_amd import capi
    x, P, fl = b.get_state()
    parts = [x, P, fl]
    if b.model == capi.MODEL_PLANAR:
        parts += [b.get_latch(), b.get_height()]
    return b"".join(np.ascontiguousarray(p).tobytes() for p in parts)


def test_argument_errors_are_decided_before_anything_runs():
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    A = 8
    inp = Inputs(A, capi.STORE_MIXED, "fixed", fill=False)
    s = inp.d_s

    def inputs(**without):
        full = dict(range_mm=inp.d_r.data_ptr(), stride_ranges=A * T, err_est=inp.d_e.data_ptr(), stride_err=0,
                    px4flow=s[pe.PX4].data_ptr(), stride_px4flow=5 * T, imu=s[pe.IMU].data_ptr(), stride_imu=24 * T,
                    mag=s[pe.MAG].data_ptr(), stride_mag=3 * T, compass=s[pe.COMPASS].data_ptr(), stride_compass=T)
        full.update(without)
        return capi.PlanarInputs(**full)

    b = inp.bank()
    rc.one_call(EACH, b, inp, n_slots=14)                              # a bank with something in it
    before = _snapshot(b)
    k, d = inp.kinds[:14].copy(), inp.d_dt
    assert set(k.tolist()) == {0, 1, 2, 3, 4}
    bad = k.copy()
    bad[4] = 5
    only = lambda kind: np.full(3, kind, dtype=np.uint8)  # noqa: E731
    refused = {
        "n_events < 0": (-1, k, d, inputs()),
        "a kind outside 0..4": (14, bad, d, inputs()),
        "kinds missing": (14, None, d, inputs()),
        "dt_events_dev missing": (14, k, None, inputs()),
        "in missing": (14, k, d, None),
        "range_mm missing, ranging slots": (14, k, d, inputs(range_mm=None)),
        "err_est missing, ranging slots": (3, only(0), d, inputs(err_est=None)),
        "px4flow missing, PX4Flow slots": (14, k, d, inputs(px4flow=None)),
        "imu missing, IMU slots": (3, only(2), d, inputs(imu=None)),
        "mag missing, magnetometer slots": (14, k, d, inputs(mag=None)),
        "compass missing, compass slots": (3, only(4), d, inputs(compass=None)),
    }
    for what, args in refused.items():
        assert _raw_call(b, *args) == ERR_ARG, what
        assert _snapshot(b) == before, what
    assert _raw_call(b, 14, bad, d, inputs()) == ERR_ARG
    msg = b.lib.kfpos_last_error()
    assert b"kfpos_run_planar_events_each_dev" in msg and b"kinds[4]" in msg     # the first offending slot is named
    assert _raw_call(b, 14, k, d, inputs(mag=None)) == ERR_ARG
    first_mag = int(np.flatnonzero(k == pe.MAG)[0])
    assert f"kinds[{first_mag}]".encode() in b.lib.kfpos_last_error()
    # n_events == 0 touches nothing; arrays of kinds that do not occur may be missing
    assert _raw_call(b, 0, None, None, None) == 0
    assert _raw_call(b, 0, k, d, inputs()) == 0
    assert _snapshot(b) == before, "n_events == 0"
    assert _raw_call(b, 3, only(0), d, inputs(px4flow=None, imu=None, mag=None, compass=None)) == 0
    assert _raw_call(b, 3, only(2), d, inputs(range_mm=None, err_est=None, px4flow=None, mag=None, compass=None)) == 0
    assert _snapshot(b) != before
    b.close()

    # another model
    w = inp.es.sch.w
    b6 = capi.KfposBank(capi.MODEL_TOA, T, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions())
    b6.step_toa_dev(inp.d_r[0], inp.d_e, 0.1)
    before = _snapshot(b6)
    assert _raw_call(b6, 14, k, d, inputs()) == ERR_MODEL
    assert _raw_call(b6, 3, only(0), d, inputs()) == ERR_MODEL
    assert _snapshot(b6) == before
    b6.close()

    # a planar handle whose anchors are not set: ranging slots are refused, sensor slots run
    lib = capi.load()
    cfg = capi._Config()
    cfg.model, cfg.n_tags, cfg.max_anchors, cfg.storage = capi.MODEL_PLANAR, T, A, capi.STORE_MIXED
    cfg.accel_noise, cfg.jolt, cfg.cost_threshold, cfg.use_init_pos = 0.5, 0.5, 0.5, 1
    cfg.init_pos = (ctypes.c_double * 3)(5.0, 5.0, 1.0)
    h = ctypes.c_void_p()
    assert lib.kfpos_create(ctypes.byref(cfg), ctypes.byref(h)) == 0
    bare = capi.KfposBank.__new__(capi.KfposBank)
    bare.lib, bare._h, bare.T, bare.A, bare.model, bare.storage = lib, h, T, A, capi.MODEL_PLANAR, capi.STORE_MIXED
    bare.n = lib.kfpos_state_dim(h)
    assert lib.kfpos_init(h) == 0
    planar_cfg = capi.PlanarConfig(**pe.cfg_of("fixed"))
    assert lib.kfpos_set_planar(h, ctypes.byref(planar_cfg)) == 0
    before = _snapshot(bare)
    assert _raw_call(bare, 14, k, d, inputs()) == ERR_STATE
    assert _snapshot(bare) == before
    assert _raw_call(bare, 3, only(2), d, inputs()) == 0
    assert _snapshot(bare) != before
    bare.close()
