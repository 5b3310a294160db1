"""kfpos_run_planar_events_dev: a multi-sensor event schedule of the 8-state planar filter in one call computes, bit for
bit, what the same events give as single kfpos_step_toa_dev / kfpos_step_sensor_dev calls -- state, height, covariance
as stored, flags, all 15 latch rows, the status word and the position of every event -- and stays with the oracle after
every event.

One schedule serves every test (tests/planar_events.py; tests/test_planar_events_schedule.py checks on the CPU that it
holds what it is meant to hold): a leading ranging event on a handle without latches, all five event kinds, PX4Flow
samples of quality 0 on every 16th tag, the dropout rows of planar.epoch_ranges; it ends on a ranging event or on a
sensor event, and prefixed with two sensor events it has tags waiting for their ML start. With KFPOS_TRACE_CHUNK_STEPS=7
a launch boundary falls between two sensor events and another directly before a ranging event."""
import copy
import ctypes

import numpy as np
import pytest

import planar_events as pe
import replay_checks as rc
from conftest import has_gpu

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_MODEL, ERR_STATE = 1, 4, 5
HAS_PX4, HAS_IMU, HAS_MAG = 1 << 5, 1 << 6, 1 << 7      # planar flags word: what a tag has latched


class Inputs:
    """a schedule's inputs in HBM, component-major"""

    def __init__(self, T, A, storage, start, end_on_sensor=True, waiting=False, dev="cuda:0"):
        from roskfpos_amd import capi
        self.T, self.A, self.storage, self.start = T, A, storage, start
        real = np.float64 if storage == capi.STORE_F64 else np.float32
        sch = self.sch = pe.Schedule(T, A, end_on_sensor, waiting, real)
        self.kinds, self.dts = sch.kinds, sch.dts.copy()
        up = lambda a: rc.up(a, dev)  # noqa: E731
        self.d_r, self.d_e = up(sch.ranges.transpose(0, 2, 1)), up(sch.err.T)
        self.d_s = {kind: up(sch.samples[kind].transpose(0, 2, 1)) for kind in pe.WIDTH}     # (n, C, T)

    def bank(self, chunk=None):
        from roskfpos_amd import capi
        with rc.env(KFPOS_TRACE_CHUNK_STEPS=chunk):
            return capi.KfposBank(capi.MODEL_PLANAR, self.T, self.sch.w.anchors, storage=self.storage,
                                  init_pos=pe.init_of(self.sch, self.start), planar=pe.cfg_of(self.start))

    def under(self, kinds):
        """the same inputs under other kinds, with the first dts of the schedule"""
        other = copy.copy(self)
        other.kinds = kinds
        return other


def _final(b):
    x, P, fl = b.get_state()
    return x, P, fl, b.get_latch(), b.get_height()


def _single(b, inp, e, kind, i, status, stream, dt):
    if kind == pe.TOA:
        b.step_toa_dev(inp.d_r[i], inp.d_e, dt, status=status, stream=stream)
    else:
        b.step_sensor_dev(kind, inp.d_s[kind][i], dt, status=status, stream=stream)


def _call(b, inp, n, dts, traj, ste, st, stream):
    T, A, s = inp.T, inp.A, inp.d_s
    b.run_planar_events_dev(inp.kinds[:n], dts, range_mm=inp.d_r, stride_ranges=A * T, err_est=inp.d_e, stride_err=0,
                            px4flow=s[pe.PX4], stride_px4flow=5 * T, imu=s[pe.IMU], stride_imu=24 * T,
                            mag=s[pe.MAG], stride_mag=3 * T, compass=s[pe.COMPASS], stride_compass=T,
                            trajectory=traj, status_events=ste, status=st, stream=stream)


NAMES = ("position after every event", "status of every event", "x", "P", "flags", "latch", "height")
FAM = rc.Family(names=NAMES, n_kinds=5, dts=lambda inp: inp.dts, final=_final,
                position=lambda b: np.vstack([b.get_state()[0][:, :2].T, b.get_height()]),
                single=_single, call=_call)


# start x ends on a sensor event x sensor events ahead of the first ranging (the waiting case of an ML start)
EVERY = [(s, e, False) for s in pe.STARTS for e in (False, True)] + [("ml3d", True, True), ("ml2d", True, True)]


def _bit_identity(T, A, storage, combos):
    for start, end_on_sensor, waiting in combos:
        inp = Inputs(T, A, storage, start, end_on_sensor, waiting)
        what = f"start={start} end_on_sensor={end_on_sensor} waiting={waiting}"
        ref = rc.check_one_call(FAM, inp, what)
        low = ref[1] & 0xFF
        assert (low == 0).mean() > 0.5, what                 # most status words are plain
        if T > 16:
            assert np.array_equal((low & 0x40) != 0, inp.sch.dropped()), what    # dropped PX4Flow samples: skipped
            assert (low & 0x40).any() and (low & 0x04).any(), what               # ... and too few ranges
        if not pe.STARTS[start][0]:
            assert (low & 0x08).any(), what                                      # ML initialisations happened
        assert np.isfinite(ref[0][-1]).all(), what           # every tag has started by the end


@pytest.mark.parametrize("A", [8, 5])               # compile-time anchor loops; run-time anchor loop
@pytest.mark.parametrize("storage", [0, 1, 2, 3])   # f64, f32, mixed, p48
def test_one_call_equals_the_single_calls_bit_for_bit(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(130, A, storage, EVERY)           # two full wavefronts and one of two lanes


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 5), (2, 5), (3, 8)])
def test_one_call_equals_the_single_calls_for_a_single_tag(storage, A):
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(1, A, storage, [("fixed", True, False), ("ml2d", False, True)])


OVER_64K = [("fixed", False, False), ("ml3d", True, True)]   # (start, end_on_sensor, waiting)


@pytest.mark.parametrize("storage", [0, 2])         # f64; mixed: 4-byte measurements
def test_one_call_equals_the_single_calls_behind_a_raised_lds_limit(storage):
    """31 anchors: the run-time loop's epoch and CovSpill8 take 66 048 bytes of LDS, the smallest count over 64 KB (30:
    64 512), so k_events_planar runs behind a raised hipFuncAttributeMaxDynamicSharedMemorySize. 65 tags: a full
    wavefront, whose lane 63 reaches the end of the block, and a ragged one"""
    if not has_gpu():
        pytest.skip("no GPU")
    _bit_identity(65, 31, storage, OVER_64K)


def test_a_schedule_that_crosses_the_launch_boundary():
    """the schedule four times over, 160 events: behind the leading ranging event a launch of 128 events -- all 16 words
    of its `kinds` in use, events of every kind at 64 or later in it -- and a second one for the rest"""
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    reps = 4
    inp = Inputs(130, 8, capi.STORE_F64, "fixed")
    kinds, inp.dts = np.tile(inp.kinds, reps), np.tile(inp.dts, reps)
    inp.kinds = kinds
    inp.d_r = inp.d_r.repeat(reps, 1, 1)
    inp.d_s = {kind: s.repeat(reps, 1, 1) for kind, s in inp.d_s.items()}
    lead = pe.launch_starts(kinds, 128)[0]
    assert kinds.size >= 130 and lead == 1 and len(pe.launch_starts(kinds, 128)) == 2
    assert set(kinds[lead + 64:lead + 128].tolist()) == {0, 1, 2, 3, 4}
    b = inp.bank()
    ref = rc.single_calls(FAM, b, inp)
    b.close()
    low = ref[1] & 0xFF
    assert (low == 0).mean() > 0.5 and (low != 0).any() and np.isfinite(ref[0][-1]).all()
    b = inp.bank()
    got = rc.one_call(FAM, b, inp)
    b.close()
    rc.same_bytes(got, ref, NAMES, "four times the schedule")


@pytest.mark.parametrize("storage,A", [(0, 8), (2, 5), (3, 8)])
def test_a_handle_that_already_holds_latched_samples(storage, A):
    """earlier single calls left all three latches behind: the leading ranging event carries them, and kinds the call
    never samples keep their rows"""
    if not has_gpu():
        pytest.skip("no GPU")
    import torch
    inp = Inputs(130, A, storage, "fixed")

    def prepare(b):
        stream = torch.cuda.current_stream().cuda_stream
        for kind in (pe.IMU, pe.PX4, pe.MAG):
            b.step_sensor_dev(kind, inp.d_s[kind][-1], 0.01, stream=stream)
        torch.cuda.synchronize()

    ref = rc.check_one_call(FAM, inp, "latched before the call", prepare)
    assert (ref[4] & (HAS_PX4 | HAS_IMU | HAS_MAG) == (HAS_PX4 | HAS_IMU | HAS_MAG)).all()
    # ranging and IMU events only: the PX4Flow and magnetometer rows are what the earlier calls left
    only = np.array([0, 2, 0, 2, 2, 0, 2], dtype=np.uint8)
    b = inp.bank()
    prepare(b)
    before = b.get_latch()
    b.close()
    ref = rc.check_one_call(FAM, inp.under(only), "latched before the call, IMU and ranging only", prepare,
                            chunks=(None, 3, 7))
    assert ref[5][:, :5].tobytes() == before[:, :5].tobytes() and ref[5][:, 13:].tobytes() == before[:, 13:].tobytes()
    assert (ref[5][:, 5:7] != before[:, 5:7]).all()


@pytest.mark.parametrize("storage,A", [(0, 8), (2, 5)])
def test_latch_rows_of_kinds_a_lane_never_sampled_keep_what_hbm_holds(storage, A):
    """the HBM latch pre-filled with a sentinel, `has` bits clear: a launch writes back only the rows of kinds the
    lane sampled in it -- also not the PX4Flow rows of a lane whose samples were all dropped"""
    if not has_gpu():
        pytest.skip("no GPU")
    SENTINEL = -12345.6789
    inp = Inputs(130, A, storage, "fixed")

    def prepare(b):
        b.set_latch(np.full((inp.T, 15), SENTINEL))

    # kinds of the schedule, and whether it samples (PX4Flow, IMU, magnetometer / compass)
    for kinds, sampled in (([0, 2, 0, 2, 2, 0], [False, True, False]), ([1, 0, 2, 0, 3, 2], [True, True, True]),
                           ([0, 4, 1, 0], [True, False, True])):
        kinds = np.array(kinds, dtype=np.uint8)
        ref = rc.check_one_call(FAM, inp.under(kinds), f"sentinel kinds={kinds.tolist()}", prepare,
                                chunks=(None, 2, 7))
        latch, flags = ref[5], ref[4]
        n_px4 = int((kinds == pe.PX4).sum())
        got_px4 = (inp.sch.samples[pe.PX4][:n_px4, :, 4] != 0).any(axis=0) if n_px4 else np.zeros(inp.T, dtype=bool)
        assert (n_px4 > 0) == sampled[0] and (n_px4 == 0 or (got_px4.any() and not got_px4.all()))
        assert ((latch[:, :5] == SENTINEL).all(axis=1) == ~got_px4).all()
        assert ((flags & HAS_PX4) != 0).tolist() == got_px4.tolist()
        assert (latch[:, 5:13] == SENTINEL).all() == (not sampled[1])
        assert (latch[:, 5:7] != SENTINEL).all() == sampled[1]
        assert (latch[:, 13:] == SENTINEL).all() == (not sampled[2])
        assert (latch[:, 13:] != SENTINEL).all() == sampled[2]
        assert ((flags & HAS_IMU) != 0).all() == sampled[1] and ((flags & HAS_MAG) != 0).all() == sampled[2]


@pytest.mark.parametrize("storage,A", [(0, 8), (1, 5)])
def test_an_event_with_dt_zero(storage, A):
    """GPU against GPU only: the oracle leg stays away from dt = 0"""
    if not has_gpu():
        pytest.skip("no GPU")
    inp = Inputs(130, A, storage, "fixed")
    at = 18                                     # an IMU event inside a run of four
    assert inp.kinds[at] == pe.IMU and inp.kinds[at - 1] == pe.IMU
    dts = inp.dts.copy()
    dts[at] = 0.0
    rc.check_one_call(FAM, inp, "dt = 0", dts=dts)


@pytest.mark.parametrize("A", [8, 5])
@pytest.mark.parametrize("start", ["fixed", "ml3d", "ml2d"])
def test_f64_storage_matches_the_oracle_after_every_event(start, A, T=130):
    """position RMS <= 1e-9 m and max <= 1e-8 m after every event (the bounds tests/test_run_events_gpu.py takes from
    tests/test_gpu_parity.py), every status word equal to the oracle's, no tag left out, every tag started by the end"""
    if not has_gpu():
        pytest.skip("no GPU")
    from planar import PlanarOracle
    inp = Inputs(T, A, 0, start, True, waiting=start != "fixed")
    b = inp.bank()
    got = rc.one_call(FAM, b, inp)
    b.close()
    po, so = pe.replay(PlanarOracle(inp.sch.w, pe.cfg_of(start), pe.init_of(inp.sch, start)), inp.sch)
    worst = [0.0, 0.0]
    for e in range(inp.kinds.size):
        pg = got[0][e].T
        assert pg.shape == po[e].shape == (T, 3)
        rms, mx, same_waiting = pe.distance(pg, po[e])
        worst = [max(worst[0], rms), max(worst[1], mx)]
        print(f"event {e} kind {inp.kinds[e]}: RMS {rms:.3e} m, max {mx:.3e} m")
        assert same_waiting, e                   # no tag left out of the comparison on one side only
        assert rms <= 1e-9 and mx <= 1e-8, (e, rms, mx)
        assert np.array_equal(so[e], got[1][e].astype(np.uint32)), (e, "status words")
    print(f"A={A} start={start}: worst RMS {worst[0]:.3e} m, worst max {worst[1]:.3e} m against the oracle over "
          f"{inp.kinds.size} events")
    assert np.isfinite(got[0][-1]).all() and np.isfinite(po[-1]).all()     # every tag has started by the end


@pytest.mark.parametrize("start", ["fixed", "fixed_free"])
def test_f64_storage_matches_the_oracle_behind_a_raised_lds_limit(start):
    """the same bounds at 31 anchors and 65 tags (more than 64 KB of LDS), from a fixed start: an ML start stays with the
    bit-identity test above. Beyond a dozen anchors the Gauss-Newton walk of a few tags' ML initialisation is chaotic
    (cases.py, "No 16-anchor ML-init case"): on the CPU alone the host emulation of the kernel arithmetic and the oracle
    then part by 1e-7 ... 3e-2 m on 2 to 4 of 130 tags and count different gain iterations. Measured with the library
    before launch selection moved into kfpos_launch_plan.h, the 9-state replays at 17 anchors miss the bound from an ML start (tests/test_run_events_gpu.py)."""
    test_f64_storage_matches_the_oracle_after_every_event(start, 31, T=65)


def _raw_call(b, n, kinds, dts, inputs):
    p = lambda x: None if x is None else (x.ctypes.data if isinstance(x, np.ndarray) else x.data_ptr())  # noqa: E731
    return b.lib.kfpos_run_planar_events_dev(b._h, n, p(kinds), p(dts),
                                             None if inputs is None else ctypes.byref(inputs), None, None, None, None)


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
    T, A = 130, 8
    inp = Inputs(T, A, capi.STORE_MIXED, "fixed")
    s = inp.d_s

    def inputs(**without):
        full = dict(range_mm=inp.d_r.data_ptr(), stride_ranges=A * T, err_est=inp.d_e.data_ptr(), stride_err=0,
                    px4flow=s[pe.PX4].data_ptr(), stride_px4flow=5 * T, imu=s[pe.IMU].data_ptr(), stride_imu=24 * T,
                    mag=s[pe.MAG].data_ptr(), stride_mag=3 * T, compass=s[pe.COMPASS].data_ptr(), stride_compass=T)
        full.update(without)
        return capi.PlanarInputs(**full)

    b = inp.bank()
    rc.one_call(FAM, b, inp, n_slots=14)            # a bank with something in it
    before = _snapshot(b)
    k, d = inp.kinds[:14].copy(), inp.dts[:14].copy()
    assert set(k.tolist()) == {0, 1, 2, 3, 4}
    bad = k.copy()
    bad[4] = 5
    only = lambda kind: np.full(3, kind, dtype=np.uint8)  # noqa: E731
    refused = {
        "n_events < 0": (-1, k, d, inputs()),
        "a kind outside 0..4": (14, bad, d, inputs()),
        "kinds missing": (14, None, d, inputs()),
        "dt_events missing": (14, k, None, inputs()),
        "in missing": (14, k, d, None),
        "range_mm missing, ranging events": (14, k, d, inputs(range_mm=None)),
        "err_est missing, ranging events": (3, only(0), d, inputs(err_est=None)),
        "px4flow missing, PX4Flow events": (14, k, d, inputs(px4flow=None)),
        "imu missing, IMU events": (3, only(2), d, inputs(imu=None)),
        "mag missing, magnetometer events": (14, k, d, inputs(mag=None)),
        "compass missing, compass events": (3, only(4), d, inputs(compass=None)),
    }
    for what, args in refused.items():
        assert _raw_call(b, *args) == ERR_ARG, what
        assert _snapshot(b) == before, what
    assert _raw_call(b, 14, bad, d, inputs()) == ERR_ARG
    assert b"kinds[4]" in b.lib.kfpos_last_error()             # the first offending event is named
    assert _raw_call(b, 14, k, d, inputs(mag=None)) == ERR_ARG
    first_mag = int(np.flatnonzero(k == pe.MAG)[0])
    assert f"kinds[{first_mag}]".encode() in b.lib.kfpos_last_error()
    # n_events == 0 changes nothing; arrays of kinds that do not occur may be missing
    assert _raw_call(b, 0, None, None, None) == 0
    assert _raw_call(b, 0, k, d, inputs()) == 0
    assert _snapshot(b) == before, "n_events == 0"
    assert _raw_call(b, 3, only(0), d, inputs(px4flow=None, imu=None, mag=None, compass=None)) == 0
    assert _raw_call(b, 3, only(2), d, inputs(range_mm=None, err_est=None, px4flow=None, mag=None, compass=None)) == 0
    assert _snapshot(b) != before
    b.close()

    # another model
    w = inp.sch.w
    b6 = capi.KfposBank(capi.MODEL_TOA, T, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions())
    b6.step_toa_dev(inp.d_r[0], inp.d_e, 0.1)
    before = _snapshot(b6)
    assert _raw_call(b6, 14, k, d, inputs()) == ERR_MODEL
    assert _raw_call(b6, 3, only(0), d, inputs()) == ERR_MODEL
    assert _snapshot(b6) == before
    b6.close()

    # a planar handle whose anchors are not set: ranging events are refused, sensor events run
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
