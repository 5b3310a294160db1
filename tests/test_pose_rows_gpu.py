"""Pose for a row list on the card: kfpos_get_pose_rows / kfpos_get_predicted_rows return, for a LIST of rows, bit for bit
the rows of kfpos_get_pose_each / kfpos_get_predicted (the same per-tag code under the same contraction mode: every
comparison here is on the bit patterns, there is no tolerance), and a row-list streaming round with KFPOS_SLOT_POSE_COV
returns the covariance and velocity of its tags.

Shapes as tests/test_tag_lifecycle_gpu.py: every model in all four storage modes, 100 tags x 8 anchors (the small bank's
mapped block) and 1000 x 8 (the device staging area; not a multiple of the wavefront). Banks are stepped EPOCHS epochs
with that file's `apply`; three rows are then reset so that tags which have not started occur in the lists."""
import ctypes
import functools

import numpy as np
import pytest

from roskfpos_amd.synth import Workload
from test_tag_lifecycle_gpu import IMU, ML, MODELS, PARAMS, apply, inputs, make_bank, real_of, snapshot

pytestmark = pytest.mark.gpu

EPOCHS = 8               # the planar trace has fed all four of its sensors by then
ERR_ARG, ERR_STATE = 1, 5
ST_NOT_STARTED = 16


def same_bits(p, q):
    p, q = np.ascontiguousarray(p), np.ascontiguousarray(q)
    return p.shape == q.shape and p.dtype == q.dtype and bool((p.view(np.uint8) == q.view(np.uint8)).all())


def reset_rows(T):
    return np.array([3, T // 2, T - 2], dtype=np.int32)


def dt_of_rows(T):
    d = 0.01 * (np.arange(T) % 7) + 0.005
    d[0], d[5] = 0.0, 0.25
    return d


def stepped_bank(name, storage, T):
    w = Workload(T, 8)
    b = make_bank(name, storage, w)
    for s in range(EPOCHS):
        apply(b, name, s, inputs(name, w, s, real_of(storage)))
    b.reset_tags(reset_rows(T))
    return b, w


@functools.lru_cache(maxsize=None)
def bank_and_reference(name, storage, T):
    """A stepped bank and what the whole-bank calls return for it: computed once, read by every test, never changed."""
    b, _ = stepped_bank(name, storage, T)
    dts = {"each": dt_of_rows(T), 0.0: np.zeros(T), 0.25: np.full(T, 0.25)}
    ref = {k: (b.get_pose_each(d), b.get_predicted(d)) for k, d in dts.items()}
    assert ref[0.0][0][3][3] & ST_NOT_STARTED and not ref[0.0][0][3][7] & ST_NOT_STARTED
    return b, dts["each"], ref


def row_lists(T):
    return [np.array([T - 1, 5, 0, T // 2, 17, 3], dtype=np.int32), np.array([T // 3], dtype=np.int32),
            np.arange(T, dtype=np.int32)[::-1].copy()]


def assert_rows_of(got, whole, rows, what):
    assert len(got) == len(whole)
    for k, (g, f) in enumerate(zip(got, whole)):
        assert same_bits(g, f[rows]), f"{what}: output {k}"


# ---------------------------------------------------------------- 1. the calls = rows of the whole-bank calls
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_pose_and_predicted_rows_equal_rows_of_the_whole_bank_calls(name, storage, T):
    b, dt_full, ref = bank_and_reference(name, storage, T)
    for rows in row_lists(T):
        for shared in (0.0, 0.25):
            assert_rows_of(b.get_pose_rows(rows, shared), ref[shared][0], rows, f"pose, shared {shared}, {rows[:6]}")
            assert_rows_of(b.get_predicted_rows(rows, shared), ref[shared][1], rows, f"predicted, shared {shared}, {rows[:6]}")
        assert_rows_of(b.get_pose_rows(rows, dt_full[rows]), ref["each"][0], rows, f"pose, per entry, {rows[:6]}")
        assert_rows_of(b.get_predicted_rows(rows, dt_full[rows]), ref["each"][1], rows, f"predicted, per entry, {rows[:6]}")
    # tags that have not started: the status word says so and the numbers are NaN
    pos, cov, vel, st = b.get_pose_rows(reset_rows(T), 0.25)
    assert np.all(st == ST_NOT_STARTED) and np.isnan(pos).all() and np.isnan(cov).all() and np.isnan(vel).all()
    x, P, st = b.get_predicted_rows(reset_rows(T), 0.25)
    assert np.all(st == ST_NOT_STARTED) and np.isnan(x).all() and np.isnan(P).all()
    # dt_ahead belongs to the entry, not to the row: a row listed twice is extrapolated twice
    twice, two_dt = np.array([7, 7], dtype=np.int32), np.array([0.0, 0.25])
    for got, k in ((b.get_pose_rows(twice, two_dt), 0), (b.get_predicted_rows(twice, two_dt), 1)):
        for g, f0, f25 in zip(got, ref[0.0][k], ref[0.25][k]):
            assert same_bits(g[0], f0[7]) and same_bits(g[1], f25[7])
    if MODELS[name][0] != ML:  # (MLLocation::getPose returns the estimate as it is, whatever the time)
        cov = b.get_pose_rows(twice, two_dt)[1]
        assert not same_bits(cov[0], cov[1])
    assert b.lib.kfpos_last_error() == b""


@pytest.mark.parametrize("name,storage,T", [pytest.param("imu9", 2, 1000, id="imu9-st2-T1000"),
                                            pytest.param("planar", 3, 100, id="planar-st3-T100")])
def test_each_output_of_the_pose_call_may_be_null(name, storage, T):
    b, dt_full, ref = bank_and_reference(name, storage, T)
    rows = row_lists(T)[0]
    d = np.ascontiguousarray(dt_full[rows])
    whole = ref["each"][0]
    for keep in range(4):
        out = [np.zeros((rows.size, 3)), np.zeros((rows.size, 9)), np.zeros((rows.size, 3)), np.zeros(rows.size, dtype=np.uint32)]
        args = [o.ctypes.data if k == keep else None for k, o in enumerate(out)]
        assert b.lib.kfpos_get_pose_rows(b._h, rows.ctypes.data, rows.size, d.ctypes.data, d.size, *args) == 0
        assert same_bits(out[keep].reshape(whole[keep][rows].shape), whole[keep][rows]), keep
    assert b.lib.kfpos_get_pose_rows(b._h, rows.ctypes.data, rows.size, d.ctypes.data, d.size, None, None, None, None) == 0


# ---------------------------------------------------------------- 2. lists longer than one staging chunk
@pytest.mark.parametrize("T,n", [(1000, 25000), (100, 4000)])
def test_lists_longer_than_one_staging_chunk(T, n):
    """25 000 entries x 736 bytes (9 + 81 doubles, dt, status, row) exceed the 16 MiB chunk of the staging area; 40 T
    entries exceed the mapped block of the 100-tag bank."""
    b, _, ref = bank_and_reference("imu9", 0, T)
    rng = np.random.default_rng(11)
    rows = rng.integers(0, T, size=n).astype(np.int32)
    late = rng.integers(0, 2, size=n).astype(bool)
    dt = np.where(late, 0.25, 0.0)
    for k, got in ((1, b.get_predicted_rows(rows, dt)), (0, b.get_pose_rows(rows, dt))):
        for g, f0, f25 in zip(got, ref[0.0][k], ref[0.25][k]):
            sel = late.reshape((n,) + (1,) * (g.ndim - 1))
            assert same_bits(g, np.where(sel, f25[rows], f0[rows]))


# ---------------------------------------------------------------- 3. the filter state is not touched
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_the_calls_leave_the_filter_state_untouched(name, storage, T):
    b, w = stepped_bank(name, storage, T)
    twin, _ = stepped_bank(name, storage, T)
    before = snapshot(b)
    for rows in row_lists(T):
        b.get_pose_rows(rows, 0.25)
        b.get_predicted_rows(rows, dt_of_rows(T)[rows])
    for p, q in zip(before, snapshot(b)):
        assert (p is None) == (q is None) and (p is None or same_bits(p, q))
    d = inputs(name, w, EPOCHS, real_of(storage))
    for sa, sb in zip(apply(b, name, EPOCHS, d), apply(twin, name, EPOCHS, d)):
        assert same_bits(sa, sb)
    for p, q in zip(snapshot(b), snapshot(twin)):
        assert (p is None) == (q is None) and (p is None or same_bits(p, q))
    b.close()
    twin.close()


# ---------------------------------------------------------------- 4. errors
@pytest.mark.parametrize("T", [100, 1000])
def test_errors_name_the_entry_and_write_nothing(T):
    b, _, _ = bank_and_reference("imu9", 0, T)
    lib, h = b.lib, b._h
    dt = np.array([0.1, 0.2, 0.3])
    out = [np.full((3, 3), 7.0), np.full((3, 9), 7.0), np.full((3, 3), 7.0), np.full(3, 7, dtype=np.uint32)]
    x, P = np.full((3, 9), 7.0), np.full((3, 81), 7.0)

    def pose(rows, n, dt_len):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_get_pose_rows(h, r.ctypes.data, n, dt.ctypes.data, dt_len, *[o.ctypes.data for o in out])

    def pred(rows, n, dt_len):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_get_predicted_rows(h, r.ctypes.data, n, dt.ctypes.data, dt_len, x.ctypes.data, P.ctypes.data,
                                            out[3].ctypes.data)

    for call, who in ((pose, "kfpos_get_pose_rows"), (pred, "kfpos_get_predicted_rows")):
        for rows, n, dt_len, named in (([1, T, 2], 3, 3, f"rows[1] = row {T} is outside"),
                                       ([4, 2, -1], 3, 1, "rows[2] = row -1 is outside"),
                                       ([4, 2, 4], 3, 2, "dt_len = 2"),
                                       ([4, 2, 4], -1, 1, "n < 0")):
            assert call(rows, n, dt_len) == ERR_ARG
            text = lib.kfpos_last_error().decode()
            assert who in text and named in text, text
        assert call([4, 2, 4], 0, 1) == 0                   # n == 0: nothing happens
        assert lib.kfpos_last_error() == b""
    r = np.array([1, 2, 3], dtype=np.int32)
    assert lib.kfpos_get_pose_rows(h, None, 3, dt.ctypes.data, 3, *[o.ctypes.data for o in out]) == ERR_ARG
    assert lib.kfpos_get_pose_rows(h, r.ctypes.data, 3, None, 1, *[o.ctypes.data for o in out]) == ERR_ARG
    assert lib.kfpos_get_predicted_rows(h, r.ctypes.data, 3, dt.ctypes.data, 3, None, P.ctypes.data, None) == ERR_ARG
    assert lib.kfpos_get_predicted_rows(h, r.ctypes.data, 3, dt.ctypes.data, 3, x.ctypes.data, None, None) == ERR_ARG
    for o in out + [x, P]:
        assert np.all(o == 7)


# ---------------------------------------------------------------- 5. streaming: a round that returns what is published
def fill_rows_round(bank, slot, name, w, s, rows, dts, real):
    d = inputs(name, w, s, real)
    n = rows.size
    v = bank.slot_acquire_rows(slot)
    v["rows"][:n] = rows
    v["range_mm"][:n] = d["r"][rows]
    v["err_est"][:n] = d["err"][rows]
    if MODELS[name][0] == IMU:
        v["accel"][:n] = d["accel"][rows]
        v["cov"][:n] = d["cov"][rows]
    v["dt"][:n] = dts
    return v, d


def sync_rows_round(bank, name, d, rows, dts):
    if MODELS[name][0] == IMU:
        return bank.step_toa_imu_rows(rows, d["r"][rows], d["err"][rows], d["accel"][rows], d["cov"][rows], dts)
    return bank.step_toa_rows(rows, d["r"][rows], d["err"][rows], dts)


STREAM = [pytest.param("toa6_fixed", 0, id="toa6-st0"), pytest.param("imu9", 0, id="imu9-st0"),
          pytest.param("toa6_mlinit", 3, id="toa6full-st3"), pytest.param("imu9", 2, id="imu9-st2")]


@pytest.mark.parametrize("name,storage", STREAM)
def test_a_flagged_round_returns_covariance_and_velocity_of_its_tags(name, storage):
    from roskfpos_amd import capi
    T, n = 1000, 37
    real = real_of(storage)
    kind = capi.SLOT_TOA_IMU if MODELS[name][0] == IMU else capi.SLOT_TOA
    b, w = stepped_bank(name, storage, T)
    twin, _ = stepped_bank(name, storage, T)
    # the last row; a tag that was reset: this round is its first epoch; the rest spread over the bank
    rows = np.concatenate([[T - 1, 3], np.random.default_rng(5).choice(np.arange(4, T - 1), size=n - 2, replace=False)]).astype(np.int32)
    dts = np.full(n, 0.05)
    dts[4] = -1.0                            # a listed tag that sits the round out
    views = []
    for bank, extra in ((b, capi.SLOT_POSE_COV), (twin, 0)):
        v, _ = fill_rows_round(bank, 0, name, w, EPOCHS, rows, dts, real)
        bank.slot_submit_rows(0, kind | capi.SLOT_DT_PER_TAG | extra, n, 0.05)
        bank.slot_wait(0)
        views.append(v)
    cov, vel = b.slot_pose_rows(0, n)
    cov, vel = cov.copy(), vel.copy()
    _, cov_sync, vel_sync, _ = b.get_pose_rows(rows, 0.0)
    assert same_bits(cov, cov_sync) and same_bits(vel, vel_sync)
    assert np.isfinite(cov[4:]).all() and np.isfinite(vel[4:]).all()   # (numbers were compared, not NaN with NaN)
    # the flag changes nothing else: status, pos and the bank are those of the round without it
    assert same_bits(views[0]["status"][:n], views[1]["status"][:n])
    assert same_bits(views[0]["pos"][:3 * n], views[1]["pos"][:3 * n])
    for p, q in zip(snapshot(b), snapshot(twin)):
        assert (p is None) == (q is None) and (p is None or same_bits(p, q))
    # the accessor belongs to flagged rounds; the flag asks for a pose
    c, v2 = ctypes.c_void_p(), ctypes.c_void_p()
    assert twin.lib.kfpos_slot_pose_rows(twin._h, 0, ctypes.byref(c), ctypes.byref(v2)) == ERR_STATE
    assert b"KFPOS_SLOT_POSE_COV" in twin.lib.kfpos_last_error()
    fill_rows_round(b, 1, name, w, EPOCHS + 1, rows, dts, real)
    assert b.lib.kfpos_slot_submit_rows(b._h, 1, kind | capi.SLOT_POSE_COV | capi.SLOT_NO_POSE, n, 0.05) == ERR_ARG
    assert b"KFPOS_SLOT_NO_POSE" in b.lib.kfpos_last_error()
    # a later round of the slot without the flag takes the arrays away again
    b.slot_submit_rows(1, kind | capi.SLOT_DT_PER_TAG, n, 0.05)
    b.slot_wait(1)
    assert b.lib.kfpos_slot_pose_rows(b._h, 1, ctypes.byref(c), ctypes.byref(v2)) == ERR_STATE
    b.close()
    twin.close()


@pytest.mark.parametrize("name,storage", STREAM[:2])
def test_flagged_rounds_in_flight_return_the_poses_of_their_own_moment(name, storage):
    from roskfpos_amd import capi
    T = 1000
    real = real_of(storage)
    imu = MODELS[name][0] == IMU
    kind = capi.SLOT_TOA_IMU if imu else capi.SLOT_TOA
    b, w = stepped_bank(name, storage, T)
    twin, _ = stepped_bank(name, storage, T)
    rng = np.random.default_rng(9)
    rows_a = rng.choice(T, size=37, replace=False).astype(np.int32)
    rows_b = np.concatenate([rows_a[:20], np.setdiff1d(np.arange(T, dtype=np.int32), rows_a)[:45]]).astype(np.int32)
    s = EPOCHS
    # streaming: flagged round A (slot 0), a whole-bank round (slot 2), flagged round B (slot 1), a whole-bank round
    # (slot 2 again: waits for the first one only) -- nothing is collected before everything is submitted
    fill_rows_round(b, 0, name, w, s, rows_a, np.full(rows_a.size, 0.05), real)
    b.slot_submit_rows(0, kind | capi.SLOT_DT_PER_TAG | capi.SLOT_POSE_COV, rows_a.size, 0.05)
    for k, (slot, rows) in enumerate(((2, None), (1, rows_b), (2, None))):
        d = inputs(name, w, s + 1 + k, real)
        if rows is None:
            v = b.slot_acquire(slot)
            v["range_mm"][:] = d["r"].T
            v["err_est"][:] = d["err"].T
            if imu:
                v["accel"][:] = d["accel"].T
                v["cov"][:] = d["cov"].T
            b.slot_submit(slot, kind | capi.SLOT_POSE_COV, 0.05)   # whole-bank rounds ignore the bit
        else:
            fill_rows_round(b, slot, name, w, s + 1 + k, rows, np.full(rows.size, 0.05), real)
            b.slot_submit_rows(slot, kind | capi.SLOT_DT_PER_TAG | capi.SLOT_POSE_COV, rows.size, 0.05)
    # the twin: the same sequence through the synchronous calls
    expect = {}
    sync_rows_round(twin, name, inputs(name, w, s, real), rows_a, np.full(rows_a.size, 0.05))
    expect[0] = twin.get_pose_rows(rows_a, 0.0)
    for k, rows in enumerate((None, rows_b, None)):
        d = inputs(name, w, s + 1 + k, real)
        if rows is None:
            if imu:
                twin.step_toa_imu(d["r"], d["err"], d["accel"], d["cov"], 0.05)
            else:
                twin.step_toa(d["r"], d["err"], 0.05)
        else:
            sync_rows_round(twin, name, d, rows, np.full(rows.size, 0.05))
            expect[1] = twin.get_pose_rows(rows, 0.0)
    for slot, rows in ((0, rows_a), (1, rows_b)):
        b.slot_wait(slot)
        cov, vel = b.slot_pose_rows(slot, rows.size)
        assert same_bits(cov, expect[slot][1]) and same_bits(vel, expect[slot][2]), slot
    assert not same_bits(expect[0][1][:20], expect[1][1][:20])     # (the two moments differ for the shared tags)
    ptr = ctypes.c_void_p()
    assert b.lib.kfpos_slot_pose_rows(b._h, 2, ctypes.byref(ptr), None) == ERR_STATE
    b.slot_wait(2)
    for p, q in zip(snapshot(b), snapshot(twin)):
        assert (p is None) == (q is None) and (p is None or same_bits(p, q))
    b.close()
    twin.close()
