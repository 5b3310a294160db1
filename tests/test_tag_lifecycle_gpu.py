"""Per-tag lifecycle through the C ABI on the card: kfpos_get_tags / kfpos_set_tags / kfpos_reset_tags read, write and
re-initialise CHOSEN rows of a bank, bit for bit what the whole-bank accessors / a fresh handle give for those rows.

Two bank sizes so that both staging paths run: 100 tags x 8 anchors (the small bank's mapped block) and 1000 x 8 (the
device staging area; not a multiple of the wavefront). The 6-state fixed-start banks are created with the library's
defaults, i.e. they run the 8-lanes-per-tag kernel."""
import numpy as np
import pytest

from planar import CFG
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

TOA, IMU, ML, PLANAR = 0, 1, 2, 3
ST_ML_INIT, ST_NOT_STARTED, ST_NONFINITE = 8, 16, 32

# name -> (model, fixed start, storages the existing GPU tests run that model in: tests/test_fused_matrix_gpu.py runs
# every model, the planar filter and the ML estimator included, in all four)
MODELS = {
    "toa6_fixed": (TOA, True, (0, 1, 2, 3)),
    "toa6_mlinit": (TOA, False, (0, 1, 2, 3)),
    "imu9": (IMU, True, (0, 1, 2, 3)),
    "planar": (PLANAR, True, (0, 1, 2, 3)),
    "ml": (ML, True, (0, 1, 2, 3)),
}
SIZES = (100, 1000)
PARAMS = [pytest.param(name, st, T, id=f"{name}-st{st}-T{T}")
          for name, (_, _, sts) in MODELS.items() for st in sts for T in SIZES]


def row_lists(T):
    """row 0, row T - 1, an unsorted order; and a list of a single row"""
    return [np.array([T - 1, 5, 0, T // 2, 17, 3], dtype=np.int32), np.array([T // 3], dtype=np.int32)]


def real_of(storage):
    return np.float64 if storage == 0 else np.float32


def make_bank(name, storage, w, init="default"):
    from roskfpos_amd import capi
    model, fixed, _ = MODELS[name]
    if isinstance(init, str):
        init = w.init_positions() if fixed else None
    return capi.KfposBank(model, w.n_tags, w.anchors, storage=storage, init_pos=init,
                          planar=CFG if model == PLANAR else None)


def inputs(name, w, s, real):
    """Everything epoch s feeds, as per-tag arrays (so that rows of two workloads can be mixed)."""
    model = MODELS[name][0]
    T = w.n_tags
    d = {"r": w.ranges_mm(s), "err": w.err_est(real), "dt": np.full(T, w.dt_of(s))}
    if model == IMU:
        d["accel"] = w.accel(s, real)
        cov = w.accel_cov(real)
        cov[:, 1] = cov[:, 3] = 0.002  # a full covariance: all six stored entries matter
        d["cov"] = cov
    if model == PLANAR:  # all four sensors, interleaved as tests/planar.py:run_trace does
        wv, la = w.planar_imu(s)
        ca = w.accel_cov()
        ca[:, 1] = ca[:, 3] = 0.002
        d.update(imu_w=wv, imu_cw=np.tile(np.eye(3).ravel() * 1e-4, (T, 1)), imu_a=la, imu_ca=ca,
                 px4=w.px4flow(s), mag=w.mag(s), compass=w.compass(s))
    return d


def mix(base, other, rows_base, rows_other):
    """`base` with rows rows_base replaced by rows rows_other of `other`"""
    out = {}
    for k, v in base.items():
        v = v.copy()
        v[rows_base] = other[k][rows_other]
        out[k] = v
    return out


def apply(bank, name, s, d):
    """One epoch of the trace: the list of status arrays of its calls."""
    model = MODELS[name][0]
    if model == IMU:
        if s % 3 == 0:
            return [bank.step_toa_imu(d["r"], d["err"], d["accel"], d["cov"], d["dt"])]
        return [bank.step_toa(d["r"], d["err"], d["dt"])]  # re-fuses the latched sample
    if model != PLANAR:
        return [bank.step_toa(d["r"], d["err"], d["dt"])]
    out, dts = [], d["dt"].copy()
    if s >= 2:
        out.append(bank.step_planar_imu(d["imu_w"], d["imu_cw"], d["imu_a"], d["imu_ca"], 0.01))
        dts = dts - 0.01
    if s >= 3:
        out.append(bank.step_px4flow(d["px4"], 0.01))
        dts = np.where(d["px4"][:, 4] == 0, dts, dts - 0.01)
    if s >= 4 and s % 2 == 0:
        out.append(bank.step_mag(d["mag"], 0.005))
        dts = dts - 0.005
    if s >= 5 and s % 2 == 1:
        out.append(bank.step_compass(d["compass"], 0.005))
        dts = dts - 0.005
    out.append(bank.step_toa(d["r"], d["err"], dts))
    return out


def snapshot(bank, rows=None):
    """(x, P, flags, latch, height) of the whole bank through the whole-bank accessors, optionally rows of it"""
    from roskfpos_amd import capi
    x, P, fl = bank.get_state()
    parts = [x, P, fl, bank.get_latch(), bank.get_height() if bank.model == capi.MODEL_PLANAR else None]
    if rows is not None:
        parts = [None if p is None else p[rows] for p in parts]
    return parts


def assert_same(a, b, what=""):
    for k, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), (what, k)
        if p is not None:
            np.testing.assert_array_equal(p, q, err_msg=f"{what} part {k}")  # NaN-aware


# ---------------------------------------------------------------- 1. get = rows of the full accessors
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_get_tags_equals_rows_of_the_full_accessors(name, storage, T):
    w = Workload(T, 8)
    real = real_of(storage)
    b = make_bank(name, storage, w)
    for s in range(20):
        apply(b, name, s, inputs(name, w, s, real))
    full = snapshot(b)
    for rows in row_lists(T) + [np.array([4, 4, T - 1, 4], dtype=np.int32)]:  # get may repeat rows
        assert_same(b.get_tags(rows), [None if p is None else p[rows] for p in full], f"rows {rows}")
    # parts that are not asked for are not touched (every output may be NULL)
    rows = row_lists(T)[0]
    fl = np.zeros(rows.size, dtype=np.uint32)
    assert b.lib.kfpos_get_tags(b._h, rows.ctypes.data, rows.size, None, None, fl.ctypes.data, None, None) == 0
    np.testing.assert_array_equal(fl, full[2][rows])
    assert b.lib.kfpos_last_error() == b""


# ---------------------------------------------------------------- 2. set = migration
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_set_tags_migrates_tags_between_banks(name, storage, T):
    real = real_of(storage)
    wa, wb = Workload(T, 8), Workload(T, 8, seed=777)
    a, b, twin = make_bank(name, storage, wa), make_bank(name, storage, wb), make_bank(name, storage, wb)
    for s in range(20):
        apply(a, name, s, inputs(name, wa, s, real))
        db = inputs(name, wb, s, real)
        apply(b, name, s, db)
        apply(twin, name, s, db)
    rows_a = row_lists(T)[0]
    rows_b = np.array([1, T - 1, T // 2 + 3, 0, 9, 64 % T], dtype=np.int32)
    others = np.setdiff1d(np.arange(T), rows_b)
    x, P, fl, latch, z = a.get_tags(rows_a)
    b.set_tags(rows_b, x, P, fl, latch, z)
    assert_same(snapshot(b, rows_b), snapshot(a, rows_a), "right after the move")
    for s in range(20, 30):
        da, db = inputs(name, wa, s, real), inputs(name, wb, s, real)
        sa = apply(a, name, s, da)
        sb = apply(b, name, s, mix(db, da, rows_b, rows_a))
        st = apply(twin, name, s, db)
        for ka, kb, kt in zip(sa, sb, st):
            np.testing.assert_array_equal(kb[rows_b], ka[rows_a])
            np.testing.assert_array_equal(kb[others], kt[others])
        assert_same(snapshot(b, rows_b), snapshot(a, rows_a), f"moved tags, epoch {s}")
    assert_same(snapshot(b, others), snapshot(twin, others), "the rows that were not written")
    # a part left out stays as it is: only the flags words of one row
    before = snapshot(b)
    b.set_tags(rows_b[:1], flags=np.array([before[2][rows_b[0]]], dtype=np.uint32))
    assert_same(snapshot(b), before, "flags-only set of the same word")


# ---------------------------------------------------------------- 3. reset = fresh handle
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_reset_tags_equals_a_fresh_handle(name, storage, T):
    from roskfpos_amd import capi
    model, fixed, _ = MODELS[name]
    real = real_of(storage)
    w = Workload(T, 8)
    a, twin = make_bank(name, storage, w), make_bank(name, storage, w)
    for s in range(20):
        d = inputs(name, w, s, real)
        apply(a, name, s, d)
        apply(twin, name, s, d)
    rows = row_lists(T)[0]
    others = np.setdiff1d(np.arange(T), rows)
    sick = int(rows[1])
    if model != ML:  # (the standalone ML estimator has no ST_NONFINITE: its kernel reports the solver's flags only)
        # a tag driven non-finite: the status word says so, and only a reset cures it
        # (NaN in y and in the whole covariance: a single NaN covariance entry is washed out by the ML-start kernel's
        # update, and a NaN x alone would send an ML-start tag back to its initialisation)
        x1, P1, _, _, _ = a.get_tags([sick])
        x1[0, 1] = np.nan
        P1[:] = np.nan
        a.set_tags([sick], x=x1, P=P1)
        st = apply(a, name, 20, inputs(name, w, 20, real))[-1]
        apply(twin, name, 20, inputs(name, w, 20, real))
        assert st[sick] & ST_NONFINITE
        assert not np.any(st[others] & ST_NONFINITE)
    else:
        # the standalone ML estimator: its one piece of per-tag state besides the estimate is the solver's seed (the
        # latch). Poisoned with NaN the tag no longer follows its twin; a reset gives it a seed again (checked below:
        # it solves like the same row of a fresh handle, finitely)
        a.set_tags([sick], latch=np.full((1, 3), np.nan))
        assert np.all(np.isnan(a.get_tags([sick])[3]))
        apply(a, name, 20, inputs(name, w, 20, real))
        apply(twin, name, 20, inputs(name, w, 20, real))
        assert not np.array_equal(a.get_tags([sick])[0], twin.get_tags([sick])[0])
        np.testing.assert_array_equal(a.get_tags(others)[0], twin.get_tags(others)[0])
    init_rows = w.position(w.time_of(21))[rows] + 0.01 if fixed else None
    a.reset_tags(rows, init_rows)
    init_c = None
    if fixed:
        init_c = w.init_positions()
        init_c[rows] = init_rows
    c = make_bank(name, storage, w, init=init_c)
    if model == PLANAR:
        # which instantiation serves ranging epochs is a property of the HANDLE (has it ever seen a sensor sample), not of
        # a tag: give the fresh handle one sensor call on a row that is not compared, so that both run the same kernel
        dts = np.full(T, -1.0)
        dts[others[0]] = 0.01
        c.step_compass(w.compass(0), dts)
    fresh = snapshot(c, rows)
    assert_same(snapshot(a, rows), fresh, "right after the reset")
    assert np.all(fresh[2] == 0) and np.all(fresh[1] == 0)
    assert np.all(a.get_pose(0.0)[3][rows] == ST_NOT_STARTED)
    for s in range(21, 33):
        d = inputs(name, w, s, real)
        sa, sc, st = apply(a, name, s, d), apply(c, name, s, d), apply(twin, name, s, d)
        for ka, kc, kt in zip(sa, sc, st):
            np.testing.assert_array_equal(ka[rows], kc[rows])
            np.testing.assert_array_equal(ka[others], kt[others])
        if s == 21 and not fixed:
            assert np.all(sa[-1][rows] & ST_ML_INIT)
        assert not np.any(sa[-1][rows] & ST_NONFINITE)
        assert_same(snapshot(a, rows), snapshot(c, rows), f"reset tags, epoch {s}")
    assert np.all(np.isfinite(snapshot(a, rows)[0])) and np.all(np.isfinite(snapshot(a, rows)[3]))
    assert_same(snapshot(a, others), snapshot(twin, others), "the rows that were not listed")
    # the shared start position of the configuration when none is given
    if fixed and model != PLANAR:
        shared = np.array([1.0, 2.0, 0.5])
        e = capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=shared)
        apply(e, name, 0, inputs(name, w, 0, real))
        e.reset_tags(row_lists(T)[1])
        f = capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=shared)
        assert_same(snapshot(e, row_lists(T)[1]), snapshot(f, row_lists(T)[1]), "reset to kfpos_config.init_pos")


# ---------------------------------------------------------------- 4. reset against the oracle
@pytest.mark.parametrize("model,fixed", [(TOA, True), (TOA, False), (IMU, True)],
                         ids=["toa6_fixed", "toa6_mlinit", "imu9"])
def test_reset_tags_restart_matches_the_oracle(model, fixed):
    """The Workload(T, 8) trace, F64. At step k = 20 a third of the tags is reset (to the true position of that moment,
    or to NaN = ML start); an oracle bank over just those tags starts at step k with the same dt values. 30 more
    epochs: identical status words, position RMS <= 1e-9 m, maximum <= 1e-8 m (the bound tests/test_gpu_parity.py holds
    these models to on this trace), over every reset tag, none left out."""
    from roskfpos_amd import capi
    import oracle_py
    T, K, S = 192, 20, 30
    w = Workload(T, 8)
    err, cov = w.err_est(), w.accel_cov()
    gpu = capi.KfposBank(model, T, w.anchors, init_pos=w.init_positions() if fixed else None)

    def gpu_epoch(s):
        if model == IMU:
            return gpu.step_toa_imu(w.ranges_mm(s), err, w.accel(s), cov, w.dt_of(s))
        return gpu.step_toa(w.ranges_mm(s), err, w.dt_of(s))

    for s in range(K):
        gpu_epoch(s)
    rows = np.arange(0, T, 3, dtype=np.int32)
    init = w.position(w.time_of(K))[rows] if fixed else None
    gpu.reset_tags(rows, init)
    orc = oracle_py.OracleBank(model, rows.size, w.anchors, init_pos=init, n_threads=4)
    sq, mx = 0.0, 0.0
    for s in range(K, K + S):
        sg = gpu_epoch(s)
        if model == IMU:
            orc.step_imu(w.accel(s)[rows], cov[rows], 0.0)
        so = orc.step_toa(w.ranges_mm(s)[rows], err[rows], w.dt_of(s))
        np.testing.assert_array_equal(sg[rows], so)
        pg = gpu.get_tags(rows)[0][:, :3]
        po = orc.get_state()[0][:, :3]
        assert np.all(np.isfinite(pg)) and np.all(np.isfinite(po))  # every reset tag counts
        sq += ((pg - po) ** 2).sum()
        mx = max(mx, float(np.abs(pg - po).max()))
    rms = float(np.sqrt(sq / (rows.size * S)))
    print(f"reset restart vs oracle: model {model} fixed {fixed}: rms {rms:.3e} m, max {mx:.3e} m")
    assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)


# ---------------------------------------------------------------- 5. slots in flight
@pytest.mark.parametrize("T", SIZES)
def test_reset_tags_waits_for_the_slots_in_flight(T):
    from roskfpos_amd import capi
    w = Workload(T, 8)
    rows = row_lists(T)[0]
    init = w.position(0.3)[rows]
    out = []
    for wait_first in (True, False):
        b = capi.KfposBank(TOA, T, w.anchors, init_pos=w.init_positions())
        for s in range(2):
            v = b.slot_acquire(s)
            v["range_mm"][:] = w.ranges_mm(s).T
            v["err_est"][:] = w.err_est().T
            b.slot_submit(s, capi.SLOT_TOA, w.dt_of(s))
        if wait_first:
            b.slot_wait(0)
            b.slot_wait(1)
        b.reset_tags(rows, init)
        out.append(snapshot(b))
    assert_same(out[0], out[1])
    assert np.all(out[0][2][rows] == 0) and np.all(out[0][2][np.setdiff1d(np.arange(T), rows)] == 1)
    np.testing.assert_array_equal(out[0][0][rows, :3], init)


# ---------------------------------------------------------------- 6. errors write nothing
@pytest.mark.parametrize("T", SIZES)
def test_errors_are_reported_before_anything_is_written(T):
    from roskfpos_amd import capi
    w = Workload(T, 8)
    b = capi.KfposBank(IMU, T, w.anchors, init_pos=w.init_positions())
    for s in range(3):
        b.step_toa_imu(w.ranges_mm(s), w.err_est(), w.accel(s), w.accel_cov(), w.dt_of(s))
    before = snapshot(b)
    lib, h = b.lib, b._h
    n, L = b.n, 12
    junk = dict(x=np.full((3, n), 7.0), P=np.full((3, n, n), 7.0), fl=np.full(3, 9, dtype=np.uint32),
                latch=np.full((3, L), 7.0), z=np.full(3, 7.0), init=np.full((3, 3), 7.0))

    def set_tags(rows, height=False):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_set_tags(h, r.ctypes.data, r.size, junk["x"].ctypes.data, junk["P"].ctypes.data,
                                  junk["fl"].ctypes.data, junk["latch"].ctypes.data,
                                  junk["z"].ctypes.data if height else None)

    def get_tags(rows, height=False):
        r = np.array(rows, dtype=np.int32)
        x, P = np.zeros((r.size, n)), np.zeros((r.size, n, n))
        z = np.zeros(r.size)
        return lib.kfpos_get_tags(h, r.ctypes.data, r.size, x.ctypes.data, P.ctypes.data, None, None,
                                  z.ctypes.data if height else None)

    def reset_tags(rows):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_reset_tags(h, r.ctypes.data, r.size, junk["init"].ctypes.data)

    ARG, MODEL_ERR, STATE = 1, 4, 5
    for call in (set_tags, get_tags, reset_tags):
        for rows, named in (([1, T, 2], str(T)), ([0, 3, -1], "-1")):
            assert call(rows) == ARG
            assert named in lib.kfpos_last_error().decode()
    r1 = np.array([1], dtype=np.int32)
    for call in (set_tags, reset_tags):
        assert call([5, 2, 5]) == ARG
        text = lib.kfpos_last_error().decode()
        assert "5" in text and "twice" in text
    for call in (set_tags, reset_tags):                              # the FIRST offending entry, whichever rule it breaks
        assert call([4, 4, 2, 3, 1, T]) == ARG
        text = lib.kfpos_last_error().decode()
        assert "rows[1]" in text and "twice" in text
        assert call([4, T, 2, 4]) == ARG
        text = lib.kfpos_last_error().decode()
        assert "rows[1]" in text and "outside" in text
        assert call([7, 3, 9, 3, 7, 3]) == ARG
        assert "rows[3]" in lib.kfpos_last_error().decode()
    assert get_tags([5, 2, 5]) == 0                                  # get may repeat rows
    assert set_tags([1, 2, 3], height=True) == MODEL_ERR             # height on a handle that is not planar
    assert get_tags([1, 2, 3], height=True) == MODEL_ERR
    assert lib.kfpos_set_tags(h, None, 2, None, None, None, None, None) == ARG       # rows == NULL with n > 0
    assert lib.kfpos_reset_tags(h, r1.ctypes.data, -1, None) == ARG                  # n < 0
    for fn in (lambda: lib.kfpos_set_tags(h, None, 0, None, None, None, None, None),
               lambda: lib.kfpos_get_tags(h, None, 0, None, None, None, None, None),
               lambda: lib.kfpos_reset_tags(h, None, 0, None)):
        assert fn() == 0                                             # n = 0 succeeds and does nothing
    assert_same(snapshot(b), before, "after the refused calls")
    # init_xyz on a handle that starts by ML initialisation; height on a 6-state handle
    m = capi.KfposBank(TOA, T, w.anchors, init_pos=None)
    m.step_toa(w.ranges_mm(0), w.err_est(), 0.1)
    before = snapshot(m)
    r = np.array([0, 1, 2], dtype=np.int32)
    assert m.lib.kfpos_reset_tags(m._h, r.ctypes.data, 3, junk["init"].ctypes.data) == STATE
    assert "init_xyz" in m.lib.kfpos_last_error().decode()
    assert m.lib.kfpos_set_tags(m._h, r.ctypes.data, 3, None, None, None, None, junk["z"].ctypes.data) == MODEL_ERR
    with pytest.raises(capi.KfposError):
        m.reset_tags(r, np.zeros(3))
    assert_same(snapshot(m), before, "after the refused calls (ML start)")


# ---------------------------------------------------------------- 7. cost follows n, not T
def test_cost_follows_the_list_not_the_bank():
    """1 048 576 tags, 6-state, F64: the full accessor moves 16 384 times the bytes of a 64-row get_tags and is unchanged
    code; an implementation that does not copy the bank is orders of magnitude inside the tenth asked for here."""
    import time
    from roskfpos_amd import capi
    T = 1 << 20
    w = Workload(T, 8)
    b = capi.KfposBank(TOA, T, w.anchors, init_pos=w.init_positions())
    b.step_toa(w.ranges_mm(0), w.err_est(), 0.1)
    rows = (np.arange(64, dtype=np.int64) * 16411 % T).astype(np.int32)
    b.get_tags(rows)  # warm-up: staging area, code object
    t = []
    for _ in range(20):
        t0 = time.perf_counter()
        part = b.get_tags(rows)
        t.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    x, P, fl = b.get_state()
    full = time.perf_counter() - t0
    med = float(np.median(t))
    print(f"get_tags(64 rows): median {med * 1e6:.1f} us; get_state() of {T} tags: {full * 1e3:.1f} ms")
    np.testing.assert_array_equal(part[0], x[rows])
    np.testing.assert_array_equal(part[1], P[rows])
    np.testing.assert_array_equal(part[2], fl[rows])
    assert med < full / 10
