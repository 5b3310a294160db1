"""Row-list steps through the C ABI on the card: kfpos_step_*_rows(rows, n, inputs of the listed tags) computes, bit for
bit, what the whole-bank call computes with those inputs and dt < 0 for every other tag.

Two banks of one configuration run the same trace: in every epoch a seeded subset of the tags reports (sizes 1, 63, 64,
65, T - 1, T and fractions of T; sorted and unsorted; every tag sits epochs out, some report late for the first time).
Bank A gets the whole-bank calls, bank B the _rows calls. After every call the listed tags' status words, and after every
epoch get_state / get_latch / get_height of the WHOLE bank, are compared as bytes (NaN payloads count).

Models, storages and sizes are those of tests/test_tag_lifecycle_gpu.py: 100 tags x 8 anchors takes the small bank's
mapped block, 1000 x 8 the device staging; the 6-state fixed-start banks run the 8-lanes-per-tag kernel."""
import os
import subprocess
import sys

import numpy as np
import pytest

from roskfpos_amd.synth import Workload
from test_tag_lifecycle_gpu import IMU, ML, MODELS, PARAMS, PLANAR, TOA, inputs, make_bank, real_of, snapshot

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ST_NONFINITE, ST_SKIPPED = 32, 64
SENSOR_PX4FLOW, SENSOR_IMU, SENSOR_MAG, SENSOR_COMPASS = 1, 2, 3, 4


def subsets(T, seed=5):
    """The reporters of each epoch: (rows, sorted?)"""
    rng = np.random.default_rng(seed)
    sizes = [T // 2, 1, 63, 65, T, T // 3, 1, 64, 7, T - 1, 65, T // 2, T]
    out = []
    for k, m in enumerate(sizes):
        rows = rng.choice(T, size=m, replace=False).astype(np.int32)
        out.append(np.sort(rows) if k % 3 == 0 else rows)  # two in three epochs come unsorted
    quiet = np.ones(T, dtype=bool)
    for rows in out:
        if rows.size < T:
            absent = np.ones(T, dtype=bool)
            absent[rows] = False
            quiet &= ~absent
    assert not quiet.any()  # every tag sits at least one epoch out
    return out


def calls_of(name, s, d):
    """The estimator calls of epoch s as (kind, per-tag input arrays, per-tag dt): what the reference's callbacks would
    make for every tag, sensors interleaved as tests/test_tag_lifecycle_gpu.py:apply does."""
    model = MODELS[name][0]
    if model == IMU:
        if s % 3 == 0:
            return [("toa_imu", (d["r"], d["err"], d["accel"], d["cov"]), d["dt"])]
        if s % 3 == 1:  # newIMUMeasurement on its own, then the ranging epoch re-fuses the latched sample
            return [("imu", (d["accel"], d["cov"]), np.full_like(d["dt"], 0.01)), ("toa", (d["r"], d["err"]), d["dt"] - 0.01)]
        return [("toa", (d["r"], d["err"]), d["dt"])]
    if model != PLANAR:
        return [("toa", (d["r"], d["err"]), d["dt"])]
    out, dts = [], d["dt"].copy()
    T = dts.size
    if s >= 2:
        out.append((SENSOR_IMU, (np.concatenate([d["imu_w"], d["imu_cw"], d["imu_a"], d["imu_ca"]], axis=1),), np.full(T, 0.01)))
        dts = dts - 0.01
    if s >= 3:
        out.append((SENSOR_PX4FLOW, (d["px4"],), np.full(T, 0.01)))
        dts = np.where(d["px4"][:, 4] == 0, dts, dts - 0.01)
    if s >= 4 and s % 2 == 0:
        out.append((SENSOR_MAG, (d["mag"],), np.full(T, 0.005)))
        dts = dts - 0.005
    if s >= 5 and s % 2 == 1:
        out.append((SENSOR_COMPASS, (np.asarray(d["compass"]).reshape(T, 1),), np.full(T, 0.005)))
        dts = dts - 0.005
    out.append(("toa", (d["r"], d["err"]), dts))
    return out


def dense(bank, call, rows):
    """the whole-bank call, dt < 0 for everyone who is not listed; the listed tags' status words"""
    kind, arrays, dt = call
    dts = np.full(bank.T, -1.0)
    dts[rows] = dt[rows]
    if kind == "toa":
        st = bank.step_toa(*arrays, dts)
    elif kind == "imu":
        st = bank.step_imu(*arrays, dts)
    elif kind == "toa_imu":
        st = bank.step_toa_imu(*arrays, dts)
    else:
        st = bank.step_sensor(kind, arrays[0], dts)
    others = np.setdiff1d(np.arange(bank.T), rows)
    assert np.all(st[others] == ST_SKIPPED)
    return st[rows]


def listed(bank, call, rows, shared_dt=False):
    kind, arrays, dt = call
    part = [a[rows] for a in arrays]
    dts = dt[rows[0]] if shared_dt else dt[rows]
    if kind == "toa":
        return bank.step_toa_rows(rows, *part, dts)
    if kind == "imu":
        return bank.step_imu_rows(rows, *part, dts)
    if kind == "toa_imu":
        return bank.step_toa_imu_rows(rows, *part, dts)
    return bank.step_sensor_rows(rows, kind, part[0], dts)


def assert_same_bytes(a, b, what=""):
    for k, (p, q) in enumerate(zip(a, b)):
        assert (p is None) == (q is None), (what, k)
        if p is not None:
            assert p.shape == q.shape and p.dtype == q.dtype, (what, k)
            same = np.ascontiguousarray(p).view(np.uint8) == np.ascontiguousarray(q).view(np.uint8)
            assert same.all(), f"{what}: part {k} differs in {int((~same).sum())} bytes"


def run_pair(name, storage, T, w, a, b, epochs=None, first=0):
    """Banks a (whole-bank calls) and b (_rows calls) through the trace; compared after every call and epoch."""
    real = real_of(storage)
    for k, rows in enumerate(epochs if epochs is not None else subsets(T)):
        s = first + k
        d = inputs(name, w, s, real)
        if k % 4 == 3:  # a listed tag may still sit the call out: negative dt[i]
            d["dt"][rows[::5]] = -1.0
        for c, call in enumerate(calls_of(name, s, d)):
            sa = dense(a, call, rows)
            # a shared dt (dt_len = 1) where the call's dt is the same for every listed tag
            shared = len(set(call[2][rows].tolist())) == 1
            sb = listed(b, call, rows, shared_dt=shared)
            assert sb.shape == (rows.size,)
            np.testing.assert_array_equal(sb, sa, err_msg=f"status words, epoch {s} call {c} ({rows.size} rows)")
        assert_same_bytes(snapshot(a), snapshot(b), f"epoch {s} ({rows.size} rows)")


# ---------------------------------------------------------------- 1. the matrix
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_rows_calls_equal_the_whole_bank_calls(name, storage, T):
    w = Workload(T, 8)
    a, b = make_bank(name, storage, w), make_bank(name, storage, w)
    run_pair(name, storage, T, w, a, b)
    assert b.lib.kfpos_last_error() == b""
    x = snapshot(b)[0]
    assert np.isfinite(x[:, :2]).all()  # the trace is a healthy one: every tag ends up with a finite estimate


# ---------------------------------------------------------------- 2. the two-wave build, n small
def test_two_wave_bank_with_short_lists():
    """More wavefronts than SIMDs: the handle runs k_step_toa6_w2 whatever n is."""
    T = 65536 + 4096 + 37
    w = Workload(T, 8)
    a, b = make_bank("toa6_fixed", 2, w), make_bank("toa6_fixed", 2, w)
    rng = np.random.default_rng(11)
    epochs = [rng.choice(T, size=m, replace=False).astype(np.int32) for m in (T // 2, 1, 65, 1000, 63)]
    real = real_of(2)
    for s, rows in enumerate(epochs):
        d = inputs("toa6_fixed", w, s, real)
        call = ("toa", (d["r"], d["err"]), d["dt"])
        np.testing.assert_array_equal(listed(b, call, rows), dense(a, call, rows))
        assert_same_bytes(snapshot(a), snapshot(b), f"epoch {s}")


# ---------------------------------------------------------------- 3. the run-time-loop kernels
def _generic_child():
    for name, storage, T in (("toa6_fixed", 0, 1000), ("toa6_mlinit", 3, 100), ("imu9", 2, 1000)):
        w = Workload(T, 8)
        a, b = make_bank(name, storage, w), make_bank(name, storage, w)
        run_pair(name, storage, T, w, a, b)
    print("GENERIC OK")


def test_generic_kernels_in_a_child_process():
    env = dict(os.environ, KFPOS_GENERIC_KERNEL="1")
    env["PYTHONPATH"] = os.pathsep.join([ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")] + [p for p in [env.get("PYTHONPATH")] if p])
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "generic"], env=env, capture_output=True, text=True,
                         timeout=600)
    print(out.stdout[-2000:], out.stderr[-2000:])
    assert out.returncode == 0 and "GENERIC OK" in out.stdout


# ---------------------------------------------------------------- 4. P48 with a non-finite tag
@pytest.mark.parametrize("name", ["toa6_fixed", "imu9"])
def test_p48_with_a_non_finite_tag(name):
    T = 1000
    w = Workload(T, 8)
    a, b = make_bank(name, 3, w), make_bank(name, 3, w)
    eps = subsets(T)
    run_pair(name, 3, T, w, a, b, epochs=eps[:4])
    sick = int(eps[4][0])  # the tag reports in the epoch that follows
    for bank in (a, b):
        x1, P1, _, _, _ = bank.get_tags([sick])
        x1[0, 1] = np.nan
        P1[:] = np.nan
        bank.set_tags([sick], x=x1, P=P1)
    real = real_of(3)
    d = inputs(name, w, 4, real)
    call = ("toa", (d["r"], d["err"]), d["dt"])
    sa, sb = dense(a, call, eps[4]), listed(b, call, eps[4])
    np.testing.assert_array_equal(sb, sa)
    assert sb[0] & ST_NONFINITE and not np.any(sb[1:] & ST_NONFINITE)
    assert_same_bytes(snapshot(a), snapshot(b), "the epoch that made the tag non-finite")
    run_pair(name, 3, T, w, a, b, epochs=eps[5:], first=5)


# ---------------------------------------------------------------- 5. errors write nothing
@pytest.mark.parametrize("T", (100, 1000))
def test_errors_are_reported_before_anything_is_written(T):
    from roskfpos_amd import capi
    w = Workload(T, 8)
    b = capi.KfposBank(IMU, T, w.anchors, init_pos=w.init_positions())
    for s in range(3):
        b.step_toa_imu(w.ranges_mm(s), w.err_est(), w.accel(s), w.accel_cov(), w.dt_of(s))
    before = snapshot(b)
    lib, h = b.lib, b._h
    r_in = np.full((8, 8), 4000, dtype=np.int32)
    e_in = np.full((8, 8), 0.0025)
    acc, cov = np.full((8, 3), 7.0), np.tile(np.eye(3).ravel(), (8, 1))
    dt = np.full(8, 0.05)
    st = np.full(8, 0xdead, dtype=np.uint32)

    def toa(rows, n=None):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_step_toa_rows(h, r.ctypes.data, r.size if n is None else n, r_in.ctypes.data, e_in.ctypes.data,
                                       dt.ctypes.data, 1, st.ctypes.data)

    def imu(rows, n=None):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_step_imu_rows(h, r.ctypes.data, r.size if n is None else n, acc.ctypes.data, cov.ctypes.data,
                                       dt.ctypes.data, 1, st.ctypes.data)

    def fused(rows, n=None):
        r = np.array(rows, dtype=np.int32)
        return lib.kfpos_step_toa_imu_rows(h, r.ctypes.data, r.size if n is None else n, r_in.ctypes.data,
                                           e_in.ctypes.data, acc.ctypes.data, cov.ctypes.data, dt.ctypes.data, 1,
                                           st.ctypes.data)

    ARG, MODEL_ERR = 1, 4
    for call in (toa, imu, fused):
        for rows, named in (([1, T, 2], str(T)), ([0, 3, -1], "-1")):  # a row out of range
            assert call(rows) == ARG
            text = lib.kfpos_last_error().decode()
            assert named in text and "outside" in text
        assert call([5, 2, 5]) == ARG                                   # a duplicate
        text = lib.kfpos_last_error().decode()
        assert "rows[2]" in text and "twice" in text
        assert call([4, T, 2, 4]) == ARG                                # the FIRST offender, whichever rule it breaks
        assert "rows[1]" in lib.kfpos_last_error().decode()
        assert call([7, 3, 9, 3, 7, 3]) == ARG
        assert "rows[3]" in lib.kfpos_last_error().decode()
        assert call([1, 2], n=-1) == ARG                                # n < 0
    assert lib.kfpos_step_toa_rows(h, None, 2, r_in.ctypes.data, e_in.ctypes.data, dt.ctypes.data, 1, None) == ARG  # rows == NULL
    assert lib.kfpos_step_toa_rows(h, None, 0, None, None, None, 1, None) == 0   # n == 0: nothing happens
    r2 = np.array([1, 2], dtype=np.int32)
    assert lib.kfpos_step_toa_rows(h, r2.ctypes.data, 2, r_in.ctypes.data, e_in.ctypes.data, dt.ctypes.data, 3, None) == ARG  # dt_len
    assert lib.kfpos_step_toa_rows(h, r2.ctypes.data, 2, None, e_in.ctypes.data, dt.ctypes.data, 1, None) == ARG
    assert lib.kfpos_step_sensor_rows(h, r2.ctypes.data, 2, 9, acc.ctypes.data, dt.ctypes.data, 1, None) == ARG   # no such sensor
    # the reference's empty virtual: a sensor sample on a handle that is not planar
    assert lib.kfpos_step_sensor_rows(h, r2.ctypes.data, 2, SENSOR_COMPASS, acc.ctypes.data, dt.ctypes.data, 1, st.ctypes.data) == 0
    assert np.all(st[:2] == 0) and np.all(st[2:] == 0xdead)
    assert_same_bytes(snapshot(b), before, "after the refused calls")
    # model rules of the whole-bank calls: a 6-state handle ignores IMU samples and refuses the fused call
    m = capi.KfposBank(TOA, T, w.anchors, init_pos=w.init_positions())
    m.step_toa(w.ranges_mm(0), w.err_est(), 0.1)
    before = snapshot(m)
    st[:] = 0xdead
    assert m.lib.kfpos_step_imu_rows(m._h, r2.ctypes.data, 2, acc.ctypes.data, cov.ctypes.data, dt.ctypes.data, 1, st.ctypes.data) == 0
    assert np.all(st[:2] == 0) and np.all(st[2:] == 0xdead)
    assert m.lib.kfpos_step_toa_imu_rows(m._h, r2.ctypes.data, 2, r_in.ctypes.data, e_in.ctypes.data, acc.ctypes.data,
                                         cov.ctypes.data, dt.ctypes.data, 1, None) == MODEL_ERR
    with pytest.raises(capi.KfposError):
        m.step_toa_rows([3, 3], r_in[:2], e_in[:2], 0.05)
    assert_same_bytes(snapshot(m), before, "after the refused calls (6-state)")


# ---------------------------------------------------------------- 6. a fresh handle: the call counts as a step
def test_rows_call_counts_as_a_step():
    from roskfpos_amd import capi
    T = 100
    w = Workload(T, 8)
    b = capi.KfposBank(TOA, T, w.anchors, init_pos=w.init_positions())
    rows = np.array([3, 1], dtype=np.int32)
    b.step_toa_rows(rows, w.ranges_mm(0)[rows], w.err_est()[rows], 0.1)
    assert b.lib.kfpos_set_init_positions(b._h, w.init_positions().ctypes.data) == 5  # KFPOS_ERR_STATE: it has stepped
    fl = b.get_state()[2]
    assert np.all(fl[rows] == 1) and fl.sum() == 2


if __name__ == "__main__" and sys.argv[1:] == ["generic"]:
    _generic_child()
