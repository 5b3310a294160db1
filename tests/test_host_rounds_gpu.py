"""The host side of a round through the C ABI on the card: which route the buffers take does not show, and what a handle
answers to a kind of round it cannot take is fixed.

1. Route equality. One bank is created with KFPOS_SMALL_BANK_ELEMS=1048576 (inputs and outputs in the mapped block), its twin
with 0 (device staging); both get the same calls. Status words, every output array and get_state / get_latch / get_height are
compared as bytes, as tests/test_streaming_gpu.py::test_small_bank_mapped_block_equals_staged_path does for the ranging and
fused whole-bank calls. Here: (a) the four sensor kinds of a planar bank interleaved with ranging epochs, T = 65; (b) the four
_rows step calls, get_pose_rows and get_predicted_rows on 6-state, 9-state and planar banks of 100 tags, lists of 1, 63, 65
and 100 rows (two unsorted), dt shared and per entry, one entry with a negative dt; (c) banks of ONE tag, where dt_len = 1 is
both "shared" and "per tag", on every synchronous call and on get_predicted.

2. Return codes. T = 4 banks of each model, anchors set and not set: the four synchronous step calls, the four _rows calls
(n = 2 and n = 0) and both slot submits with the three kinds. The expected table is a literal (read off the entry points'
bodies); an empty virtual returns KFPOS_OK with its n status words zeroed. Null arguments: KFPOS_ERR_ARG."""
import ctypes as C
import os

import numpy as np
import pytest

from planar import CFG
from roskfpos_amd.synth import Workload
from test_step_rows_gpu import assert_same_bytes, calls_of, listed
from test_tag_lifecycle_gpu import IMU, ML, MODELS, PLANAR, TOA, inputs, make_bank, snapshot

pytestmark = pytest.mark.gpu


def on_both_routes(run):
    """run() with banks that take the mapped block, then with banks that stage: the two lists of arrays it returns"""
    out = []
    for limit in (1 << 20, 0):
        old = os.environ.get("KFPOS_SMALL_BANK_ELEMS")
        os.environ["KFPOS_SMALL_BANK_ELEMS"] = str(limit)  # read at kfpos_create
        try:
            out.append(run())
        finally:
            if old is None:
                os.environ.pop("KFPOS_SMALL_BANK_ELEMS")
            else:
                os.environ["KFPOS_SMALL_BANK_ELEMS"] = old
    return out


def whole_bank(bank, call, shared):
    kind, arrays, dt = call
    dts = float(dt[0]) if shared else dt
    if kind == "toa":
        return bank.step_toa(*arrays, dts)
    if kind == "imu":
        return bank.step_imu(*arrays, dts)
    if kind == "toa_imu":
        return bank.step_toa_imu(*arrays, dts)
    return bank.step_sensor(kind, arrays[0], dts)


def poses(bank, T, s):
    pos, c3, vel, pst = bank.get_pose(0.02)
    xp, Pp, xst = bank.get_predicted(np.full(T, 0.03) if s % 2 else 0.03)
    pe = bank.get_pose_each(np.linspace(0.0, 0.05, T))
    return [pos, c3, vel, pst, xp, Pp, xst, *pe]


# ---------------------------------------------------------------- 1a. planar sensors, whole bank
def test_planar_sensor_calls_on_both_routes():
    T, S = 65, 8
    w = Workload(T, 8)

    def run():
        b = make_bank("planar", 0, w)
        out = []
        for s in range(S):
            d = inputs("planar", w, s, np.float64)
            if s % 4 == 3:
                d["dt"][::5] = -1.0
            for call in calls_of("planar", s, d):  # from s = 5 on all four sensor kinds have been fed
                out.append(whole_bank(b, call, shared=len(set(call[2].tolist())) == 1))
            out += poses(b, T, s)
        out += snapshot(b)
        b.close()
        return out

    mapped, staged = on_both_routes(run)
    assert len(mapped) > S * 12
    assert_same_bytes(mapped, staged, "planar, T = 65")


# ---------------------------------------------------------------- 1b. the row-list calls
@pytest.mark.parametrize("name", ["toa6_fixed", "imu9", "planar"])
def test_rows_calls_on_both_routes(name):
    T = 100
    w = Workload(T, 8)
    rng = np.random.default_rng(3)
    lists = []
    for k, m in enumerate((65, 1, 63, T, 1, 65, 63, T)):  # 8 epochs: a planar bank gets all four sensor kinds
        rows = rng.choice(T, size=m, replace=False).astype(np.int32)
        lists.append(rows if k in (0, 2, 5) else np.sort(rows))
    assert np.any(np.diff(lists[0]) < 0) and np.any(np.diff(lists[2]) < 0)

    def run():
        b = make_bank(name, 0, w)
        out = []
        for s, rows in enumerate(lists):
            d = inputs(name, w, s, np.float64)
            each = s % 2 == 1 or rows.size == 1   # dt per entry; a list of one row: dt_len = 1 = n
            if each and rows.size > 1:
                d["dt"][rows[rows.size // 2]] = -1.0  # a listed tag that sits the call out
            for call in calls_of(name, s, d):
                out.append(listed(b, call, rows, shared_dt=not each))
            ahead = np.linspace(0.0, 0.05, rows.size) if each else 0.02
            out += list(b.get_pose_rows(rows, ahead)) + list(b.get_predicted_rows(rows, ahead))
            out += snapshot(b)
        b.close()
        return out

    mapped, staged = on_both_routes(run)
    assert_same_bytes(mapped, staged, f"{name}, row lists")


# ---------------------------------------------------------------- 1c. one tag: dt_len = 1 is shared and per tag at once
@pytest.mark.parametrize("name", ["toa6_fixed", "toa6_mlinit", "imu9", "planar", "ml"])
def test_single_tag_banks_on_both_routes(name):
    w = Workload(1, 8)
    row = np.zeros(1, dtype=np.int32)

    def run():
        b = make_bank(name, 0, w)
        out = []
        for s in range(8):
            d = inputs(name, w, s, np.float64)
            for call in calls_of(name, s, d):
                out.append(whole_bank(b, call, shared=True) if s % 2 == 0 else listed(b, call, row))
            out += poses(b, 1, s) + list(b.get_pose_rows(row, 0.02)) + list(b.get_predicted_rows(row, 0.03))
        out += snapshot(b)
        b.close()
        return out

    mapped, staged = on_both_routes(run)
    assert_same_bytes(mapped, staged, f"{name}, T = 1")


# ---------------------------------------------------------------- 2. return codes
OK, ARG, MODEL_ERR, STATE = 0, 1, 4, 5
EMPTY = "empty"  # KFPOS_OK, the call's n status words zeroed, nothing computed
SLOT_TOA, SLOT_IMU, SLOT_TOA_IMU = 0, 1, 2
MODEL_ORDER = (TOA, IMU, PLANAR, ML)
# call -> per model of MODEL_ORDER: (with anchors, without). The _rows calls with n = 2 answer as their whole-bank calls do;
# with n = 0 every one of them returns KFPOS_OK before it looks at the model.
CODES = {
    "toa": ((OK, STATE), (OK, STATE), (OK, STATE), (OK, STATE)),
    "imu": ((EMPTY, EMPTY), (OK, OK), (EMPTY, EMPTY), (EMPTY, EMPTY)),
    "sensor": ((EMPTY, EMPTY), (EMPTY, EMPTY), (OK, OK), (EMPTY, EMPTY)),
    "toa_imu": ((MODEL_ERR, MODEL_ERR), (OK, STATE), (MODEL_ERR, MODEL_ERR), (MODEL_ERR, MODEL_ERR)),
    # a slot carries no planar sensor sample: a planar bank refuses everything but ranging
    SLOT_TOA: ((OK, STATE), (OK, STATE), (OK, STATE), (OK, STATE)),
    SLOT_IMU: ((EMPTY, EMPTY), (OK, OK), (MODEL_ERR, MODEL_ERR), (EMPTY, EMPTY)),
    SLOT_TOA_IMU: ((MODEL_ERR, MODEL_ERR), (OK, STATE), (MODEL_ERR, MODEL_ERR), (MODEL_ERR, MODEL_ERR)),
}
DEAD = 0xdead


class Raw:
    """a T = 4 handle straight from kfpos_create, with or without anchors, and one set of plausible inputs"""
    T, A = 4, 8

    def __init__(self, model, anchors):
        from roskfpos_amd import capi
        self.lib = capi.load()
        w = Workload(self.T, self.A)
        cfg = capi._Config()
        cfg.model, cfg.n_tags, cfg.max_anchors, cfg.storage = model, self.T, self.A, 0
        cfg.accel_noise = cfg.jolt = cfg.cost_threshold = 0.5
        cfg.use_init_pos, cfg.init_pos = 1, (C.c_double * 3)(*w.init_positions()[0])
        self.h = C.c_void_p()
        assert self.lib.kfpos_create(C.byref(cfg), C.byref(self.h)) == OK
        if anchors:
            a = np.ascontiguousarray(w.anchors, dtype=np.float64)
            assert self.lib.kfpos_set_anchors(self.h, a.ctypes.data, None, a.shape[0]) == OK
        if model == PLANAR:
            self.planar = capi.PlanarConfig(**CFG)
            assert self.lib.kfpos_set_planar(self.h, C.byref(self.planar)) == OK
        self.r = np.ascontiguousarray(w.ranges_mm(0), dtype=np.int32)
        self.e = np.ascontiguousarray(w.err_est(np.float64))
        self.acc = np.ascontiguousarray(w.accel(0, np.float64))
        self.cov = np.ascontiguousarray(w.accel_cov(np.float64))
        self.sens = np.full((self.T, 24), 0.01)
        self.dt = np.full(self.T, 0.05)
        self.rows = np.array([3, 1], dtype=np.int32)
        self.st = np.zeros(self.T, dtype=np.uint32)

    def close(self):
        self.lib.kfpos_destroy(self.h)

    def sync(self, call, n=None, sensor=1, drop=None, h="own"):
        """the synchronous call `call`, whole-bank (n is None) or for the first n of self.rows; drop = the index of a
        pointer argument to pass as NULL"""
        L, p = self.lib, lambda a: a.ctypes.data
        inputs = {"toa": [p(self.r), p(self.e)], "imu": [p(self.acc), p(self.cov)], "sensor": [p(self.sens)],
                  "toa_imu": [p(self.r), p(self.e), p(self.acc), p(self.cov)]}[call]
        args = inputs + [p(self.dt)]
        if drop is not None:
            args[drop] = None
        args += [1, p(self.st)]
        if call == "sensor":
            args = [sensor] + args
        self.st[:] = DEAD
        hh = self.h if h == "own" else h
        if n is None:
            return getattr(L, f"kfpos_step_{call}")(hh, *args)
        return getattr(L, f"kfpos_step_{call}_rows")(hh, p(self.rows), n, *args)


def check(answer, rc, status, n, what):
    assert rc == (OK if answer == EMPTY else answer), what
    if answer == EMPTY:
        assert np.all(status[:n] == 0) and np.all(status[n:] == DEAD), what
    elif answer != OK:
        assert np.all(status == DEAD), what  # a refused call writes no status word


@pytest.mark.parametrize("anchors", [True, False], ids=["anchors", "no_anchors"])
@pytest.mark.parametrize("model", MODEL_ORDER, ids=["toa", "toa_imu", "planar", "ml"])
def test_return_codes_of_the_synchronous_calls(model, anchors):
    b = Raw(model, anchors)
    col, T = MODEL_ORDER.index(model), Raw.T
    for call in ("toa", "imu", "sensor", "toa_imu"):
        answer = CODES[call][col][0 if anchors else 1]
        for sensor in ((1, 2, 3, 4) if call == "sensor" else (0,)):
            what = f"{call} sensor {sensor}"
            check(answer, b.sync(call, sensor=sensor), b.st, T, what)
            check(answer, b.sync(call, n=2, sensor=sensor), b.st, 2, what + " rows")
            assert b.sync(call, n=0, sensor=sensor) == OK and np.all(b.st == DEAD), what + " n = 0"
        # null arguments: the handle, each input, dt; for the _rows calls also the list
        n_in = {"toa": 2, "imu": 2, "sensor": 1, "toa_imu": 4}[call]
        for n in (None, 2):
            assert b.sync(call, n=n, h=None) == ARG
            for drop in range(n_in):
                assert b.sync(call, n=n, drop=drop) == ARG, (call, n, drop)
            if answer == OK:  # dt is looked at once the round is known to run
                assert b.sync(call, n=n, drop=n_in) == ARG, (call, n, "dt")
        assert getattr(b.lib, f"kfpos_step_{call}_rows")(b.h, None, 2, *([1] if call == "sensor" else []),
                                                         *([b.r.ctypes.data] * n_in), b.dt.ctypes.data, 1, None) == ARG
    assert b.sync("sensor", sensor=0) == ARG and b.sync("sensor", sensor=5) == ARG and b.sync("sensor", n=2, sensor=9) == ARG
    b.close()


@pytest.mark.parametrize("anchors", [True, False], ids=["anchors", "no_anchors"])
@pytest.mark.parametrize("model", MODEL_ORDER, ids=["toa", "toa_imu", "planar", "ml"])
def test_return_codes_of_the_slot_submits(model, anchors):
    from roskfpos_amd import capi
    b = Raw(model, anchors)
    L, col, T = b.lib, MODEL_ORDER.index(model), Raw.T

    def view(ptr, n, dtype):
        buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
        return np.frombuffer(buf, dtype=dtype, count=n)

    assert L.kfpos_slot_submit(b.h, 0, SLOT_TOA, 0.05) == STATE        # not acquired
    assert L.kfpos_slot_submit_rows(b.h, 0, SLOT_TOA, 2, 0.05) == STATE
    for kind in (SLOT_TOA, SLOT_IMU, SLOT_TOA_IMU):
        answer = CODES[kind][col][0 if anchors else 1]
        for n in (None, 2, 0):  # whole bank, a list of two, an empty list
            sl = capi._EpochSlot() if n is None else capi._RowsSlot()
            acquire = L.kfpos_slot_acquire if n is None else L.kfpos_slot_acquire_rows
            assert acquire(b.h, 1, C.byref(sl)) == OK
            m = T if n is None else n
            view(sl.range_mm, T * b.A, np.int32)[:] = (b.r.T if n is None else b.r).ravel()
            view(sl.err_est, T * b.A, np.float64)[:] = (b.e.T if n is None else b.e).ravel()
            view(sl.accel, T * 3, np.float64)[:] = (b.acc.T if n is None else b.acc).ravel()
            view(sl.cov, T * 9, np.float64)[:] = (b.cov.T if n is None else b.cov).ravel()
            status = view(sl.status, T, np.uint32)
            status[:] = DEAD
            if n is None:
                rc = L.kfpos_slot_submit(b.h, 1, kind, 0.05)
            else:
                view(sl.rows, T, np.int32)[:2] = b.rows
                rc = L.kfpos_slot_submit_rows(b.h, 1, kind, n, 0.05)
            assert L.kfpos_slot_wait(b.h, 1) == OK
            if n == 0:
                assert rc == OK and np.all(status == DEAD), (kind, "n = 0")
            else:
                check(answer, rc, status, m, (kind, n))
                if answer == OK:
                    assert np.all(status[:m] != DEAD), (kind, n)
    # no such kind, no such slot, no handle
    sl = capi._EpochSlot()
    assert L.kfpos_slot_acquire(b.h, 2, C.byref(sl)) == OK
    assert L.kfpos_slot_submit(b.h, 2, 3, 0.05) == ARG and L.kfpos_slot_submit(b.h, 3, SLOT_TOA, 0.05) == ARG
    assert L.kfpos_slot_submit(None, 2, SLOT_TOA, 0.05) == ARG and L.kfpos_slot_acquire(b.h, 2, None) == ARG
    rs = capi._RowsSlot()
    assert L.kfpos_slot_acquire_rows(b.h, 2, C.byref(rs)) == OK and rs.capacity == T
    assert L.kfpos_slot_submit_rows(b.h, 2, 3, 0, 0.05) == ARG and L.kfpos_slot_submit_rows(b.h, -1, SLOT_TOA, 0, 0.05) == ARG
    assert L.kfpos_slot_submit_rows(None, 2, SLOT_TOA, 0, 0.05) == ARG and L.kfpos_slot_acquire_rows(b.h, 2, None) == ARG
    assert L.kfpos_slot_submit_rows(b.h, 2, SLOT_TOA, T + 1, 0.05) == ARG
    b.close()
