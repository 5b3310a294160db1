"""KFPOS_SLOT_RANGES_D16 (include/kfpos.h, include/kfpos_d16.h): whole-bank streaming rounds whose ranges travel as int16
deltas against a base plus an escape list and are rebuilt on the device (k_decode_d16). A bank fed through D16 slots is
compared, bit for bit, with a bank fed through the synchronous API: status words and poses of every epoch, the final
state. The structure is test_streaming_gpu.py::test_slot_api_equals_synchronous_api's, over 24 epochs.

Shapes (T, A): (1, 8) a lone tag, (64, 1) one anchor row, (65, 5) a partial wavefront with rows off any vector boundary,
(4099, 8) a prime row length. Inputs: Workload.ranges_mm(s) with the absences of test_streaming_gpu.py::_epoch, plus
40 000 mm where (7 t + 3 a + s) % 97 == 0 (escapes up and back down), for T = 1 a 40 000 mm jump at epoch 2 on anchor 0.
Every fifth epoch carries a per-tag dt with (t + s) % 6 == 1 silent: those tags' codes are overwritten with random int16
and a forged escape entry is planted for one of them. Every sixth epoch is a plain int32 round: the base must not move.
Half the parametrisations write the codes from Python (tests/d16.py), the other half call slot_encode_ranges.

Conditions on the inputs, asserted: every shape sees at least one escape over the run and at most a quarter of its
elements escaped in any round (counted in numpy over the twenty D16 rounds, silent tags left out: 4, 20, 109 and 12 523
escapes, largest share 12.5 %); the synchronous bank ends with every tag finite.

The lone tag's silent round (T = 1, epoch 19) makes no synchronous call: that API reads a dt array of one entry as the
shared dt, so "this tag sits the round out" cannot be said to it; the expected word is KFPOS_ST_SKIPPED and the pose stays."""
import numpy as np
import pytest

import d16
from conftest import has_gpu
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = 1, 5
SHAPES = [(1, 8), (64, 1), (65, 5), (4099, 8)]
BANKS = [(0, 1), (0, 0), (1, 2)]  # 6-state F32, 6-state F64, 9-state MIXED


def _ranges(w, s):
    T, A = w.n_tags, w.n_anchors
    r = w.ranges_mm(s)
    if s % 7 == 3:
        r[:, 1:2] = -1
    if s % 11 == 5:
        r[::3, 2:] = 0
    t, a = np.arange(T)[:, None], np.arange(A)[None, :]
    r = r + np.where((7 * t + 3 * a + s) % 97 == 0, 40000, 0).astype(np.int32)
    if T == 1 and s == 2:
        r[0, 0] += 40000
    return r


class _Pair:
    """a bank fed through the synchronous API and one fed through the slots, epoch by epoch"""

    def __init__(self, model, storage, T, A):
        from roskfpos_amd import capi
        self.capi, self.model, self.T, self.A = capi, model, T, A
        self.w = w = Workload(T, A)
        self.real = np.float64 if storage == capi.STORE_F64 else np.float32
        self.err, self.cov = w.err_est(self.real), w.accel_cov(self.real)
        self.sync = capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=w.init_positions())
        self.strm = capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=w.init_positions())
        self.NS = self.strm.lib.kfpos_slot_count(self.strm._h)
        self.rng = np.random.default_rng(T * 100 + A)
        self.pending, self.pos_sync, self.st_sync, self.pos_slot, self.st_slot = [], [], [], [], []
        self.escapes, self.mirror = [], None
        self.uploaded_err = self.uploaded_cov = False
        self.expect_restart = False   # the next slot_delta must hand out a zero base

    def close(self):
        self.sync.close()
        self.strm.close()

    def collect(self):
        slot, v = self.pending.pop(0)
        self.strm.slot_wait(slot)
        self.pos_slot.append(v["pos"].T.copy())
        self.st_slot.append(v["status"].copy())

    def drain(self):
        while self.pending:
            self.collect()

    def epoch(self, s, plain=False, encode_call=False):
        capi, T, w = self.capi, self.T, self.w
        r, dt, a = _ranges(w, s), w.dt_of(s), w.accel(s, self.real)
        per_tag = s % 5 == 4
        silent = (np.arange(T) + s) % 6 == 1
        dts = np.where(silent, -1.0, dt) if per_tag else None
        if per_tag and T == 1 and silent[0]:
            # the synchronous API reads a dt array of one entry as the shared dt: a lone tag that is silent makes no call
            st = np.array([capi.ST_SKIPPED], dtype=np.uint32)
        elif self.model == 1:
            st = self.sync.step_toa_imu(r, self.err, a, self.cov, dts if per_tag else dt)
        else:
            st = self.sync.step_toa(r, self.err, dts if per_tag else dt)
        self.st_sync.append(st)
        self.pos_sync.append(self.sync.get_pose(0.0)[0])
        slot = s % self.NS
        v = self.strm.slot_acquire(slot)
        flags = capi.SLOT_TOA_IMU if self.model == 1 else capi.SLOT_TOA
        if not self.uploaded_err or s % 4 == 0:
            v["err_est"][:] = self.err.T
            self.uploaded_err = True
        else:
            flags |= capi.SLOT_REUSE_ERR
        if self.model == 1:
            v["accel"][:] = a.T
            if not self.uploaded_cov or s % 3 == 0:
                v["cov"][:] = self.cov.T
                self.uploaded_cov = True
            else:
                flags |= capi.SLOT_REUSE_COV
        if per_tag:
            v["dt"][:] = dts
            flags |= capi.SLOT_DT_PER_TAG
        if plain:
            before = None if self.mirror is None else self.mirror.copy()
            v["range_mm"][:] = r.T
            self.strm.slot_submit(slot, flags, dt)
            assert before is None or np.array_equal(before, self.mirror), "a plain round moved the base"
        else:
            d = self.strm.slot_delta(slot)
            self.mirror = d["base"]
            if self.expect_restart:
                assert not d["base"].any() and int(d["n_esc"][0]) == 0, "the base did not restart"
                self.expect_restart = False
            if encode_call:
                v["range_mm"][:] = r.T
                self.strm.slot_encode_ranges(slot, flags & capi.SLOT_DT_PER_TAG)
            else:
                v["range_mm"][:] = 0x55555555            # not read by a D16 round
                d16.fill(d, r.T, silent if per_tag else None)
            n = int(d["n_esc"][0])
            self.escapes.append(n)
            live = r.T > 0 if not per_tag else (r.T > 0) & ~silent[None, :]
            assert np.array_equal(d["base"][live], r.T[live])
            if per_tag and silent.any():                # stale codes and a forged entry for tags that are not read
                d["code"][:, silent] = self.rng.integers(-32768, 32768, size=(self.A, int(silent.sum()))).astype(np.int16)
                t = int(np.flatnonzero(silent)[0])
                e = (self.A - 1) * T + t
                esc = d["esc"][:n].copy()
                k = int(np.searchsorted(esc[:, 0], e))
                d["esc"][:n + 1] = np.insert(esc, k, [e, 123456], axis=0)
                d["n_esc"][0] = n + 1
            self.strm.slot_submit(slot, flags | capi.SLOT_RANGES_D16, dt)
        self.pending.append((slot, v))
        if len(self.pending) == self.NS:
            self.collect()

    def compare(self):
        self.drain()
        assert len(self.pos_slot) == len(self.pos_sync)
        for s in range(len(self.pos_sync)):
            assert np.array_equal(self.st_slot[s], self.st_sync[s]), f"status words, round {s}"
            assert np.array_equal(self.pos_slot[s], self.pos_sync[s], equal_nan=True), f"poses, round {s}"
        xs, Ps, fs = self.sync.get_state()
        xt, Pt, ft = self.strm.get_state()
        assert np.array_equal(xs, xt) and np.array_equal(Ps, Pt) and np.array_equal(fs, ft)
        return xs


@pytest.mark.parametrize("T,A", SHAPES)
@pytest.mark.parametrize("model,storage", BANKS)
def test_d16_slots_equal_synchronous_api(model, storage, T, A):
    if not has_gpu():
        pytest.skip("no GPU")
    encode_call = (SHAPES.index((T, A)) + BANKS.index((model, storage))) % 2 == 1
    p = _Pair(model, storage, T, A)
    for s in range(24):
        p.epoch(s, plain=s % 6 == 5, encode_call=encode_call)
    xs = p.compare()
    # conditions on the inputs
    assert sum(p.escapes) >= 1 and max(p.escapes) <= T * A / 4, p.escapes
    assert np.isfinite(xs).all()
    p.close()


def test_d16_misuse_is_refused_and_the_base_restarts():
    """each misuse gets its error before anything is enqueued, and the next D16 round -- its base restarted at zero on both
    sides, although the refused round had moved the mirror -- is bit-identical again"""
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    T, A = 65, 5
    p = _Pair(1, capi.STORE_MIXED, T, A)
    b, lib, h = p.strm, p.strm.lib, p.strm._h
    state = {"s": 0}

    def good(n=1):
        for _ in range(n):
            p.epoch(state["s"])
            state["s"] += 1
        p.drain()

    def refused(rc, code, *needles):
        text = lib.kfpos_last_error().decode()
        assert rc == code, (rc, text)
        for n in needles:
            assert n in text, text

    def opened():
        """the slot of the next round acquired and opened, the mirror moved by a round that will never arrive"""
        slot = state["s"] % p.NS
        b.slot_acquire(slot)
        d = b.slot_delta(slot)
        d16.fill(d, _ranges(p.w, state["s"]).T + 7)
        assert d["base"].any()
        return slot, d

    def restarted():
        p.expect_restart = True
        good()
        assert not p.expect_restart

    flags = capi.SLOT_TOA_IMU | capi.SLOT_RANGES_D16
    good(3)
    # two slots open (the next round opens its slot again: a round that was never sent restarts the base)
    slot, _ = opened()
    other = (slot + 1) % p.NS
    b.slot_acquire(other)
    ds = capi._DeltaSlot()
    refused(lib.kfpos_slot_delta(h, other, capi.C.byref(ds)), ERR_STATE, f"slot {slot} is open")
    restarted()
    # the flag without kfpos_slot_delta
    slot = state["s"] % p.NS
    b.slot_acquire(slot)
    refused(lib.kfpos_slot_submit(h, slot, flags, 0.05), ERR_STATE, "kfpos_slot_delta")
    restarted()
    # the flag on a row-list round
    slot, _ = opened()
    b.slot_acquire_rows(slot)["rows"][0] = 3
    refused(lib.kfpos_slot_submit_rows(h, slot, flags, 1, 0.05), ERR_ARG, "whole-bank")
    restarted()
    # the flag on a round without ranging
    slot, _ = opened()
    refused(lib.kfpos_slot_submit(h, slot, capi.SLOT_IMU | capi.SLOT_RANGES_D16, 0.05), ERR_ARG, "KFPOS_SLOT_IMU")
    restarted()
    # the escape list: descending, out of range (either side), pointing at a code that is no ESCAPE, longer than capacity
    cases = [([(9, 5), (4, 5)], {9: d16.ESCAPE, 4: d16.ESCAPE}, None, "escape entry 1", "ascend"),
             ([(4, 5), (4, 5)], {4: d16.ESCAPE}, None, "escape entry 1", "ascend"),
             ([(A * T, 5)], {}, None, "escape entry 0", "outside"),
             ([(-1, 5)], {}, None, "escape entry 0", "outside"),
             ([(3, 5), (11, 5)], {3: d16.ESCAPE, 11: 17}, None, "escape entry 1", "not KFPOS_D16_ESCAPE"),
             ([], {}, A * T + 1, "n_esc", "capacity"),
             ([], {}, -1, "n_esc", "capacity")]
    for k, (esc, codes, n_esc, *needles) in enumerate(cases):
        slot, d = opened()
        d["code"][:] = 0
        for e, c in codes.items():
            d["code"].reshape(-1)[e] = c
        for i, pair in enumerate(esc):
            d["esc"][i] = pair
        d["n_esc"][0] = len(esc) if n_esc is None else n_esc
        refused(lib.kfpos_slot_submit(h, slot, flags, 0.05), ERR_ARG, *needles)
        # the slot is closed by the refusal: the flag again is "not opened"
        refused(lib.kfpos_slot_submit(h, slot, flags, 0.05), ERR_STATE, "kfpos_slot_delta")
        restarted()
    good(2)
    xs = p.compare()
    assert np.isfinite(xs).all()
    p.close()
