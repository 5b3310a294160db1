"""Row-list rounds through the streaming slots (kfpos_slot_acquire_rows / kfpos_slot_submit_rows): whole-bank and
row-list submissions interleaved over the three slots, never waiting for more than the slot being refilled, compute bit
for bit what the same sequence through the synchronous API computes; a slot's pos is get_pose(0) of the listed rows;
a row-list round neither accepts KFPOS_SLOT_REUSE_* nor becomes what a later whole-bank REUSE refers to."""
import numpy as np
import pytest

from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

TOA, IMU = 0, 1


def _bank(model, T, w, storage):
    from roskfpos_amd import capi
    return capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=w.init_positions())


def _bytes_equal(p, q):
    return p.shape == q.shape and bool((np.ascontiguousarray(p).view(np.uint8) == np.ascontiguousarray(q).view(np.uint8)).all())


@pytest.mark.parametrize("model,storage,T", [(IMU, 2, 3000), (IMU, 0, 100), (TOA, 0, 3000), (TOA, 3, 1000), (IMU, 3, 1000)])
def test_interleaved_rounds_equal_the_synchronous_api(model, storage, T):
    from roskfpos_amd import capi
    S = 36
    w = Workload(T, 8)
    real = np.float64 if storage == capi.STORE_F64 else np.float32
    cov = w.accel_cov(real)
    cov[:, 1] = cov[:, 3] = 0.002
    sync, strm = _bank(model, T, w, storage), _bank(model, T, w, storage)
    NS = strm.lib.kfpos_slot_count(strm._h)
    assert NS == 3
    rng = np.random.default_rng(3)
    sizes = [1, 63, 65, T // 3, T, T // 2, 64, 7]
    expect, got, pending = [], [], []
    last_err = None                          # the errorEstimations of the last whole-bank upload

    def collect(slot, views, n, no_pose):
        strm.slot_wait(slot)
        st = views["status"][:n].copy() if n is not None else views["status"].copy()
        if no_pose:
            pos = None
        elif n is None:
            pos = views["pos"].T.copy()
        else:
            pos = views["pos"][:3 * n].reshape(3, n).T.copy()
        got.append((st, pos))

    for s in range(S):
        r, dt = w.ranges_mm(s), w.dt_of(s)
        # a different errorEstimation per upload, so that a REUSE_ERR that picked up the wrong one changes the result
        err = (w.err_est(real) * (1.0 + 0.25 * (s % 5))).astype(real)
        a = w.accel(s, real)
        rows_round = s % 4 != 0              # three in four rounds carry a row list; with slot = s % 3 every slot
                                             # changes its kind of round again and again while others are in flight
        no_pose = s % 4 == 1
        per_tag = s % 5 in (2, 4)
        kind = "toa"
        if model == IMU:
            kind = ("toa_imu", "toa", "imu")[(s // 2) % 3]
        fl = {"toa": capi.SLOT_TOA, "imu": capi.SLOT_IMU, "toa_imu": capi.SLOT_TOA_IMU}[kind]
        fl |= capi.SLOT_NO_POSE if no_pose else 0
        fl |= capi.SLOT_DT_PER_TAG if per_tag else 0
        slot = s % NS
        if rows_round:
            n = sizes[s % len(sizes)]
            rows = rng.choice(T, size=n, replace=False).astype(np.int32)
            dts = np.full(n, dt)
            if per_tag:
                dts[::4] = -1.0              # a listed tag that sits the round out
            d = dts if per_tag else dt
            if kind == "toa":
                st = sync.step_toa_rows(rows, r[rows], err[rows], d)
            elif kind == "imu":
                st = sync.step_imu_rows(rows, a[rows], cov[rows], d)
            else:
                st = sync.step_toa_imu_rows(rows, r[rows], err[rows], a[rows], cov[rows], d)
            expect.append((st, None if no_pose else sync.get_pose(0.0)[0][rows]))
            v = strm.slot_acquire_rows(slot)
            v["rows"][:n] = rows
            v["range_mm"][:n] = r[rows]
            v["err_est"][:n] = err[rows]
            v["accel"][:n] = a[rows]
            v["cov"][:n] = cov[rows]
            if per_tag:
                v["dt"][:n] = dts
            strm.slot_submit_rows(slot, fl, n, dt)
            pending.append((slot, v, n, no_pose))
        else:
            # whole-bank round; REUSE_ERR whenever an earlier whole-bank round uploaded errorEstimations: the row-list
            # rounds in between must not have become "the previous submission"
            reuse = kind != "imu" and (s // 4) % 2 == 1 and last_err is not None
            dts = np.full(T, dt)
            if per_tag:
                dts[(np.arange(T) + s) % 6 == 1] = -1.0
            d = dts if per_tag else dt
            use_err = last_err if reuse else err
            if kind == "toa":
                st = sync.step_toa(r, use_err, d)
            elif kind == "imu":
                st = sync.step_imu(a, cov, d)
            else:
                st = sync.step_toa_imu(r, use_err, a, cov, d)
            expect.append((st, None if no_pose else sync.get_pose(0.0)[0]))
            v = strm.slot_acquire(slot)
            v["range_mm"][:] = r.T
            if reuse:
                fl |= capi.SLOT_REUSE_ERR
                v["err_est"][:] = 0      # not uploaded: what the slot holds must not matter
            else:
                v["err_est"][:] = err.T
                if kind != "imu":
                    last_err = err
            v["accel"][:] = a.T
            v["cov"][:] = cov.T
            if per_tag:
                v["dt"][:] = dts
            strm.slot_submit(slot, fl, dt)
            pending.append((slot, v, None, no_pose))
        if len(pending) == NS:               # NS - 1 submissions stay in flight behind the one being collected
            collect(*pending.pop(0))
    while pending:
        collect(*pending.pop(0))
    assert len(got) == S >= 30
    for s in range(S):
        assert np.array_equal(got[s][0], expect[s][0]), f"status words, submission {s}"
        assert (got[s][1] is None) == (expect[s][1] is None)
        if got[s][1] is not None:
            assert _bytes_equal(got[s][1], expect[s][1]), f"poses, submission {s}"
    for p, q in zip(sync.get_state() + (sync.get_latch(),), strm.get_state() + (strm.get_latch(),)):
        assert _bytes_equal(p, q)
    sync.close()
    strm.close()


def test_reuse_flags_and_misuse_of_a_rows_round():
    from roskfpos_amd import capi
    T = 1000
    w = Workload(T, 8)
    b, twin = _bank(IMU, T, w, 0), _bank(IMU, T, w, 0)
    err, cov = w.err_est(), w.accel_cov()
    with pytest.raises(capi.KfposError):     # nothing acquired yet
        b.slot_submit_rows(0, capi.SLOT_TOA, 1, 0.1)
    v = b.slot_acquire(0)
    with pytest.raises(capi.KfposError):     # acquired as a whole-bank slot only: it has no row list yet
        b.slot_submit_rows(0, capi.SLOT_TOA, 1, 0.1)
    # a whole-bank round uploads errorEstimations and the covariance ...
    v["range_mm"][:] = w.ranges_mm(0).T
    v["err_est"][:] = err.T
    v["accel"][:] = w.accel(0).T
    v["cov"][:] = cov.T
    b.slot_submit(0, capi.SLOT_TOA_IMU, 0.1)
    twin.step_toa_imu(w.ranges_mm(0), err, w.accel(0), cov, 0.1)
    # ... a row-list round with OTHER values follows in the same slot and in the next one ...
    rows = np.array([5, 999, 0, 17], dtype=np.int32)
    for slot, s in ((0, 1), (1, 2)):
        q = b.slot_acquire_rows(slot)
        assert q["rows"].size == T
        q["rows"][:4] = rows
        q["range_mm"][:4] = w.ranges_mm(s)[rows]
        q["err_est"][:4] = 3 * err[rows]
        q["accel"][:4] = w.accel(s)[rows]
        q["cov"][:4] = 2 * cov[rows]
        for bad in (capi.SLOT_REUSE_ERR, capi.SLOT_REUSE_COV, capi.SLOT_REUSE_ERR | capi.SLOT_REUSE_COV):
            assert b.lib.kfpos_slot_submit_rows(b._h, slot, capi.SLOT_TOA_IMU | bad, 4, 0.05) == 1  # KFPOS_ERR_ARG
            assert b"REUSE" in b.lib.kfpos_last_error()
        b.slot_submit_rows(slot, capi.SLOT_TOA_IMU, 4, 0.05)
        twin.step_toa_imu_rows(rows, w.ranges_mm(s)[rows], 3 * err[rows], w.accel(s)[rows], 2 * cov[rows], 0.05)
        if slot == 1:
            b.slot_wait(1)
            np.testing.assert_array_equal(q["pos"][:12].reshape(3, 4).T, twin.get_pose(0.0)[0][rows])
    # ... and a whole-bank REUSE still means the values of the last WHOLE-BANK upload
    v = b.slot_acquire(2)
    v["range_mm"][:] = w.ranges_mm(3).T
    v["accel"][:] = w.accel(3).T
    b.slot_submit(2, capi.SLOT_TOA_IMU | capi.SLOT_REUSE_ERR | capi.SLOT_REUSE_COV, 0.05)
    twin.step_toa_imu(w.ranges_mm(3), err, w.accel(3), cov, 0.05)
    b.slot_wait(2)
    np.testing.assert_array_equal(v["pos"].T, twin.get_pose(0.0)[0])
    # row lists are validated at submit, before anything is enqueued
    before = [p.copy() for p in b.get_state()]
    q = b.slot_acquire_rows(0)
    for lst, named in (([1, T, 2], "outside"), ([4, 2, 4], "twice"), ([0, -1], "outside")):
        q["rows"][:len(lst)] = lst
        assert b.lib.kfpos_slot_submit_rows(b._h, 0, capi.SLOT_TOA, len(lst), 0.05) == 1
        assert named in b.lib.kfpos_last_error().decode()
    assert b.lib.kfpos_slot_submit_rows(b._h, 0, capi.SLOT_TOA, -1, 0.05) == 1
    assert b.lib.kfpos_slot_submit_rows(b._h, 0, capi.SLOT_TOA, T + 1, 0.05) == 1
    assert b.lib.kfpos_slot_submit_rows(b._h, 0, capi.SLOT_TOA, 0, 0.05) == 0      # n == 0: nothing is enqueued
    b.slot_wait(0)
    for p, q2 in zip(before, b.get_state()):
        assert _bytes_equal(p, q2)
    b.close()
    twin.close()
