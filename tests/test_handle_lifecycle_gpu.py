"""The handle's resources over its whole life: a bank is created, stepped, takes every part it allocates on first use,
is read and closed, twenty times in one process, and the twentieth computes the bytes of the first. kfpos_destroy frees
nothing by name any more -- each member of the handle gives back what it owns (roskfpos_amd/csrc/kfpos_owned.h) -- so a
member freed twice, or used after its release, shows here as a refused call, a fault or different bytes.

Each of the four models at T = 130 (two full wavefronts and a partial one), A = 8, KFPOS_STORE_MIXED, fixed start. The
parts allocated on first use: the work block (a row-list step), the slots with their streams and events (a streaming
round), the slot's row list and pose arrays (a row-list streaming round with KFPOS_SLOT_POSE_COV), the D16 blocks and
base (a D16 round), the cells' table and map (kfpos_set_anchor_cells, on the two filters that have cells kernels; ahead
of the first step, since a fixed-start 6-state bank of this size runs the 8-lanes-per-tag kernel until then, and undone
with kfpos_set_anchors, since a bank with cells refuses row lists). Every call returns KFPOS_OK (KfposBank raises
otherwise; kfpos_destroy's answer is asserted). No memory is measured: free-memory readings on a shared card belong to
everybody."""
import numpy as np
import pytest

from planar import CFG
from replay_checks import same_bytes
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

T, A, LIVES = 130, 8, 20
ROWS = np.array([129, 0, 64, 65, 7, 128, 63], dtype=np.int32)   # every wavefront, both ends of the bank, unsorted
NAMES = ["cells status", "step status", "rows status", "slot status", "slot pos", "rows slot status", "rows slot pos",
         "rows slot cov", "rows slot vel", "d16 status", "d16 pos", "pose", "pose cov", "pose vel", "pose status", "x", "P",
         "flags", "latch"]


def one_life(model, w):
    """create, step, every part allocated on first use, read, close -> what the bank computed on the way"""
    from roskfpos_amd import capi
    imu9, planar = model == capi.MODEL_TOA_IMU, model == capi.MODEL_PLANAR
    b = capi.KfposBank(model, T, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions(),
                       planar=CFG if planar else None)
    err, acc, cov = w.err_est(np.float32), w.accel(0, np.float32), w.accel_cov(np.float32)
    out = []
    if model in (capi.MODEL_TOA, capi.MODEL_TOA_IMU):
        b.set_anchor_cells(np.stack([w.anchors, w.anchors + (0.25, -0.5, 0.125)]), np.array([0, 1, 0], dtype=np.int32))
        out.append(b.step_toa(w.ranges_mm(0), err, w.dt_of(0)))
        b.set_anchors(w.anchors)
    else:
        out.append(np.zeros(T, dtype=np.uint32))
    r = w.ranges_mm(1)
    out.append(b.step_toa_imu(r, err, acc, cov, w.dt_of(1)) if imu9 else b.step_toa(r, err, w.dt_of(1)))
    r = w.ranges_mm(2)
    out.append(b.step_toa_rows(ROWS, r[ROWS], err[ROWS], w.dt_of(2)))
    # a streaming round
    v = b.slot_acquire(0)
    v["range_mm"][:], v["err_est"][:] = w.ranges_mm(3).T, err.T
    b.slot_submit(0, capi.SLOT_TOA, w.dt_of(3))
    b.slot_wait(0)
    out += [v["status"].copy(), v["pos"].copy()]
    # a row-list streaming round that returns what is published
    n, r = ROWS.size, w.ranges_mm(4)
    v = b.slot_acquire_rows(1)
    v["rows"][:n], v["range_mm"][:n], v["err_est"][:n] = ROWS, r[ROWS], err[ROWS]
    b.slot_submit_rows(1, capi.SLOT_TOA | capi.SLOT_POSE_COV, n, w.dt_of(4))
    b.slot_wait(1)
    pcov, pvel = b.slot_pose_rows(1, n)
    out += [v["status"][:n].copy(), v["pos"][:3 * n].copy(), pcov.copy(), pvel.copy()]
    # a D16 round
    v = b.slot_acquire(2)
    b.slot_delta(2)
    v["range_mm"][:], v["err_est"][:] = w.ranges_mm(5).T, err.T
    b.slot_encode_ranges(2)
    b.slot_submit(2, capi.SLOT_TOA | capi.SLOT_RANGES_D16, w.dt_of(5))
    b.slot_wait(2)
    out += [v["status"].copy(), v["pos"].copy()]
    out += list(b.get_pose(0.0))
    out += list(b.get_state()) + [b.get_latch()]
    assert b.lib.kfpos_destroy(b._h) == 0
    b._h = None
    return out


@pytest.mark.parametrize("model", [0, 1, 2, 3], ids=["toa6", "imu9", "ml", "planar"])
def test_the_twentieth_bank_computes_what_the_first_did(model):
    w = Workload(T, A)
    first = one_life(model, w)
    assert len(first) == len(NAMES)
    assert np.isfinite(first[NAMES.index("pose")]).all()   # (a bank of NaN would repeat its bytes whatever happened)
    for _ in range(LIVES - 2):
        one_life(model, w)
    same_bytes(one_life(model, w), first, NAMES, f"bank {LIVES} against bank 1, model {model}")
