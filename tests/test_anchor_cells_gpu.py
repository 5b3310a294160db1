"""kfpos_set_anchor_cells (include/kfpos.h): one bank, one launch, an anchor table per block of 64 rows.

The sentence the header gives: a handle with cells and a handle with the same configuration created under KFPOS_NO_COOP=1
that holds cell c's table in kfpos_set_anchors leave, after the same calls with the same inputs, the same bytes for every
row of every block assigned to c -- every status word, every pose, state, covariance, flags and latch. Every test here
makes those calls on the bank with cells and on one reference bank per block (or per cell) and compares those rows with
replay_checks.same_bytes (tests/anchor_cells.py).

Base shape: T = 209 (three full blocks and one of 17), 3 cells, map [2, 0, 2, 1] (not monotonic, one cell twice, a
partial block), 6 epochs with the gaps of step_checks.Trace (an absent range in epoch 2, fewer than four ranges in epoch
4) and a per-tag dt with negative entries in epoch 3. Cell c's table: the workload's anchors, rows rotated by c, moved
by (0, 0, 0), (64, -128, 2), (-37.5, 12.25, 0.5) m; its tags get the workload's ranges with the columns rotated alike
and start positions moved alike, so a block that ranged against the wrong cell is wrong by metres.

The oracle leg (F64 storage): identical status words and positions within 1e-9 m of oracle_py.OracleBank per cell, the
bound of test_gpu_parity.py; fixed start with 8 and 5 anchors for both models, ML start with 8 anchors. ML start with 5 or
16 anchors is the known unpinned edge of the oracle and belongs to the byte comparison only."""
import numpy as np
import pytest

import anchor_cells as ac
import step_checks
from conftest import has_gpu
from roskfpos_amd import capi

pytestmark = pytest.mark.gpu

T, MAP, CELLS, S = 209, [2, 0, 2, 1], 3, 6
STORAGES = [capi.STORE_F64, capi.STORE_F32, capi.STORE_MIXED, capi.STORE_P48]
ST_NAMES = {capi.STORE_F64: "f64", capi.STORE_F32: "f32", capi.STORE_MIXED: "mixed", capi.STORE_P48: "p48"}
ERR_ARG, ERR_MODEL, ERR_STATE = "invalid argument", "call not defined for this model", "call out of sequence"

# name -> (model, rounds of anchor_cells.sync_epochs, fixed start, bank options)
CONFIGS = {
    "toa6": (capi.MODEL_TOA, "toa", True, {}),
    "toa6_topn": (capi.MODEL_TOA, "toa", True, {"top_n": 4}),
    "toa6_loo": (capi.MODEL_TOA, "toa", True, {"ignore_worst": True}),
    "toa6_mlstart": (capi.MODEL_TOA, "toa", False, {}),
    "imu9_fused": (capi.MODEL_TOA_IMU, "fused", True, {}),
    "imu9_ranging": (capi.MODEL_TOA_IMU, "ranging9", True, {}),
}
MATRIX = [(c, st, A) for c in CONFIGS for st in STORAGES for A in ((8, 5, 16) if c.startswith("toa6") else (8, 5))]


def _skip():
    if not has_gpu():
        pytest.skip("no GPU")


def _per_tag_dt(n_tags, dts):
    """epoch 3: every fifth tag from the third sits out, the others have a dt of their own"""
    d = dts[3] + 0.001 * (np.arange(n_tags) % 4)
    d[2::5] = -1.0
    return {3: d}


def _trace(lay, storage, n_epochs=S, outliers=False):
    r = lay.ranges(n_epochs)
    if outliers:  # something for the outlier heuristics to leave out: 2.5 m too long, every fifth tag, epochs 1 and 5
        r[1, ::5, 3 % lay.A] += 2500
        r[5 % n_epochs, 1::5, 0] += 2500
    return step_checks.Trace(lay.w, n_epochs, storage, r=r, gaps=True)


def _sync_check(lay, config, storage, *, by="block", what):
    model, rounds, fixed, opts = CONFIGS[config]
    tr, dts = _trace(lay, storage, outliers=bool(opts)), step_checks.dts(S)
    banks = ac.Banks(lay, model, storage, by=by, init=fixed, **opts)
    try:
        assert banks.cells.anchor_cells == lay.n_cells
        res = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(S), rounds=rounds, per_tag_dt=_per_tag_dt(lay.T, dts)))
    finally:
        banks.close()
    ac.compare_rows(res, banks.groups, ac.SYNC_NAMES, what)
    st, poses = res[0][0], res[0][1]
    # the inputs did what the shape is for: tags sat epoch 3 out, and the filters ran (no NaN where a tag has started)
    assert (st[3] & 0xFF == capi.ST_SKIPPED).sum() == len(range(2, lay.T, 5))
    assert np.isfinite(poses[-1]).all()
    return res


# ---- 1. the matrix through the synchronous calls
@pytest.mark.parametrize("config,storage,A", MATRIX, ids=[f"{c}-{ST_NAMES[s]}-A{a}" for c, s, a in MATRIX])
def test_rows_of_a_cell_equal_a_bank_with_that_table(config, storage, A):
    _skip()
    _sync_check(ac.Layout(T, A, CELLS, MAP), config, storage, what=f"{config} {ST_NAMES[storage]} A={A}")


def test_a_wrong_cell_would_show_in_metres():
    """the layout's own claim: the rooms are apart, so the references of two cells differ by metres, not by last bits"""
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    res = _sync_check(lay, "toa6", capi.STORE_F64, what="toa6 f64")
    x = res[0][2]
    cells = lay.cell_of_tag()
    centre = np.stack([x[cells == c, :3].mean(0) for c in range(CELLS)])
    room = centre - lay.offsets
    assert np.abs(room[:, :2] - 5.0).max() < 1.5, room           # every cell's tags circle the middle of ITS room
    assert np.linalg.norm(centre[0] - centre[1]) > 30 and np.linalg.norm(centre[0] - centre[2]) > 30


# ---- 2. the other routes, one 6-state and one 9-state MIXED configuration
ROUTES = [(capi.MODEL_TOA, capi.STORE_MIXED), (capi.MODEL_TOA_IMU, capi.STORE_MIXED)]
ROUTE_IDS = ["toa6-mixed", "imu9-mixed"]


@pytest.mark.parametrize("model,storage", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("route", ["dev", "trace", "trace_split"])
def test_device_calls_and_trace_replay_honour_cells(model, storage, route):
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts, accel = _trace(lay, storage), step_checks.dts(S), model == capi.MODEL_TOA_IMU
    run = {"dev": lambda b: step_checks.single_calls(b, tr, dts, S, accel=accel),
           "trace": lambda b: step_checks.fused(b, tr, dts, S, accel=accel),
           "trace_split": lambda b: step_checks.fused_split(b, tr, dts, S, accel=accel, split=2)}[route]
    banks = ac.Banks(lay, model, storage)
    try:
        res = banks.call(run)
        # the replay computes what the single calls do, cells or not: one more comparison, whole bank
        if route != "dev":
            again = ac.make_bank(lay, model, storage)
            again.set_anchor_cells(lay.tables(), lay.map)
            single = step_checks.single_calls(again, tr, dts, S, accel=accel)
            again.close()
            step_checks.same(res[0], single.last(), f"{route} against single calls")
    finally:
        banks.close()
    ac.compare_rows([list(r) for r in res], banks.groups, ac.RUN_NAMES, route)


def _slot_epochs(b, tr, dts, *, d16, fused):
    """every epoch as a whole-bank slot round (d16: the ranges as int16 deltas) -> [status, poses] + left"""
    ns = b.lib.kfpos_slot_count(b._h)
    err = tr.err.cpu().numpy()
    acc, cov = tr.accel.cpu().numpy(), tr.cov.cpu().numpy()
    stats, poses = [], []
    for s in range(tr.S):
        slot = s % ns
        v = b.slot_acquire(slot)
        flags = capi.SLOT_TOA_IMU if fused else capi.SLOT_TOA
        v["err_est"][:] = err
        if fused:
            v["accel"][:] = acc[s]
            v["cov"][:] = cov
        if s == 3:
            v["dt"][:] = _per_tag_dt(tr.T, dts)[3]
            flags |= capi.SLOT_DT_PER_TAG
        if d16:
            b.slot_delta(slot)
            v["range_mm"][:] = tr.r_host[s].T
            b.slot_encode_ranges(slot, flags & capi.SLOT_DT_PER_TAG)
            flags |= capi.SLOT_RANGES_D16
        else:
            v["range_mm"][:] = tr.r_host[s].T
        b.slot_submit(slot, flags, dts[s])
        b.slot_wait(slot)
        stats.append(v["status"].copy())
        poses.append(v["pos"].T.copy())
    return [np.stack(stats), np.stack(poses)] + ac.left(b)


@pytest.mark.parametrize("model,storage", ROUTES, ids=ROUTE_IDS)
@pytest.mark.parametrize("d16", [False, True], ids=["plain", "d16"])
def test_whole_bank_slot_rounds_honour_cells(model, storage, d16):
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts = _trace(lay, storage), step_checks.dts(S)
    banks = ac.Banks(lay, model, storage)
    try:
        res = banks.call(lambda b: _slot_epochs(b, tr, dts, d16=d16, fused=model == capi.MODEL_TOA_IMU))
    finally:
        banks.close()
    ac.compare_rows(res, banks.groups, ac.SYNC_NAMES, f"slot rounds d16={d16}")
    assert (res[0][0][3] & 0xFF == capi.ST_SKIPPED).any()


# ---- 3. a larger map: an index taken from the lane instead of the block hides behind a map of four blocks
@pytest.mark.parametrize("config", ["toa6", "imu9_fused"])
def test_a_larger_random_map(config):
    _skip()
    n_blocks, n_cells = 42, 7
    cell_map = np.random.default_rng(20260).integers(0, n_cells, n_blocks)
    cell_map[:n_cells] = np.random.default_rng(7).permutation(n_cells)   # every cell occurs
    lay = ac.Layout(41 * 64 + 5, 8, n_cells, cell_map)
    assert len(set(cell_map.tolist())) == n_cells and (np.diff(cell_map) < 0).any()
    _sync_check(lay, config, capi.STORE_MIXED, by="cell", what=f"{config}, 42 blocks")


# ---- 4. remapping between two epochs
@pytest.mark.parametrize("config", ["toa6", "imu9_fused"])
def test_remapping_takes_effect_for_the_calls_after_it(config):
    """after epoch 3 block 1 changes cell (0 -> 1) and cell 2's anchors move; the references follow with set_anchors"""
    _skip()
    model, rounds, fixed, opts = CONFIGS[config]
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts = _trace(lay, capi.STORE_MIXED), step_checks.dts(S)
    new_map = [2, 1, 2, 1]
    banks = ac.Banks(lay, model, capi.STORE_MIXED, init=fixed, **opts)
    try:
        first = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(0, 4), rounds=rounds, per_tag_dt=_per_tag_dt(T, dts)))
        banks.remap(new_map, moved=(2,))
        assert banks.cells.anchor_cells == CELLS
        second = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(4, S), rounds=rounds))
    finally:
        banks.close()
    ac.compare_rows(first, banks.groups, ac.SYNC_NAMES, "before the remap")
    ac.compare_rows(second, banks.groups, ac.SYNC_NAMES, "after the remap")
    # the remap did something: block 1 ranged against a table 140 m away, blocks 0 and 2 against anchors that moved
    unmoved = ac.make_bank(lay, model, capi.STORE_MIXED, init=fixed, **opts)
    try:
        unmoved.set_anchor_cells(lay.tables(), lay.map)
        ac.sync_epochs(unmoved, tr, dts, range(0, 4), rounds=rounds, per_tag_dt=_per_tag_dt(T, dts))
        stay = ac.sync_epochs(unmoved, tr, dts, range(4, S), rounds=rounds)
    finally:
        unmoved.close()
    for b in (0, 1, 2):
        m = lay.block_of_tag == b
        assert not np.array_equal(stay[1][:, m], second[0][1][:, m]), f"block {b} did not notice the remap"
    m = lay.block_of_tag == 3
    assert stay[1][:, m].tobytes() == second[0][1][:, m].tobytes(), "block 3 (cell 1, untouched) changed"


# ---- 5. one cell is kfpos_set_anchors, and kfpos_set_anchors returns to one table
@pytest.mark.parametrize("config", ["toa6", "imu9_fused"])
def test_one_cell_is_one_table_and_set_anchors_returns_to_it(config):
    _skip()
    model, rounds, fixed, opts = CONFIGS[config]
    lay = ac.Layout(T, 8, 1, [0, 0, 0, 0])
    tr, dts = _trace(lay, capi.STORE_MIXED), step_checks.dts(S)
    banks = ac.Banks(lay, model, capi.STORE_MIXED, by="cell", init=fixed, **opts)
    try:
        first = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(0, 3), rounds=rounds))
        assert banks.cells.anchor_cells == 1
        banks.cells.set_anchors(lay.tables()[0])
        assert banks.cells.anchor_cells == 0
        second = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(3, S), rounds=rounds, per_tag_dt=_per_tag_dt(T, dts)))
        # one table again: the calls that refuse cells are back
        banks.cells.step_toa_rows(np.arange(5, dtype=np.int32), tr.r_host[0][:5], np.full((5, 8), 0.0025), 0.05)
    finally:
        banks.close()
    ac.compare_rows(first, banks.groups, ac.SYNC_NAMES, "one cell")
    ac.compare_rows(second, banks.groups, ac.SYNC_NAMES, "back to one table")


# ---- 6. refusals: they answer as the header says, and the handle steps as before
def _raises(text, f, *args, **kw):
    with pytest.raises(capi.KfposError) as e:
        f(*args, **kw)
    assert str(e.value).startswith(text), str(e.value)
    return str(e.value)


def test_bad_arguments_change_nothing():
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts = _trace(lay, capi.STORE_F64), step_checks.dts(S)
    banks = ac.Banks(lay, capi.MODEL_TOA, capi.STORE_F64)
    try:
        b, tabs = banks.cells, lay.tables()
        first = banks.call(lambda k: ac.sync_epochs(k, tr, dts, range(0, 2), rounds="toa"))
        msg = _raises(ERR_ARG, b.set_anchor_cells, tabs, [2, 0, 3, 1])
        assert "cell_of_block[2]" in msg and "= 3" in msg, msg
        msg = _raises(ERR_ARG, b.set_anchor_cells, tabs, [2, -1, 3, 1])
        assert "cell_of_block[1]" in msg, msg
        _raises(ERR_ARG, b.set_anchor_cells, np.zeros((2, 9, 3)), [0, 1, 0, 1])      # n_anchors > max_anchors
        _raises(ERR_ARG, b.set_anchor_cells, np.zeros((0, 8, 3)), [0, 0, 0, 0])      # n_cells < 1
        _raises(ERR_ARG, b.set_anchor_cells, np.zeros((1, 0, 3)), [0, 0, 0, 0])      # n_anchors < 1
        lib, h = b.lib, b._h
        m = np.asarray(MAP, dtype=np.int32)
        assert lib.kfpos_set_anchor_cells(h, 3, 8, None, m.ctypes.data) == 1
        assert lib.kfpos_set_anchor_cells(h, 3, 8, tabs.ctypes.data, None) == 1
        assert b.anchor_cells == CELLS
        second = banks.call(lambda k: ac.sync_epochs(k, tr, dts, range(2, S), rounds="toa"))
    finally:
        banks.close()
    ac.compare_rows(first, banks.groups, ac.SYNC_NAMES, "before the refused calls")
    ac.compare_rows(second, banks.groups, ac.SYNC_NAMES, "after the refused calls")


@pytest.mark.parametrize("model", [capi.MODEL_ML, capi.MODEL_PLANAR], ids=["ml", "planar"])
def test_models_without_a_cells_kernel_refuse(model):
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    b = ac.make_bank(lay, model, capi.STORE_F64)
    try:
        msg = _raises(ERR_MODEL, b.set_anchor_cells, lay.tables(), lay.map)
        assert "KFPOS_MODEL_ML and KFPOS_MODEL_PLANAR" in msg
        assert b.anchor_cells == 0
    finally:
        b.close()


@pytest.mark.parametrize("model,storage", ROUTES, ids=ROUTE_IDS)
def test_calls_that_cannot_honour_cells_refuse_and_leave_the_handle_alone(model, storage):
    _skip()
    import torch
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts = _trace(lay, storage), step_checks.dts(S)
    fusedr = model == capi.MODEL_TOA_IMU
    rounds = "fused" if fusedr else "toa"
    banks = ac.Banks(lay, model, storage)
    try:
        b = banks.cells
        first = banks.call(lambda k: ac.sync_epochs(k, tr, dts, range(0, 2), rounds=rounds))
        rows = np.array([3, 70, 200], dtype=np.int32)
        r3, e3 = tr.r_host[2][rows], np.full((3, 8), 0.0025, dtype=b.real)
        a3, c3 = np.zeros((3, 3), dtype=b.real), np.tile(np.eye(3).reshape(1, 9), (3, 1)).astype(b.real)
        why_rows, why_replay = "mixes rows of different cells in one wavefront", "no cells form of it is built"
        assert why_rows in _raises(ERR_MODEL, b.step_toa_rows, rows, r3, e3, 0.05)
        assert "kfpos_step_toa_rows" in _raises(ERR_MODEL, b.step_toa_rows, rows, r3, e3, 0.05)
        assert why_rows in _raises(ERR_MODEL, b.step_imu_rows, rows, a3, c3, 0.05)
        if fusedr:
            assert why_rows in _raises(ERR_MODEL, b.step_toa_imu_rows, rows, r3, e3, a3, c3, 0.05)
        v = b.slot_acquire_rows(0)
        v["rows"][:3] = rows
        assert why_rows in _raises(ERR_MODEL, b.slot_submit_rows, 0, capi.SLOT_TOA, 3, 0.05)
        dt_each = torch.full((2, T), 0.05, dtype=torch.float64, device=tr.r.device)
        if fusedr:
            kinds = np.array([capi.EVENT_TOA, capi.EVENT_IMU], dtype=np.uint8)
            kw = dict(range_mm=tr.r[2], stride_ranges=8 * T, err_est=tr.err, accel=tr.accel[2], stride_accel=3 * T, cov=tr.cov)
            assert why_replay in _raises(ERR_MODEL, b.run_events_dev, kinds, [0.05, 0.01], **kw)
            assert why_replay in _raises(ERR_MODEL, b.run_events_each_dev, kinds, dt_each, **kw)
        else:
            assert why_replay in _raises(ERR_MODEL, b.run_trace_each_dev, dt_each, tr.r[2], 8 * T, tr.err)
        torch.cuda.synchronize()
        assert b.anchor_cells == CELLS
        second = banks.call(lambda k: ac.sync_epochs(k, tr, dts, range(2, S), rounds=rounds, per_tag_dt=_per_tag_dt(T, dts)))
    finally:
        banks.close()
    ac.compare_rows(first, banks.groups, ac.SYNC_NAMES, "before the refused calls")
    ac.compare_rows(second, banks.groups, ac.SYNC_NAMES, "after the refused calls")


@pytest.mark.parametrize("storage", [capi.STORE_F64, capi.STORE_MIXED], ids=["f64", "mixed"])
def test_a_handle_of_the_eight_lanes_kernel_leaves_it_before_its_first_step(storage):
    """a small plain 6-state bank (<= 8 192 tags, <= 8 anchors, fixed start) would run the 8-lanes-per-tag kernel: cells
    before the first step make it a KFPOS_NO_COOP=1 handle for good -- also after kfpos_set_anchors"""
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts = _trace(lay, storage), step_checks.dts(S)
    banks = ac.Banks(lay, capi.MODEL_TOA, storage)          # (the cells bank is created WITHOUT KFPOS_NO_COOP)
    try:
        first = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(0, 3), rounds="toa"))
        ac.compare_rows(first, banks.groups, ac.SYNC_NAMES, "cells before the first step")
        # back to one table: still the one-tag-per-lane kernel, the bits of a KFPOS_NO_COOP=1 handle
        one = lay.tables()[1]
        banks.cells.set_anchors(one)
        for r in banks.refs:
            r.set_anchors(one)
        second = banks.call(lambda b: ac.sync_epochs(b, tr, dts, range(3, S), rounds="toa"))
        ac.compare_rows(second, banks.groups, ac.SYNC_NAMES, "one table after cells")
    finally:
        banks.close()


def test_a_handle_of_the_eight_lanes_kernel_that_has_stepped_refuses():
    _skip()
    lay = ac.Layout(T, 8, CELLS, MAP)
    tr, dts = _trace(lay, capi.STORE_F64), step_checks.dts(S)
    coop = ac.make_bank(lay, capi.MODEL_TOA, capi.STORE_F64)
    twin = ac.make_bank(lay, capi.MODEL_TOA, capi.STORE_F64)
    no_coop = ac.make_bank(lay, capi.MODEL_TOA, capi.STORE_F64, no_coop=1)
    try:
        a0 = ac.sync_epochs(coop, tr, dts, range(0, 2), rounds="toa")
        b0 = ac.sync_epochs(twin, tr, dts, range(0, 2), rounds="toa")
        msg = _raises(ERR_STATE, coop.set_anchor_cells, lay.tables(), lay.map)
        assert "8-lanes-per-tag" in msg and coop.anchor_cells == 0
        a1 = ac.sync_epochs(coop, tr, dts, range(2, S), rounds="toa")
        b1 = ac.sync_epochs(twin, tr, dts, range(2, S), rounds="toa")
        # a handle created under KFPOS_NO_COOP=1 never ran that kernel: it takes cells after a step
        ac.sync_epochs(no_coop, tr, dts, range(0, 2), rounds="toa")
        no_coop.set_anchor_cells(lay.tables(), lay.map)
        assert no_coop.anchor_cells == CELLS
    finally:
        for b in (coop, twin, no_coop):
            b.close()
    names = [n for n, _ in ac.SYNC_NAMES]
    ac.same_bytes(a0, b0, names, "before the refused call")
    ac.same_bytes(a1, b1, names, "after the refused call")


# ---- 7. the oracle leg
ORACLE = [("toa6", True, 8), ("toa6", True, 5), ("imu9_fused", True, 8), ("imu9_fused", True, 5), ("toa6", False, 8),
          ("imu9_fused", False, 8)]


@pytest.mark.parametrize("config,fixed,A", ORACLE, ids=[f"{c}-{'fixed' if f else 'mlstart'}-A{a}" for c, f, a in ORACLE])
def test_every_cell_meets_the_oracle(config, fixed, A):
    """F64 storage: identical status words, positions within 1e-9 m (test_gpu_parity.py's bound), per cell"""
    _skip()
    import oracle_py
    model, rounds, _, _ = CONFIGS[config]
    lay = ac.Layout(T, A, CELLS, MAP)
    tr, dts = _trace(lay, capi.STORE_F64), step_checks.dts(S)
    per_tag = _per_tag_dt(T, dts)
    b = ac.make_bank(lay, model, capi.STORE_F64, init=fixed)
    b.set_anchor_cells(lay.tables(), lay.map)
    try:
        st, poses = ac.sync_epochs(b, tr, dts, range(S), rounds=rounds, per_tag_dt=per_tag)[:2]
    finally:
        b.close()
    err = tr.err.cpu().numpy().T.astype(np.float64)
    acc, cov = tr.accel.cpu().numpy().transpose(0, 2, 1).astype(np.float64), tr.cov_host.astype(np.float64)
    cells, worst = lay.cell_of_tag(), 0.0
    for c in range(CELLS):
        o = oracle_py.OracleBank(model, T, lay.tables()[c], init_pos=lay.init() if fixed else None, n_threads=8)
        m = cells == c
        for s in range(S):
            dt = per_tag.get(s, dts[s])
            if model == capi.MODEL_TOA_IMU:
                o.step_imu(acc[s], cov, np.where(np.asarray(dt) < 0, -1.0, 0.0) if s in per_tag else 0.0)
            so = np.asarray(o.step_toa(tr.r_host[s], err, dt)).astype(np.uint32)
            po = o.get_state()[0][:, :3]
            assert np.array_equal(so[m], st[s][m]), f"status words, cell {c}, epoch {s}"
            assert np.array_equal(np.isnan(po[m]), np.isnan(poses[s][m])), f"cell {c}, epoch {s}"
            d = np.abs(po[m] - poses[s][m])
            worst = max(worst, float(np.nanmax(d)) if np.isfinite(d).any() else 0.0)
    print(f"{config} fixed={fixed} A={A}: largest position difference against the oracle {worst:.3e} m")
    assert worst <= 1e-9, worst
