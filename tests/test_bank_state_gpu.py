"""The whole-bank accessors through the C ABI on the card: kfpos_get_state / kfpos_set_state, kfpos_get_latch /
kfpos_set_latch, kfpos_get_height / kfpos_set_height, every model in every storage mode, after a handful of epochs so that
nothing in the bank is zero.

Bank sizes: 1 tag, and 65 -- a second wavefront with one lane in it, and a row stride that is no multiple of 64. What a
set stores and a get returns is pinned bit for bit: doubles as they are, 4-byte elements as np.float32 rounds, 48-bit
covariance entries as tests/p48.py (the numpy mirror of kfpos_p48.h) rounds; a packed covariance keeps j >= i, the 9-state
latch covariance i >= j."""
import numpy as np
import pytest

from p48 import p48_round_trip
from roskfpos_amd.synth import Workload
from test_tag_lifecycle_gpu import IMU, ML, MODELS, PLANAR, apply, assert_same, inputs, make_bank, real_of, snapshot

pytestmark = pytest.mark.gpu

SIZES = (1, 65)
EPOCHS = 6  # the planar trace has fed all four sensors by then (test_tag_lifecycle_gpu.apply)
PARAMS = [pytest.param(name, st, T, id=f"{name}-st{st}-T{T}")
          for name, (_, _, sts) in MODELS.items() for st in sts for T in SIZES]


def stepped_bank(name, storage, T):
    w = Workload(T, 8)
    b = make_bank(name, storage, w)
    for s in range(EPOCHS):
        apply(b, name, s, inputs(name, w, s, real_of(storage)))
    return b, w


def cov_rounding(storage):
    """what the storage mode keeps of a covariance entry"""
    from roskfpos_amd import capi
    if storage == capi.STORE_F32:
        return lambda v: v.astype(np.float32).astype(np.float64)
    if storage == capi.STORE_P48:
        return lambda v: p48_round_trip(v).reshape(v.shape)
    return lambda v: v.copy()


def expected(name, storage, x, P, latch):
    """what the getters return after the setters stored (x, P, latch)"""
    model, fixed, _ = MODELS[name]
    n = x.shape[1]
    ex = x.copy()
    if n == 6:
        ex[:, 3:] = 0.0   # the 6-state velocity is not a stored member
    if n == 9:
        ex[:, 6:] = 0.0   # a = 0
    if n == 8:
        ex[:, 4:6] = 0.0  # [x y vx vy 0 0 theta omega]
    full = model == 0 and not fixed  # COV_FULL: the 6-state filter with ML initialisation
    eP = P if full else np.triu(P) + np.transpose(np.triu(P, 1), (0, 2, 1))
    eP = cov_rounding(storage)(eP)
    el = latch.copy()
    if model == IMU:  # acceleration + the lower triangle of its covariance, in kfpos_real
        c = latch[:, 3:].reshape(-1, 3, 3)
        c = np.tril(c) + np.transpose(np.tril(c, -1), (0, 2, 1))
        el = np.concatenate([latch[:, :3], c.reshape(-1, 9)], axis=1).astype(real_of(storage)).astype(np.float64)
    return ex, eP, el


def random_record(b, seed):
    rng = np.random.default_rng(seed)
    L = b.lib.kfpos_latch_dim(b._h)
    return (rng.standard_normal((b.T, b.n)), rng.standard_normal((b.T, b.n, b.n)) * 1e-3,
            rng.integers(0, 4, b.T).astype(np.uint32), rng.standard_normal((b.T, L)))


# ---------------------------------------------------------------- 1. round trip
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_set_then_get_returns_the_stored_rounding(name, storage, T):
    b, _ = stepped_bank(name, storage, T)
    x, P, fl, latch = random_record(b, 11 * T + storage)
    z = np.random.default_rng(5).standard_normal(T)
    b.set_state(x, P, fl)
    b.set_latch(latch)
    if b.model == PLANAR:
        b.set_height(z)
    ex, eP, el = expected(name, storage, x, P, latch)
    gx, gP, gfl = b.get_state()
    np.testing.assert_array_equal(gx, ex)
    np.testing.assert_array_equal(gP, eP)
    np.testing.assert_array_equal(gfl, fl)
    np.testing.assert_array_equal(b.get_latch(), el)
    if b.model == PLANAR:
        np.testing.assert_array_equal(b.get_height(), z)


# ---------------------------------------------------------------- 2. absent parts (capi always passes x and P)
@pytest.mark.parametrize("name,storage,T", PARAMS)
def test_absent_parts_are_neither_read_nor_written(name, storage, T):
    b, _ = stepped_bank(name, storage, T)
    lib, h = b.lib, b._h
    x0, P0, fl0 = b.get_state()
    x, P, fl = np.full_like(x0, 7.0), np.full_like(P0, 7.0), np.full_like(fl0, 7)
    assert lib.kfpos_get_state(h, x.ctypes.data, None, None) == 0
    assert lib.kfpos_get_state(h, None, P.ctypes.data, None) == 0
    assert lib.kfpos_get_state(h, None, None, fl.ctypes.data) == 0
    assert_same([x, P, fl], [x0, P0, fl0], "one part at a time")
    before = snapshot(b)
    _, P1, _, _ = random_record(b, 3)
    assert lib.kfpos_set_state(h, None, P1.ctypes.data, None) == 0
    after = snapshot(b)
    np.testing.assert_array_equal(after[1], expected(name, storage, x0, P1, before[3])[1])
    after[1] = before[1]
    assert_same(after, before, "everything but P")
    assert lib.kfpos_last_error() == b""


# ---------------------------------------------------------------- 3. the planar filter's rows of d_pos
@pytest.mark.parametrize("storage", MODELS["planar"][2])
@pytest.mark.parametrize("T", SIZES)
def test_planar_state_and_height_keep_each_other(storage, T):
    b, _ = stepped_bank("planar", storage, T)
    before = snapshot(b)
    x, P, fl, _ = random_record(b, 17)
    b.set_state(x, P, fl)
    np.testing.assert_array_equal(b.get_height(), before[4])
    x1 = b.get_state()[0]
    b.set_height(before[4] + 1.5)
    np.testing.assert_array_equal(b.get_state()[0], x1)
    np.testing.assert_array_equal(b.get_height(), before[4] + 1.5)
    np.testing.assert_array_equal(b.get_latch(), before[3])


# ---------------------------------------------------------------- 4. asymmetric P into a packed bank
@pytest.mark.parametrize("name", ["toa6_fixed", "imu9", "planar", "ml"])
def test_packed_bank_reads_back_the_upper_half_of_an_asymmetric_P(name):
    b, _ = stepped_bank(name, 0, 65)
    x, P, fl, _ = random_record(b, 23)
    lower = np.tril_indices(b.n, -1)
    assert np.all(P[:, lower[0], lower[1]] != P[:, lower[1], lower[0]])
    b.set_state(x, P, fl)
    got = b.get_state()[1]
    np.testing.assert_array_equal(got, np.transpose(got, (0, 2, 1)))
    np.testing.assert_array_equal(np.triu(got), np.triu(P))


# ---------------------------------------------------------------- 5. restored planar latch bits select the kernel
@pytest.mark.parametrize("T", SIZES)
def test_planar_flags_with_latch_bits_switch_the_ranging_kernel(T):
    fed, w = stepped_bank("planar", 0, T)  # has seen every sensor: its ranging epochs honour the latches
    x, P, fl, latch, z = snapshot(fed)
    assert np.all(fl >> 4)  # every tag carries latch bits (PX4Flow / IMU / magnetometer)
    restored = make_bank("planar", 0, w)  # never fed a sensor sample
    restored.set_state(x, P, fl)
    restored.set_latch(latch)
    restored.set_height(z)
    assert_same(snapshot(restored), [x, P, fl, latch, z], "right after the restore")
    r, err = w.ranges_mm(EPOCHS), w.err_est()
    sa, sb = fed.step_toa(r, err, 0.1), restored.step_toa(r, err, 0.1)
    np.testing.assert_array_equal(sa, sb)
    assert_same(snapshot(restored), snapshot(fed), "after a ranging epoch")
