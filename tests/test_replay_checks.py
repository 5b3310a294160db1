"""tests/replay_checks.py: the byte comparison the GPU tests of the five replay entry points rest on tells apart what it
must, and the environment manager puts back what it found. No GPU, no library."""
import os

import numpy as np
import pytest

import replay_checks as rc

NAMES = ("first", "second", "third")


def _tuple():
    rng = np.random.default_rng(1)
    return rng.normal(size=(4, 3)), rng.integers(0, 99, size=5).astype(np.int32), rng.normal(size=7)


def _differs(got, ref, name, **kw):
    with pytest.raises(AssertionError) as err:
        rc.same_bytes(got, ref, NAMES, "case", **kw)
    assert err.value.args[0] == ("case", name)


def test_same_bytes_passes_on_equal_tuples():
    rc.same_bytes(_tuple(), _tuple(), NAMES, "case")


def test_same_bytes_sees_one_bit_of_a_float64():
    got, ref = _tuple(), _tuple()
    got[2].view(np.uint64)[3] ^= 1                  # the lowest mantissa bit of one element
    assert np.allclose(got[2], ref[2], rtol=1e-15, atol=0)
    _differs(got, ref, "third")


def test_same_bytes_tells_the_zeros_apart():
    assert np.array_equal(np.array([0.0]), np.array([-0.0]))
    _differs((np.array([0.0]),), (np.array([-0.0]),), "first")


def test_same_bytes_compares_dtype_and_shape_ahead_of_the_bytes():
    a = np.arange(6, dtype=np.int32)
    assert a.tobytes() == a.astype(np.uint32).tobytes()
    _differs((a,), (a.astype(np.uint32),), "first")
    assert a.reshape(2, 3).tobytes() == a.reshape(3, 2).tobytes()
    _differs((a.reshape(2, 3),), (a.reshape(3, 2),), "first")


def test_same_bytes_passes_the_same_nan_payload():
    nan = np.array([0x7FF8000000000123, 0xFFF0000000000001], dtype=np.uint64).view(np.float64)
    assert np.isnan(nan).all() and not np.array_equal(nan, nan.copy())
    rc.same_bytes((nan,), (nan.copy(),), NAMES, "case")
    other = nan.copy()
    other.view(np.uint64)[0] ^= 1                   # another payload: still NaN, other bytes
    _differs((nan,), (other,), "first")


def test_same_bytes_skips_the_entries_before_first():
    got, ref = _tuple(), _tuple()
    got[0][0, 0] += 1.0
    rc.same_bytes(got, ref, NAMES, "case", first=2)
    rc.same_bytes(got, ref, NAMES, "case", first=1)
    _differs(got, ref, "first", first=0)
    rc.same_bytes((None,) + got[1:], ref, NAMES, "case", first=1)     # what a call without per-slot outputs returns


SET, UNSET, NEW = "KFPOS_TEST_REPLAY_SET", "KFPOS_TEST_REPLAY_UNSET", "KFPOS_TEST_REPLAY_NEW"


@pytest.mark.parametrize("raises", [False, True])
def test_env_sets_unsets_and_restores(raises):
    os.environ[SET], os.environ[UNSET] = "before", "here"
    os.environ.pop(NEW, None)
    try:
        try:
            with rc.env(**{SET: 7, UNSET: None, NEW: "x"}):
                assert os.environ[SET] == "7" and UNSET not in os.environ and os.environ[NEW] == "x"
                if raises:
                    raise KeyError("from the body")
        except KeyError:
            assert raises
        assert os.environ[SET] == "before" and os.environ[UNSET] == "here"
        assert NEW not in os.environ                # it did not exist before: not set again
    finally:
        for k in (SET, UNSET, NEW):
            os.environ.pop(k, None)


def test_ordinals_count_within_a_kind():
    got = list(rc.ordinals(np.array([0, 2, 2, 0, 1, 2], dtype=np.uint8), 3))
    assert [e for e, _, _ in got] == [0, 1, 2, 3, 4, 5]
    assert [k for _, k, _ in got] == [0, 2, 2, 0, 1, 2] and all(type(k) is int for _, k, _ in got)
    assert [i for _, _, i in got] == [0, 0, 1, 1, 0, 2]
