"""Where the lanes of a 9-state wavefront meet to hand the tail of the gain iteration to pairs (iekf9_next_meet in
kfpos_core_imu9.h, a KFPOS_HD function: the kernels walk it on the device, kfpos_pair9_meet_points walks the same function
on the host) and how kfpos_create reads KFPOS_PAIR9_MEET=first,dense_until. (CPU only: the library loads without a GPU,
and kfpos_create judges the variable before it looks for a device.) And the seed of tests/test_pairs9_meet_gpu.py: the oracle
alone sees every way a wavefront can meet, at T = 128, in the trace of tests/pairs9_meet_cases.py."""
import ctypes as C

import pytest

import pairs9_meet_cases as pm

from replay_checks import env
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload

CAP = 20


def _points(first, dense_until):
    lib = capi.load()
    lib.kfpos_pair9_meet_points.argtypes = [C.c_int32, C.c_int32, C.POINTER(C.c_int32)]
    lib.kfpos_pair9_meet_points.restype = C.c_int
    out = (C.c_int32 * (CAP + 4))(*([-7] * (CAP + 4)))
    n = lib.kfpos_pair9_meet_points(first, dense_until, out)
    assert all(v == -7 for v in out[max(n, 0):]), "written beyond what it returned"
    return None if n < 0 else list(out[:n])


def test_the_two_schedules_by_name():
    assert _points(8, 8) == [8, 12, 16, 20]                      # what the kernels did before the schedule was data
    assert _points(7, 10) == [7, 8, 9, 10, 14, 18, 20]
    assert _points(8, 10) == [8, 9, 10, 14, 18, 20]              # the default
    assert _points(1, 20) == list(range(1, 21))                  # a meeting after every solve
    assert _points(20, 20) == [20]


def test_every_schedule_in_range():
    for first in range(1, CAP + 1):
        for dense_until in range(first, CAP + 1):
            p = _points(first, dense_until)
            what = (first, dense_until, p)
            assert p[0] == first and p[-1] == CAP and len(p) <= CAP, what
            assert all(b > a for a, b in zip(p, p[1:])), what    # strictly increasing
            for a, b in zip(p, p[1:]):                            # one solve on below dense_until, four from there, capped
                assert b == min(a + (1 if a < dense_until else 4), CAP), what


@pytest.mark.parametrize("first,dense_until", [(0, 8), (-1, 4), (9, 8), (7, 21), (21, 21), (0, 0), (1 << 30, 1 << 30)])
def test_out_of_range_schedules_have_no_points(first, dense_until):
    assert _points(first, dense_until) is None
    lib = capi.load()
    assert lib.kfpos_pair9_meet_points(7, 10, None) == -1


def _create(value):
    """kfpos_create with KFPOS_PAIR9_MEET=value -> the error text, or None when a bank was made (a GPU is present)"""
    w = Workload(64, 8)
    with env(KFPOS_PAIR9_MEET=value):
        try:
            capi.KfposBank(capi.MODEL_TOA_IMU, 64, w.anchors, storage=capi.STORE_MIXED, init_pos=w.init_positions()).close()
        except capi.KfposError as e:
            return str(e)
    return None


@pytest.mark.parametrize("value", ["0,8", "9,8", "7,21", "21,21", "-1,4", "7", "7,", ",10", "7,10,3", "7,10x", "a,b", "7;10", " "])
def test_kfpos_create_refuses_what_is_not_a_schedule(value):
    text = _create(value)
    assert text is not None and text.startswith("invalid argument") and "KFPOS_PAIR9_MEET" in text, text


@pytest.mark.parametrize("value", [None, "", "7,10", "8,8", "1,20", "20,20", "1,1"])
def test_kfpos_create_takes_every_schedule_in_range(value):
    text = _create(value)         # without a GPU the call goes on to fail for want of one -- not for its arguments
    assert text is None or (not text.startswith("invalid argument") and "KFPOS_PAIR9_MEET" not in text), text


def test_the_oracle_alone_sees_every_meeting_scenario_for_the_chosen_seed():
    g = pm.gain_iters(pm.oracle_run(128, pm.seed())[1])
    first, second = pm.scenarios(g[:, :64], pm.MARGIN), pm.scenarios(g[:, 64:])
    print(f"seed {pm.seed()}: first wavefront {({k: v.tolist() for k, v in first.items()})}, "
          f"second {({k: v.tolist() for k, v in second.items()})}")
    assert set(first) == set(pm.SCENARIOS) and all(len(v) for v in first.values()), first
    assert 4 in first["at most 32 by 6"]          # the epoch with tags of fewer than four ranges hands over at the first meeting
