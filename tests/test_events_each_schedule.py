"""roskfpos_amd.synth.merge_timelines: per-tag timelines merged into the slots of kfpos_run_events_each_dev. Every tag
finds its own timeline again in the slots it takes part in, and the oracle stepped slot by slot with per-tag dt < 0
gives each tag exactly what it gives that tag stepped alone on its own timeline (no GPU needed)."""
import numpy as np
import pytest

from cases import Case
from roskfpos_amd import synth
from roskfpos_amd.synth import Workload

T, A, PERIODS = 6, 8, 5
PERIOD = np.array([0.05, 0.05, 0.05, 0.04, 0.1, 0.05])
N_SUB = np.array([4, 4, 2, 3, 0, 4])
PHASE = np.array([0.0, 0.0125, 0.0, 0.003, 0.02, 0.0])     # tags 0 and 5 are synchronous with each other


@pytest.fixture(scope="module")
def sched():
    return synth.merge_timelines(PERIOD, N_SUB, PHASE, PERIODS)


def test_every_tag_finds_its_own_timeline_in_its_slots(sched):
    E = sched.kinds.size
    assert sched.dt.shape == sched.step.shape == sched.sub.shape == (E, T)
    assert set(np.unique(sched.kinds)) == {0, 1}
    assert (np.diff(sched.time) >= 0).all()
    present = sched.present
    assert np.array_equal(present, sched.step >= 0)
    assert (sched.dt[~present] < 0).all() and (sched.dt[present] > 0).all()
    assert present.any(axis=1).all(), "a slot nobody takes part in"
    for t in range(T):
        own = synth.tag_timeline(PERIOD[t], N_SUB[t], PHASE[t], PERIODS)
        slots = np.flatnonzero(present[:, t])
        assert slots.size == len(own) == PERIODS * (N_SUB[t] + 1)
        assert [int(k) for k in sched.kinds[slots]] == [ev[1] for ev in own]
        assert [int(s) for s in sched.step[slots, t]] == [ev[2] for ev in own]
        assert [int(s) for s in sched.sub[slots, t]] == [ev[3] for ev in own]
        times = np.array([ev[0] for ev in own])
        assert np.allclose(np.cumsum(sched.dt[slots, t]), times, rtol=0, atol=1e-12)
        assert abs(sched.dt[slots, t].sum() - (PHASE[t] + PERIODS * PERIOD[t])) < 1e-12   # its elapsed time
        assert np.allclose(sched.time[slots], times, rtol=0, atol=1e-9)
    # tags on the same clock share every slot; a fully synchronous bank has no absent entry at all
    assert np.array_equal(sched.dt[:, 0], sched.dt[:, 5])
    sync = synth.merge_timelines(0.05, 4, 0.0, 3)
    assert sync.dt.shape == (15, 1) and (sync.dt > 0).all()
    sync = synth.merge_timelines(np.full(4, 0.05), 4, 0.0, 3)
    assert sync.dt.shape == (15, 4) and (sync.dt > 0).all()
    assert [int(k) for k in sync.kinds] == [0, 0, 0, 0, 1] * 3


def test_slot_inputs_hold_each_tags_own_samples_and_nothing_for_absent_tags(sched):
    w = Workload(T, A)
    case = Case("each", 1, A, T=T)
    ranges, accel = synth.slot_inputs(w, sched, np.float64, epoch=case.epoch, absent_mm=-777)
    assert ranges.shape == (int((sched.kinds == 1).sum()), T, A) and accel.shape == (int((sched.kinds == 0).sum()), T, 3)
    j = i = 0
    for e, kind in enumerate(sched.kinds):
        for t in range(T):
            here = sched.step[e, t] >= 0
            if kind == 1:
                want = case.epoch(w, int(sched.step[e, t]))[t] if here else np.full(A, -777)
                assert np.array_equal(ranges[j, t], want)
            elif here:
                want = w.accel_between(int(sched.step[e, t]), int(sched.sub[e, t]), int(N_SUB[t]))[t]
                assert np.array_equal(accel[i, t], want)
            else:
                assert np.isnan(accel[i, t]).all()
        j += kind == 1
        i += kind == 0


@pytest.mark.parametrize("fixed", [True, False])
def test_oracle_over_the_merged_slots_equals_each_tag_stepped_alone(sched, fixed):
    import oracle_py
    w = Workload(T, A)
    case = Case("each", 1, A, T=T, fixed=fixed, cov_full=True)
    ranges, accel = synth.slot_inputs(w, sched, np.float64, epoch=case.epoch)
    err, cov = w.err_est(), case.accel_cov(w)
    init = w.init_positions() if fixed else None
    bank = oracle_py.OracleBank(1, T, w.anchors, init_pos=init)
    words = np.zeros(sched.dt.shape, dtype=np.uint32)
    j = i = 0
    for e, kind in enumerate(sched.kinds):
        if kind == 1:
            words[e] = bank.step_toa(ranges[j], err, sched.dt[e])
            j += 1
        else:
            words[e] = bank.step_imu(np.nan_to_num(accel[i], nan=0.0), cov, sched.dt[e])
            i += 1
    assert ((words == 64) == ~sched.present).all()          # KFPOS_ST_SKIPPED exactly where the tag is absent
    xb, Pb = bank.get_state()[:2]
    for t in range(T):
        one = oracle_py.OracleBank(1, 1, w.anchors, init_pos=None if init is None else init[t:t + 1])
        own = []
        j = i = 0
        for e, kind in enumerate(sched.kinds):
            if sched.step[e, t] >= 0:
                if kind == 1:
                    own.append(one.step_toa(ranges[j, t:t + 1], err[t:t + 1], sched.dt[e, t])[0])
                else:
                    own.append(one.step_imu(accel[i, t:t + 1], cov[t:t + 1], sched.dt[e, t])[0])
            j += kind == 1
            i += kind == 0
        x1, P1 = one.get_state()[:2]
        assert x1[0].tobytes() == xb[t].tobytes() and P1[0].tobytes() == Pb[t].tobytes(), t
        assert np.array_equal(np.array(own, dtype=np.uint32), words[sched.present[:, t], t]), t
