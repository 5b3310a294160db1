"""roskfpos_amd.synth.merge_timelines with no IMU samples (n_sub = 0) yields the ranging-only slot schedules of
kfpos_run_trace_each_dev: all-TOA kinds, every tag's own timeline in the slots it takes part in, and the oracle of the
6-state filter stepped slot by slot with the dt rows (dt < 0 = the tag sits the slot out) gives each tag exactly what it
gives that tag stepped alone on its own timeline (no GPU needed)."""
import numpy as np
import pytest

from cases import Case
from roskfpos_amd import synth
from roskfpos_amd.synth import Workload

T, A, PERIODS = 6, 8, 9
PERIOD = np.array([0.05, 0.05, 0.05, 0.04, 0.1, 0.05])
PHASE = np.array([0.0, 0.0125, 0.0, 0.003, 0.02, 0.0])     # tags 0, 2 and 5 range in the same TDMA slot


@pytest.fixture(scope="module")
def sched():
    return synth.merge_timelines(PERIOD, 0, PHASE, PERIODS)


def test_ranging_only_timelines_merge_into_all_toa_slots(sched):
    E = sched.kinds.size
    assert sched.dt.shape == sched.step.shape == (E, T)
    assert (sched.kinds == 1).all()                                     # every slot is a ranging slot
    assert (sched.sub == -1).all() and (sched.n_sub == 0).all()
    assert (np.diff(sched.time) > 0).all()
    present = sched.present
    assert np.array_equal(present, sched.step >= 0)
    assert (sched.dt[~present] < 0).all() and (sched.dt[present] > 0).all()
    assert present.any(axis=1).all(), "a slot nobody takes part in"
    assert not present.all(axis=1).any(), "differing clocks never meet in one slot here"
    for t in range(T):
        slots = np.flatnonzero(present[:, t])
        # no tag appears twice in a slot: its PERIODS epochs sit in PERIODS different slots, in order
        assert slots.size == PERIODS and [int(s) for s in sched.step[slots, t]] == list(range(PERIODS))
        last = PHASE[t] + PERIODS * PERIOD[t]
        assert abs(sched.dt[slots, t].sum() - last) < 1e-12             # its dts sum to its last event time
        assert abs(sched.time[slots[-1]] - last) < 1e-9
        assert np.allclose(sched.dt[slots[1:], t], PERIOD[t], rtol=0, atol=1e-12)
        assert abs(sched.dt[slots[0], t] - (PHASE[t] + PERIOD[t])) < 1e-12
    assert np.array_equal(sched.dt[:, 0], sched.dt[:, 5]) and np.array_equal(sched.dt[:, 0], sched.dt[:, 2])
    sync = synth.merge_timelines(np.full(4, 0.05), 0, 0.0, 3)           # one clock: nobody is ever absent
    assert sync.dt.shape == (3, 4) and (sync.dt > 0).all() and (sync.kinds == 1).all()


@pytest.mark.parametrize("fixed,ignore_worst", [(True, False), (False, False), (True, True)])
def test_oracle_over_the_merged_slots_equals_each_tag_stepped_alone(sched, fixed, ignore_worst):
    import oracle_py
    w = Workload(T, A)
    case = Case("each", 0, A, T=T, fixed=fixed, outlier=ignore_worst)
    ranges, _ = synth.slot_inputs(w, sched, np.float64, epoch=case.epoch, absent_mm=1999999999)
    assert ranges.shape == (sched.kinds.size, T, A)
    err = w.err_est()
    init = w.init_positions() if fixed else None
    bank = oracle_py.OracleBank(0, T, w.anchors, ignore_worst=ignore_worst, init_pos=init)
    words = np.zeros(sched.dt.shape, dtype=np.uint32)
    for e in range(sched.kinds.size):
        words[e] = bank.step_toa(ranges[e], err, sched.dt[e])
    assert ((words == 64) == ~sched.present).all()          # KFPOS_ST_SKIPPED exactly where the tag is absent
    xb, Pb = bank.get_state()[:2]
    assert np.isfinite(xb).all()
    for t in range(T):
        one = oracle_py.OracleBank(0, 1, w.anchors, ignore_worst=ignore_worst,
                                   init_pos=None if init is None else init[t:t + 1])
        own = [one.step_toa(case.epoch(w, int(sched.step[e, t]))[t:t + 1], err[t:t + 1], sched.dt[e, t])[0]
               for e in np.flatnonzero(sched.present[:, t])]
        x1, P1 = one.get_state()[:2]
        assert x1[0].tobytes() == xb[t].tobytes() and P1[0].tobytes() == Pb[t].tobytes(), t
        assert np.array_equal(np.array(own, dtype=np.uint32), words[sched.present[:, t], t]), t
