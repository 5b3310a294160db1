"""The per-tag planar schedule (no GPU): the merger of roskfpos_amd.synth builds the slots the header describes; the
fixed schedule and participation mask that tests/test_planar_events_each_gpu.py replays hold what they are meant to
hold; and over that schedule, with the per-tag timeLags, the oracle and the host build of the kernel body (PlanarEmu)
agree after every slot within the bounds of tests/test_planar_events_schedule.py."""
import numpy as np
import pytest

import planar_events as pe
import planar_events_each as pee
from planar import PlanarEmu, PlanarOracle
from roskfpos_amd import synth

T = pee.T
RMS_BOUND, MAX_BOUND = 1e-9, 1e-8   # tests/test_planar_events_schedule.py


def _lines():
    """four robots: different periods, phases and sensor rates"""
    return [synth.planar_tag_timeline(0.10, 0.000, 3, n_imu=4, n_px4=2, n_mag=1),
            synth.planar_tag_timeline(0.10, 0.013, 3, n_imu=4, n_px4=1, n_mag=0, n_compass=1),
            synth.planar_tag_timeline(0.07, 0.000, 4, n_imu=2, n_px4=0, n_mag=1),
            synth.planar_tag_timeline(0.10, 0.000, 2, n_imu=4, n_px4=2, n_mag=1)]


def test_the_merger_builds_the_slots_of_the_call():
    lines = _lines()
    s = synth.merge_planar_timelines(lines)
    E = s.kinds.size
    assert s.dt.shape == s.ordinal.shape == (E, 4) and s.time.shape == (E,)
    assert np.array_equal(s.present, s.ordinal >= 0) and (s.dt[~s.present] == -1.0).all()
    assert set(s.kinds.tolist()) == {0, 1, 2, 3, 4}
    for t, line in enumerate(lines):
        # every event of the tag is in exactly one slot, in its own order; its dts add up to the time of its last event
        assert int(s.present[:, t].sum()) == len(line)
        at = np.flatnonzero(s.present[:, t])
        assert [(int(s.kinds[e]), int(s.ordinal[e, t])) for e in at] == [(ev[1], ev[2]) for ev in line]
        assert abs(s.dt[at, t].sum() - line[-1][0]) < 1e-12
        assert np.allclose(np.cumsum(s.dt[at, t]), [ev[0] for ev in line], atol=1e-12)
    assert (np.diff(s.time) >= 0).all()
    # tags 0 and 3 share a clock: they share every slot of tag 3's two periods
    assert (s.present[:, 0] >= s.present[:, 3]).all()
    # at one instant: sensor slots in kind order 1..4 ahead of the ranging slot
    same = [(a, b) for a, b in zip(range(E - 1), range(1, E)) if s.time[a] == s.time[b]]
    for a, b in same:
        assert s.kinds[a] != 0 and (s.kinds[b] == 0 or s.kinds[a] < s.kinds[b])


def test_the_ordering_rule_at_one_instant_and_tick_merging():
    # five robots, one event each at t = 0.5 (to within the tick), one kind each, handed over in the wrong order
    lines = [[(0.5, 0, 0)], [(0.5 + 2e-10, 4, 0)], [(0.5, 2, 0)], [(0.5 - 3e-10, 1, 0)], [(0.5, 3, 0)]]
    s = synth.merge_planar_timelines(lines, tick=1e-9)
    assert s.kinds.tolist() == [1, 2, 3, 4, 0]
    assert s.present.sum(axis=1).tolist() == [1] * 5
    # two robots whose IMU samples agree to the tick share a slot, a third one 3 ticks later has a slot of its own
    lines = [[(0.25, 2, 0), (0.5, 0, 0)], [(0.25 + 4e-10, 2, 0), (0.5, 0, 0)], [(0.25 + 3e-9, 2, 0), (0.5 + 3e-9, 0, 0)]]
    s = synth.merge_planar_timelines(lines, tick=1e-9)
    assert s.kinds.tolist() == [2, 2, 0, 0]
    assert s.present.tolist() == [[True, True, False], [False, False, True], [True, True, False], [False, False, True]]
    assert s.dt[0, 1] == 0.25 + 4e-10               # the tag's own time, not the slot's
    assert synth.merge_planar_timelines(lines, tick=1e-8).kinds.tolist() == [2, 0]     # a coarser tick merges all three


def test_events_of_a_tag_inside_one_tick_never_get_a_negative_dt():
    # a sensor sample 2e-10 s BEHIND a ranging epoch, same quantum: the sensor slot comes first, and the ranging slot
    # that follows it gets dt = 0.0 -- a negative dt would read as "absent" and lose the event
    line = [(0.25, 2, 0), (0.5, 0, 0), (0.5 + 2e-10, 3, 0), (0.75, 2, 1)]
    s = synth.merge_planar_timelines([line], tick=1e-9)
    assert s.kinds.tolist() == [2, 3, 0, 2] and s.present.all()
    assert s.dt[:, 0].tolist() == [0.25, 0.25 + 2e-10, 0.0, 0.75 - (0.5 + 2e-10)]
    assert abs(s.dt.sum() - 0.75) < 1e-15


def test_two_events_of_a_tag_in_one_slot_are_refused():
    with pytest.raises(ValueError, match="two events in one slot"):
        synth.merge_planar_timelines([[(0.25, 2, 0), (0.25 + 2e-10, 2, 1), (0.5, 0, 0)]], tick=1e-9)
    with pytest.raises(ValueError):
        synth.merge_planar_timelines([[(0.25, 5, 0)]])


def test_an_all_equal_bank_merges_to_the_shared_timeline_schedule():
    line = synth.planar_tag_timeline(0.1, 0.0, 3)           # 10 IMU + 2 PX4Flow + 1 magnetometer + ranging
    s = synth.merge_planar_timelines([line] * 6)
    assert s.kinds.tolist() == [ev[1] for ev in line] and s.kinds.size == 3 * 14
    assert s.present.all()
    times = np.array([ev[0] for ev in line])
    assert np.allclose(s.dt, np.diff(times, prepend=0.0)[:, None], atol=1e-15) and (s.dt == s.dt[:, :1]).all()
    assert (s.ordinal == s.ordinal[:, :1]).all()
    assert (np.bincount(s.kinds, minlength=5) == [3, 6, 30, 3, 0]).all()


def test_the_slot_inputs_hold_each_tags_own_sample():
    w = synth.Workload(4, 8)
    s = synth.merge_planar_timelines(_lines())
    inp = synth.planar_slot_inputs(w, s)
    n = [0] * 5
    for e, kind in enumerate(s.kinds):
        a = inp[int(kind)][n[kind]]
        n[kind] += 1
        for t in range(4):
            if s.present[e, t]:
                own = w.ranges_mm(int(s.ordinal[e, t])) if kind == 0 else synth.planar_sample(w, int(kind), int(s.ordinal[e, t]))
                assert np.array_equal(a[t], own[t]), (e, t)
            else:
                assert (a[t] == -1).all() if kind == 0 else np.isnan(a[t]).all(), (e, t)
    assert [inp[k].shape[0] for k in range(5)] == n
    assert inp[0].dtype == np.int32 and inp[2].shape[1:] == (4, 24)


def test_the_schedule_holds_what_it_is_meant_to_hold():
    k = pe.kinds_of(True)
    m = pee.mask_of(k)
    E = k.size
    assert T == 130 and m.shape == (E, T) and E == 40 and set(k.tolist()) == {0, 1, 2, 3, 4}
    assert m[:, pee.EVERYWHERE].all() and not m[:, pee.NOWHERE].any()
    for kind in range(5):                       # the second wavefront sits a slot of every kind out ...
        out = [e for e in np.flatnonzero(k == kind) if not m[e, 64:128].any()]
        assert out, kind
        assert m[out, :64].any(axis=1).all()    # ... while the first one runs it
    assert 0.50 <= m.mean() <= 0.75, m.mean()
    es = pee.EachSchedule(8)
    assert np.array_equal(es.mask, m) and np.array_equal(es.dt < 0, ~m) and (es.dt[m] > 0).all()   # dt = 0 stays out
    assert es.ran[:, :64].any(axis=1).all()     # somebody of tags 0..63 RUNS every slot: present and not dropped
    assert es.ran[:, 128:].any() and not es.ran[:, 128:].all()
    px4 = k == pe.PX4
    assert (es.dropped[px4] & m[px4]).any() and (es.dropped[px4] & ~m[px4]).any()     # quality 0: present, and absent
    assert not es.dropped[~px4].any()
    # what absent and dropped pairs hold
    n = [0] * 5
    for e, kind in enumerate(k):
        i, n[kind] = n[kind], n[kind] + 1
        if kind == pe.TOA:
            assert (es.ranges[i][~m[e]] == pee.ABSENT_MM).all() and (es.ranges[i][m[e]] != pee.ABSENT_MM).all()
        else:
            assert np.isnan(es.samples[kind][i][~m[e]]).all()
            keep = m[e] & ~es.dropped[e]
            assert np.isfinite(es.samples[kind][i][keep]).all()
            if kind == pe.PX4:
                gone = m[e] & es.dropped[e]
                assert np.isnan(es.samples[kind][i][gone, :4]).all() and (es.samples[kind][i][gone, 4] == 0).all()
    # first sensor sample behind the first ranging slot, and the other way round
    first = lambda t, sel: int(np.flatnonzero(m[:, t] & sel)[0])  # noqa: E731
    assert first(pee.EVERYWHERE, k == pe.TOA) < first(pee.EVERYWHERE, k != pe.TOA)
    assert first(pee.SENSOR_FIRST, k != pe.TOA) < first(pee.SENSOR_FIRST, k == pe.TOA)
    # launches of 7 slots (the slots ahead of the first sensor slot go down the ranging path): a boundary between two
    # sensor slots, another directly before a ranging slot
    for kinds in (k, pe.kinds_of(False)):
        starts = pe.launch_starts(kinds, 7)[1:]
        assert any(kinds[s - 1] != pe.TOA and kinds[s] != pe.TOA for s in starts), "no boundary between sensor slots"
        assert any(kinds[s] == pe.TOA for s in starts), "no boundary directly before a ranging slot"
    # the single-tag test takes column 1: it skips slots and runs slots
    assert 0 < m[:, 1].sum() < E
    # the waiting prefix: tags that run sensor slots ahead of their first ranging
    mw = pee.mask_of(pe.kinds_of(True, waiting=True))
    assert mw[:2].any(axis=0).sum() > 64 and not mw[:2].all(axis=0).all()


@pytest.mark.parametrize("A", [8, 5])
@pytest.mark.parametrize("start", ["fixed", "ml3d", "ml2d"])
def test_oracle_and_host_build_agree_over_the_schedule(start, A):
    es = pee.EachSchedule(A, end_on_sensor=True, waiting=start != "fixed")
    sch = es.sch
    cfg, init = pe.cfg_of(start), pe.init_of(sch, start)
    po, so = pee.replay(PlanarOracle(sch.w, cfg, init), es)
    pg, sg = pee.replay(PlanarEmu(sch.w, cfg, init, sensors=True), es)
    worst = [0.0, 0.0]
    for e in range(es.kinds.size):
        assert np.array_equal(so[e], sg[e]), (e, "status words")
        assert np.array_equal(so[e] == pee.ST_SKIPPED, ~es.ran[e]), (e, "who sits the slot out")
        rms, mx, same_waiting = pe.distance(pg[e], po[e])
        worst = [max(worst[0], rms), max(worst[1], mx)]
        assert same_waiting, e
        assert rms <= RMS_BOUND and mx <= MAX_BOUND, (e, rms, mx)
        if e:                                   # a tag that sat the slot out is where it was
            out = ~es.ran[e]
            assert po[e][out].tobytes() == po[e - 1][out].tobytes() and pg[e][out].tobytes() == pg[e - 1][out].tobytes()
    print(f"start={start} A={A}: worst RMS {worst[0]:.3e} m, worst max {worst[1]:.3e} m over {es.kinds.size} slots")
    low = so[es.ran] & 0xFF
    assert (low == 0).mean() > 0.5 and (low & 0x04).any()       # most events are plain; too few ranges happened
    if start != "fixed":
        assert (low & 0x08).any()                               # ML initialisations
    started = np.isfinite(po[-1]).all(axis=1)
    assert started[np.arange(T) != pee.NOWHERE].all() and (start != "fixed" or started.all())
