"""The schedule that tests/test_planar_events_gpu.py replays holds what it is meant to hold (no GPU): the oracle and the
host build of the kernel body (PlanarEmu) agree on every status word over it, the dropout, few-ranges, ML-start and
dropped-sample paths all run, the positions stay within the bounds the GPU test applies, and with launches of 7 events
one launch boundary falls between two sensor events and one directly before a ranging event."""
import numpy as np
import pytest

import planar_events as pe
from planar import PlanarEmu, PlanarOracle

T = 130
RMS_BOUND, MAX_BOUND = 1e-9, 1e-8   # tests/test_gpu_parity.py, as tests/test_run_events_gpu.py takes them


def test_the_schedule_holds_what_it_is_meant_to_hold():
    k = pe.kinds_of(True)
    assert k.size == 40 and k[0] == pe.TOA and k[-1] == pe.MAG
    assert set(k.tolist()) == {0, 1, 2, 3, 4}
    assert pe.kinds_of(False).size == 38 and pe.kinds_of(False)[-1] == pe.TOA
    kw = pe.kinds_of(True, waiting=True)
    assert kw.size == 42 and list(kw[:3]) == [pe.IMU, pe.PX4, pe.TOA]
    assert any(k[e] == pe.TOA and k[e + 1] == pe.TOA for e in range(k.size - 1))        # two rangings back to back
    assert any(k[e] == pe.PX4 and k[e + 1] == pe.PX4 for e in range(k.size - 1))
    assert any(k[e] == pe.COMPASS and pe.PX4 in k[:e] and pe.IMU in k[:e] for e in range(k.size))
    for kinds in (k, pe.kinds_of(False)):
        starts = pe.launch_starts(kinds, 7)[1:]       # KFPOS_TRACE_CHUNK_STEPS=7
        assert any(kinds[s - 1] != pe.TOA and kinds[s] != pe.TOA for s in starts), "no boundary between sensor events"
        assert any(kinds[s] == pe.TOA for s in starts), "no boundary directly before a ranging event"
    sch = pe.Schedule(T, 8)
    assert (sch.dts > 0).all()                         # dt = 0 stays out of the oracle leg
    n_drop = int(sch.dropped().sum())
    assert 58 <= n_drop <= 66, n_drop
    eps = range(int((k == pe.TOA).sum()))
    assert any(s % 7 == 3 for s in eps) and any(s % 11 == 5 for s in eps) and any(s % 13 == 6 for s in eps)


@pytest.mark.parametrize("A", [8, 5])
@pytest.mark.parametrize("start", ["fixed", "ml3d", "ml2d"])
def test_oracle_and_host_build_agree_over_the_schedule(start, A):
    sch = pe.Schedule(T, A, end_on_sensor=True, waiting=start != "fixed")
    cfg, init = pe.cfg_of(start), pe.init_of(sch, start)
    po, so = pe.replay(PlanarOracle(sch.w, cfg, init), sch)
    pg, sg = pe.replay(PlanarEmu(sch.w, cfg, init, sensors=True), sch)
    worst = [0.0, 0.0]
    for e in range(sch.kinds.size):
        assert np.array_equal(so[e], sg[e]), (e, "status words")
        rms, mx, same_waiting = pe.distance(pg[e], po[e])
        worst = [max(worst[0], rms), max(worst[1], mx)]
        assert same_waiting, e
        assert rms <= RMS_BOUND and mx <= MAX_BOUND, (e, rms, mx)
    print(f"start={start} A={A}: worst RMS {worst[0]:.3e} m, worst max {worst[1]:.3e} m over {sch.kinds.size} events")
    low = so & 0xFF
    assert (low == 0).mean() > 0.5
    assert (low & 0x40).any() and np.array_equal((low & 0x40) != 0, sch.dropped())      # dropped PX4Flow samples
    assert (low & 0x04).any()                                                           # too few ranges
    if start != "fixed":
        assert (low & 0x08).any()                                                       # ML initialisations
        assert np.isnan(po[1][:, :2]).all()        # the two sensor events ahead of the first ranging leave every tag waiting
    assert np.isfinite(po[-1]).all()         # every tag has started by the end
