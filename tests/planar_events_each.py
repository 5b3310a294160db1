"""The schedule of the kfpos_run_planar_events_each_dev tests: the kinds and inputs of tests/planar_events.py, an explicit
participation mask over 130 tags (who takes part in which slot), the per-tag timeLags that follow from it (-1.0 = the
tag sits the slot out), and the replay of it through anything with the five entry points of the planar filter (oracle,
host emulation), which all take a per-tag dt array with negative = absent.

tests/test_planar_events_each_schedule.py asserts on the CPU that the mask holds what it is meant to hold."""
import numpy as np

import planar_events as pe

T = 130                      # two full wavefronts and one of two lanes
EVERYWHERE, NOWHERE = 0, 5   # a tag present in every slot, a tag in none
SENSOR_FIRST = 7             # a tag whose first sensor sample comes ahead of its first ranging slot
ABSENT_MM = 1999999999       # what the ranges of an absent (tag, slot) pair hold
ST_SKIPPED = 64


def mask_of(kinds):
    """(E, T) bool: who takes part in which slot"""
    E = kinds.size
    m = np.random.default_rng(20261019).random((E, T)) < 0.65
    m[:, EVERYWHERE] = True
    m[:, NOWHERE] = False
    # the second wavefront sits out the first slot of each kind that has an earlier slot of the call ahead of it
    for kind in range(5):
        at = [e for e in np.flatnonzero(kinds == kind) if e > 0]
        m[at[0], 64:128] = False
    # tag SENSOR_FIRST: absent from every ranging slot ahead of its first sensor slot
    sensor = [e for e in range(E) if kinds[e] != pe.TOA and m[e, SENSOR_FIRST]]
    m[:sensor[0], SENSOR_FIRST] = False
    return m


class EachSchedule:
    """pe.Schedule plus the mask: dt (E, T) per-tag timeLags, and the inputs as the GPU gets them, in which absent pairs
    and dropped PX4Flow samples hold NaN / ABSENT_MM (a dropped sample keeps its quality 0: that is what drops it)"""

    def __init__(self, A, end_on_sensor=True, waiting=False, real=np.float64, kinds=None, fill=True):
        sch = self.sch = pe.Schedule(T, A, end_on_sensor, waiting, real)
        if kinds is not None:   # another kinds pattern over the same inputs: every kind has at least as many samples
            kinds = np.asarray(kinds, dtype=np.uint8)
            assert all((kinds == k).sum() <= (sch.kinds == k).sum() for k in range(5))
            sch.kinds, sch.dts = kinds, sch.dts[:kinds.size]
        self.kinds, self.base = sch.kinds, sch.dts.copy()
        self.mask = mask_of(self.kinds)
        self.dt = np.where(self.mask, self.base[:, None], -1.0)
        self.dropped = sch.dropped()                      # (E, T): PX4Flow quality 0, present or not
        self.ran = self.mask & ~self.dropped              # who runs the slot's event
        self.ranges = sch.ranges.copy()
        self.samples = {k: v.copy() for k, v in sch.samples.items()}
        if fill:
            for e, kind, i, _ in sch.events():
                out = ~self.mask[e]
                if kind == pe.TOA:
                    self.ranges[i][out] = ABSENT_MM
                else:
                    self.samples[kind][i][out] = np.nan
                    if kind == pe.PX4:
                        gone = self.mask[e] & self.dropped[e]
                        self.samples[kind][i][gone, :4] = np.nan


def replay(impl, es):
    """the schedule through an implementation's entry points with the per-tag dts -> (position (x, y, height) after
    every slot [n][T][3], status of every slot [n][T]). The implementations get the inputs as they were before absent
    pairs were filled: they skip on dt < 0 as the library does, and tidy numbers keep their own checks quiet."""
    sch = es.sch
    pos, st = [], []
    err = sch.err.astype(np.float64)
    for e, kind, i, _ in sch.events():
        dt = es.dt[e]
        if kind == pe.TOA:
            s = impl.step_toa(sch.ranges[i], err, dt)
        elif kind == pe.PX4:
            s = impl.step_px4flow(sch.samples[pe.PX4][i], dt)
        elif kind == pe.IMU:
            d = sch.samples[pe.IMU][i]
            s = impl.step_planar_imu(d[:, 0:3], d[:, 3:12], d[:, 12:15], d[:, 15:24], dt)
        elif kind == pe.MAG:
            s = impl.step_mag(sch.samples[pe.MAG][i], dt)
        else:
            s = impl.step_compass(sch.samples[pe.COMPASS][i][:, 0], dt)
        st.append(np.asarray(s, dtype=np.uint32).copy())
        pos.append(np.concatenate([impl.get_state()[0][:, :2], impl.get_height()[:, None]], axis=1))
    return np.stack(pos), np.stack(st)
