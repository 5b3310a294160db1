"""Synthetic UWB ranging / IMU traces for the batched EKF core.

The reference has no data sets; this is the workload BASELINE.md section 3 defines:
anchors on the corners of a 10 x 10 x (0.3..3.0) m room (+8 interior anchors for the
16-anchor case), per-tag circular trajectories, ranges = true distance + N(0, 0.05^2) m
floored to integer millimetres exactly as the node does (Posgenerator.cpp:213, :484),
errorEstimation = 0.0025 m^2, accel = true acceleration + N(0, 0.1^2), covariance 0.01*I,
dt = 0.05 s with the reference's hard-coded 0.1 s first step (KalmanFilterTOA.cpp:81).

Every draw is a pure function of (seed, global tag index, step, channel) through a
counter-based SplitMix64 hash, so any shard of the tag batch regenerates its own inputs
without seeing the others (multi-GPU sharding).
"""
from __future__ import annotations

import numpy as np

SEED = 12345
DT = 0.05
DT_FIRST = 0.1
RANGE_SIGMA = 0.05
ERR_EST = 0.0025
ACC_SIGMA = 0.1
ACC_COV = 0.01
_CH_PER_STEP = np.uint64(256)
_SUB_BASE = np.uint64(1 << 40)  # counters of the samples between two ranging epochs (accel_between): beyond any step's channels
_SUB_PER_STEP = 64
_GOLD = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def anchors_xyz(n_anchors: int) -> np.ndarray:
    """Anchor table (A, 3) float64: 8 room corners, 8 interior anchors, then -- only for
    tests of large anchor counts, up to MAX_NUM_ANCS = 64 -- a second ring."""
    if not 1 <= n_anchors <= 64:
        raise ValueError("synthetic anchor layout is defined for 1..64 anchors")
    out = np.zeros((64, 3))
    for i in range(8):
        out[i] = (10.0 * (i & 1), 10.0 * ((i >> 1) & 1), 0.3 + 2.7 * ((i >> 2) & 1))
    for i in range(8, 16):
        out[i] = (5.0 + 3.0 * np.cos(float(i)), 5.0 + 3.0 * np.sin(float(i)), 1.5 + 0.1 * i)
    for i in range(16, 64):
        out[i] = (5.0 + 4.5 * np.cos(0.7 * i), 5.0 + 4.5 * np.sin(0.7 * i), 0.4 + 0.04 * i)
    return out[:n_anchors].copy()


def _mix(z: np.ndarray) -> np.ndarray:
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def _tag_key(tags: np.ndarray, seed: int) -> np.ndarray:
    with np.errstate(over="ignore"):
        return _mix(np.uint64(seed) ^ _mix(tags.astype(np.uint64) * _GOLD + np.uint64(1)))


def _uniform(key: np.ndarray, counter) -> np.ndarray:
    """U[0,1) with 53 random bits; key (T,) broadcast against counter."""
    with np.errstate(over="ignore"):
        u = _mix(key + _GOLD * np.asarray(counter, dtype=np.uint64))
    return (u >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def _normal(key: np.ndarray, counter) -> np.ndarray:
    c = np.asarray(counter, dtype=np.uint64)
    u1 = 1.0 - _uniform(key, c)  # (0, 1]
    u2 = _uniform(key, c + np.uint64(1))
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


class Workload:
    """Deterministic trace for global tags [tag0, tag0 + n_tags)."""

    def __init__(self, n_tags: int, n_anchors: int = 8, tag0: int = 0, seed: int = SEED):
        self.n_tags, self.n_anchors, self.tag0, self.seed = n_tags, n_anchors, tag0, seed
        self.anchors = anchors_xyz(n_anchors)
        tags = np.arange(tag0, tag0 + n_tags, dtype=np.uint64)
        self._key = _tag_key(tags, seed)
        self.rho = 1.0 + 3.0 * _uniform(self._key, 0)
        self.omega = 0.1 + 0.3 * _uniform(self._key, 1)
        self.phi = 2.0 * np.pi * _uniform(self._key, 2)

    # -- ground truth ------------------------------------------------------------
    @staticmethod
    def time_of(step: int) -> float:
        """Time stamp of ranging epoch `step` (step 0 happens DT_FIRST after t = 0)."""
        return DT_FIRST + DT * step

    @staticmethod
    def dt_of(step: int) -> float:
        return DT_FIRST if step == 0 else DT

    def position(self, t: float) -> np.ndarray:
        ang = self.omega * t + self.phi
        return np.stack([5.0 + self.rho * np.cos(ang), 5.0 + self.rho * np.sin(ang),
                         1.0 + 0.2 * np.sin(0.1 * t + self.phi)], axis=1)

    def acceleration(self, t: float) -> np.ndarray:
        ang = self.omega * t + self.phi
        w2 = self.omega * self.omega
        return np.stack([-self.rho * w2 * np.cos(ang), -self.rho * w2 * np.sin(ang),
                         -0.2 * 0.01 * np.sin(0.1 * t + self.phi)], axis=1)

    def init_positions(self) -> np.ndarray:
        """Fixed start = true position at t = 0 (P0 = 0), shape (T, 3)."""
        return self.position(0.0)

    # -- measurements ------------------------------------------------------------
    def ranges_mm(self, step: int) -> np.ndarray:
        """(T, A) int32 millimetres, the node's wire format (floor(), Posgenerator.cpp:213)."""
        p = self.position(self.time_of(step))
        d = np.sqrt(((p[:, None, :] - self.anchors[None, :, :]) ** 2).sum(-1))
        base = np.uint64(step + 1) * _CH_PER_STEP
        ch = base + np.uint64(2) * np.arange(self.n_anchors, dtype=np.uint64)
        noise = _normal(self._key[:, None], ch[None, :])
        return np.floor((d + RANGE_SIGMA * noise) * 1000.0).astype(np.int32)

    def err_est(self, dtype=np.float64) -> np.ndarray:
        return np.full((self.n_tags, self.n_anchors), ERR_EST, dtype=dtype)

    def accel(self, step: int, dtype=np.float64) -> np.ndarray:
        """(T, 3) accelerometer sample for epoch `step`."""
        a = self.acceleration(self.time_of(step))
        base = np.uint64(step + 1) * _CH_PER_STEP + np.uint64(200)
        ch = base + np.uint64(2) * np.arange(3, dtype=np.uint64)
        return (a + ACC_SIGMA * _normal(self._key[:, None], ch[None, :])).astype(dtype)

    def accel_between(self, step: int, sub: int, n_sub: int, dtype=np.float64) -> np.ndarray:
        """(T, 3) accelerometer sample `sub` (0 .. n_sub - 1) of the n_sub that an IMU running faster than the ranging
        delivers between ranging epochs step - 1 and step, evenly spaced: sample sub is taken dt_of(step) * (sub + 1) /
        (n_sub + 1) after epoch step - 1 (each of the n_sub + 1 events of the period then has that fraction of dt_of(step)
        as its timeLag). Noise counters of its own, above every per-step channel: accel(), ranges_mm() and the planar
        sensors draw exactly what they drew before."""
        if not (0 <= sub < n_sub <= _SUB_PER_STEP):
            raise ValueError("0 <= sub < n_sub <= %d" % _SUB_PER_STEP)
        t = self.time_of(step) - self.dt_of(step) * (n_sub - sub) / (n_sub + 1)
        base = _SUB_BASE + (np.uint64(step + 1) * np.uint64(_SUB_PER_STEP) + np.uint64(sub)) * np.uint64(8)
        ch = base + np.uint64(2) * np.arange(3, dtype=np.uint64)
        return (self.acceleration(t) + ACC_SIGMA * _normal(self._key[:, None], ch[None, :])).astype(dtype)

    def accel_cov(self, dtype=np.float64) -> np.ndarray:
        """(T, 9) row-major 3x3 accelerometer covariance."""
        return np.tile((ACC_COV * np.eye(3)).reshape(1, 9), (self.n_tags, 1)).astype(dtype)

    def trace(self, n_steps: int, step0: int = 0):
        """ranges (S, T, A) int32, accel (S, T, 3) float64, dt (S,) float64."""
        r = np.stack([self.ranges_mm(s) for s in range(step0, step0 + n_steps)])
        a = np.stack([self.accel(s) for s in range(step0, step0 + n_steps)])
        dt = np.array([self.dt_of(s) for s in range(step0, step0 + n_steps)])
        return r, a, dt

    # -- planar filter sensors (KalmanFilter: PX4Flow, IMU, magnetometer, compass) -----------------
    # The vehicle heads along its velocity: heading = trajectory angle + pi/2, yaw rate = omega. Sensor frames
    # follow KalmanFilter::px4flowOutput / imuOutput (KalmanFilter.cpp:558-576): body = R(-heading) * world.
    PX4_HEIGHT = 0.8        # <px4flow sensorHeight/>
    PX4_TIME_US = 50000.0   # integration time of one flow sample
    PX4_SIGMA = 0.02
    GYRO_SIGMA = 0.01
    MAG_SIGMA = 0.02

    def heading(self, t: float) -> np.ndarray:
        return self.omega * t + self.phi + 0.5 * np.pi

    def velocity(self, t: float) -> np.ndarray:
        ang = self.omega * t + self.phi
        return np.stack([-self.rho * self.omega * np.sin(ang), self.rho * self.omega * np.cos(ang),
                         0.02 * np.cos(0.1 * t + self.phi)], axis=1)

    def _body(self, t: float, v: np.ndarray) -> np.ndarray:
        th = self.heading(t)
        c, s = np.cos(th), np.sin(th)
        return np.stack([c * v[:, 0] + s * v[:, 1], -s * v[:, 0] + c * v[:, 1]], axis=1)

    def _noise(self, step: int, base_channel: int, n: int) -> np.ndarray:
        base = np.uint64(step + 1) * _CH_PER_STEP + np.uint64(base_channel)
        ch = base + np.uint64(2) * np.arange(n, dtype=np.uint64)
        return _normal(self._key[:, None], ch[None, :])

    def px4flow(self, step: int) -> np.ndarray:
        """(T, 5): integrationX, integrationY, integrationRotationZ, integrationTime [us], quality -- the
        arguments of newPX4FlowMeasurement (KalmanFilter.cpp:102). Every 16th tag reports quality 0."""
        t = self.time_of(step)
        vb = self._body(t, self.velocity(t)) + self.PX4_SIGMA * self._noise(step, 210, 2)
        sec = self.PX4_TIME_US / 1e6
        gz = self.omega + self.GYRO_SIGMA * self._noise(step, 216, 1)[:, 0]
        q = np.where((np.arange(self.tag0, self.tag0 + self.n_tags) + step) % 16 == 5, 0.0, 200.0)
        return np.stack([vb[:, 0] * sec / self.PX4_HEIGHT, vb[:, 1] * sec / self.PX4_HEIGHT, gz * sec,
                         np.full(self.n_tags, self.PX4_TIME_US), q], axis=1)

    def planar_imu(self, step: int):
        """angular velocity (T, 3) and body-frame linear acceleration (T, 3) for newIMUMeasurement."""
        t = self.time_of(step)
        ab = self._body(t, self.acceleration(t)) + ACC_SIGMA * self._noise(step, 220, 2)
        w = np.zeros((self.n_tags, 3))
        w[:, 2] = self.omega + self.GYRO_SIGMA * self._noise(step, 226, 1)[:, 0]
        a = np.concatenate([ab, np.full((self.n_tags, 1), 9.81)], axis=1)
        return w, a

    def mag(self, step: int) -> np.ndarray:
        """(T, 3) magnetometer vector whose atan2(y, x) is the heading."""
        th = self.heading(self.time_of(step)) + self.MAG_SIGMA * self._noise(step, 230, 1)[:, 0]
        return np.stack([np.cos(th), np.sin(th), np.full(self.n_tags, -0.4)], axis=1)

    def compass(self, step: int) -> np.ndarray:
        """(T,) compass heading in radians, unwrapped on purpose (newCompassMeasurement normalises once)."""
        return self.heading(self.time_of(step)) + self.MAG_SIGMA * self._noise(step, 234, 1)[:, 0]


# -- per-tag timelines merged into event slots (kfpos_run_events_each_dev) ---------------------------------
class EachSchedule:
    """What merge_timelines returns. E slots, T tags:
    kinds (E,) uint8        0 = IMU slot, 1 = TOA slot (capi.EVENT_IMU / EVENT_TOA)
    dt    (E, T) float64    the tag's timeLag in the slot: time since its own previous event; -1.0 where it is absent
    step  (E, T) int32      the Workload step (ranging period) the tag's event belongs to; -1 where it is absent
    sub   (E, T) int32      IMU slots: which of the period's n_sub[t] samples (Workload.accel_between); -1 otherwise
    n_sub (T,)   int32      IMU samples per ranging period of every tag
    time  (E,)   float64    the instant of the slot"""

    def __init__(self, kinds, dt, step, sub, n_sub, time):
        self.kinds, self.dt, self.step, self.sub, self.n_sub, self.time = kinds, dt, step, sub, n_sub, time

    @property
    def present(self):
        return ~(self.dt < 0.0)


def tag_timeline(period: float, n_sub: int, phase: float, n_periods: int):
    """One tag's own event sequence: [(time, kind, step, sub)], n_periods ranging periods of `period` seconds that
    start `phase` seconds after t = 0, each with n_sub evenly spaced IMU samples ahead of its ranging epoch (the
    spacing of Workload.accel_between)."""
    out = []
    for p in range(n_periods):
        for i in range(n_sub):
            out.append((phase + period * (p + (i + 1) / (n_sub + 1)), 0, p, i))
        out.append((phase + period * (p + 1), 1, p, -1))
    return out


def merge_timelines(period, n_sub, phase, n_periods: int, tick: float = 1e-9) -> EachSchedule:
    """Merge per-tag timelines (tag_timeline of period[t], n_sub[t], phase[t]; scalars broadcast) into the slots of
    kfpos_run_events_each_dev. Events of the same kind whose times agree to `tick` seconds share a slot; slots are
    ordered by time, an IMU slot ahead of a TOA slot of the same instant. A tag's dt in a slot is the time since its own
    previous event (its first: since t = 0), so its dts add up to the time of its last event."""
    n_sub = np.atleast_1d(np.asarray(n_sub, dtype=np.int32))
    T = max(np.size(period), n_sub.size, np.size(phase))
    period = np.broadcast_to(np.asarray(period, dtype=np.float64), (T,))
    phase = np.broadcast_to(np.asarray(phase, dtype=np.float64), (T,))
    n_sub = np.broadcast_to(n_sub, (T,)).copy()
    lines = [tag_timeline(float(period[t]), int(n_sub[t]), float(phase[t]), n_periods) for t in range(T)]
    key = lambda ev: (int(round(ev[0] / tick)), ev[1])  # noqa: E731
    slots = sorted({key(ev) for line in lines for ev in line})
    index = {k: e for e, k in enumerate(slots)}
    E = len(slots)
    dt = np.full((E, T), -1.0)
    step = np.full((E, T), -1, dtype=np.int32)
    sub = np.full((E, T), -1, dtype=np.int32)
    for t, line in enumerate(lines):
        prev = 0.0
        for ev in line:
            e = index[key(ev)]
            if step[e, t] >= 0:
                raise ValueError("tag %d has two events in one slot: its samples are closer than `tick`" % t)
            dt[e, t], step[e, t], sub[e, t] = ev[0] - prev, ev[2], ev[3]
            prev = ev[0]
    kinds = np.array([k for _, k in slots], dtype=np.uint8)
    time = np.array([q for q, _ in slots], dtype=np.float64) * tick
    return EachSchedule(kinds, dt, step, sub, n_sub, time)


def slot_inputs(w: "Workload", sched: EachSchedule, dtype=np.float64, epoch=None, absent_mm: int = -1):
    """The inputs of a merged schedule in slot order: ranges (J, T, A) int32 of the J TOA slots, accel (I, T, 3) of the
    I IMU slots. Every participating tag reads its own step / sub-sample (sched.step, sched.sub); entries of absent
    tags are `absent_mm` / NaN. epoch(w, step) -> (T, A) replaces w.ranges_mm (tests: cases.Case.epoch)."""
    epoch = epoch or (lambda w_, s: w_.ranges_mm(s))
    T, A = w.n_tags, w.n_anchors
    rows = np.arange(T)
    ranges, accel = [], []
    for e, kind in enumerate(sched.kinds):
        here = sched.step[e] >= 0
        if kind == 1:
            r = np.full((T, A), absent_mm, dtype=np.int32)
            for s in np.unique(sched.step[e][here]):
                m = here & (sched.step[e] == s)
                r[m] = epoch(w, int(s))[rows[m]]
            ranges.append(r)
        else:
            a = np.full((T, 3), np.nan, dtype=dtype)
            combos = {(int(s), int(i), int(k)) for s, i, k in zip(sched.step[e][here], sched.sub[e][here], sched.n_sub[here])}
            for s, i, k in sorted(combos):
                m = here & (sched.step[e] == s) & (sched.sub[e] == i) & (sched.n_sub == k)
                a[m] = w.accel_between(s, i, k, dtype)[rows[m]]
            accel.append(a)
    J = np.stack(ranges) if ranges else np.zeros((0, T, A), dtype=np.int32)
    I = np.stack(accel) if accel else np.zeros((0, T, 3), dtype=dtype)  # noqa: E741
    return J, I


# -- per-tag timelines of the planar filter merged into event slots (kfpos_run_planar_events_each_dev) ------
PLANAR_WIDTH = {1: 5, 2: 24, 3: 3, 4: 1}   # components of a PX4Flow / IMU / magnetometer / compass sample


class PlanarEachSchedule:
    """What merge_planar_timelines returns. E slots, T tags:
    kinds   (E,)   uint8     0 = ranging slot, 1..4 = PX4Flow / IMU / magnetometer / compass slot
    dt      (E, T) float64   the tag's timeLag in the slot: time since its own previous event; -1.0 where it is absent
    ordinal (E, T) int32     which of the tag's OWN samples of that kind the slot carries; -1 where it is absent
    time    (E,)   float64   the instant of the slot"""

    def __init__(self, kinds, dt, ordinal, time):
        self.kinds, self.dt, self.ordinal, self.time = kinds, dt, ordinal, time

    @property
    def present(self):
        return ~(self.dt < 0.0)


def planar_tag_timeline(period: float, phase: float, n_periods: int, n_imu: int = 10, n_px4: int = 2, n_mag: int = 1,
                        n_compass: int = 0):
    """One robot's own event sequence: [(time, kind, ordinal of its own sample of that kind)], n_periods ranging
    periods of `period` seconds that start `phase` seconds after t = 0; inside each, every sensor's samples are evenly
    spaced ahead of the period's ranging epoch (sample i of n at (i + 1) / (n + 1) of the period)."""
    out = []
    for p in range(n_periods):
        inside = []
        for kind, n in ((1, n_px4), (2, n_imu), (3, n_mag), (4, n_compass)):
            inside += [(phase + period * (p + (i + 1) / (n + 1)), kind, p * n + i) for i in range(n)]
        out += sorted(inside, key=lambda ev: (ev[0], ev[1]))
        out.append((phase + period * (p + 1), 0, p))
    return out


def merge_planar_timelines(lines, tick: float = 1e-9) -> PlanarEachSchedule:
    """Merge per-tag event lists [(time, kind, ordinal of the tag's own sample of that kind)] (kind 0 = ranging, 1..4 =
    PX4Flow, IMU, magnetometer, compass) into the slots of kfpos_run_planar_events_each_dev. Time is counted in quanta
    of `tick` seconds, round(time / tick): events of one kind in the same quantum share a slot (times that differ by
    less than a tick but fall either side of a rounding boundary do not); slots are ordered by quantum, and within one
    quantum the sensor slots come in kind order 1..4 ahead of the ranging slot. A tag's dt in a slot is the time since
    its own previous event (its first: since t = 0), so its dts add up to the time of its last event. Events of one tag
    in the same quantum are simultaneous at the clock's resolution and run in slot order, whatever their raw times say:
    where that order turns two raw times round, the later slot gets dt = 0.0, never a negative dt, which the call would
    read as "absent"."""
    T = len(lines)
    key = lambda ev: (int(round(ev[0] / tick)), 4 if ev[1] == 0 else int(ev[1]) - 1)  # noqa: E731
    for line in lines:
        for ev in line:
            if not 0 <= int(ev[1]) <= 4:
                raise ValueError("kind %r is no planar event kind" % (ev[1],))
    slots = sorted({key(ev) for line in lines for ev in line})
    index = {k: e for e, k in enumerate(slots)}
    E = len(slots)
    dt = np.full((E, T), -1.0)
    ordinal = np.full((E, T), -1, dtype=np.int32)
    for t, line in enumerate(lines):
        prev = 0.0
        for ev in sorted(line, key=key):
            e = index[key(ev)]
            if ordinal[e, t] >= 0:
                raise ValueError("tag %d has two events in one slot: its samples are closer than `tick`" % t)
            dt[e, t], ordinal[e, t] = max(ev[0] - prev, 0.0), ev[2]
            prev = max(prev, ev[0])
    kinds = np.array([0 if o == 4 else o + 1 for _, o in slots], dtype=np.uint8)
    time = np.array([q for q, _ in slots], dtype=np.float64) * tick
    return PlanarEachSchedule(kinds, dt, ordinal, time)


def planar_sample(w: "Workload", kind: int, n: int) -> np.ndarray:
    """(T, PLANAR_WIDTH[kind]) sample n of a sensor kind for every tag of the workload, in the layout of
    kfpos_step_sensor_dev (IMU: angular velocity 3, its covariance 9, linear acceleration 3, its covariance 9)."""
    if kind == 1:
        return w.px4flow(n)
    if kind == 2:
        wv, la = w.planar_imu(n)
        cw = np.tile(np.eye(3).ravel() * 1e-4, (w.n_tags, 1))
        return np.concatenate([wv, cw, la, w.accel_cov()], axis=1)
    if kind == 3:
        return w.mag(n)
    return w.compass(n)[:, None]


def planar_slot_inputs(w: "Workload", sched: PlanarEachSchedule, absent_mm: int = -1, epoch=None, sample=None):
    """The inputs of a merged planar schedule in slot order: {0: ranges (J, T, A) int32, 1: (n, T, 5), 2: (n, T, 24),
    3: (n, T, 3), 4: (n, T, 1)}. Every participating tag reads its OWN sample sched.ordinal[e, t]; entries of absent
    tags are NaN, `absent_mm` for ranges. epoch(w, n) -> (T, A) replaces w.ranges_mm, sample(w, kind, n) planar_sample."""
    epoch = epoch or (lambda w_, n: w_.ranges_mm(n))
    sample = sample or planar_sample
    T, A = w.n_tags, w.n_anchors
    out = {0: []}
    out.update({k: [] for k in PLANAR_WIDTH})
    for e, kind in enumerate(sched.kinds):
        kind = int(kind)
        here = sched.ordinal[e] >= 0
        a = np.full((T, A), absent_mm, dtype=np.int32) if kind == 0 else np.full((T, PLANAR_WIDTH[kind]), np.nan)
        for n in np.unique(sched.ordinal[e][here]):
            m = here & (sched.ordinal[e] == n)
            a[m] = (epoch(w, int(n)) if kind == 0 else sample(w, kind, int(n)))[m]
        out[kind].append(a)
    empty = {0: np.zeros((0, T, A), dtype=np.int32)}
    empty.update({k: np.zeros((0, T, c)) for k, c in PLANAR_WIDTH.items()})
    return {k: (np.stack(v) if v else empty[k]) for k, v in out.items()}
