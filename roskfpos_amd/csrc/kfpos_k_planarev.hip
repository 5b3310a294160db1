/*
 * kfpos_k_planarev.hip -- k_events_planar: a multi-sensor event schedule of the 8-state planar filter in one launch
 * (kfpos_run_planar_events_dev). The reference's KalmanFilter has five entry points -- newTOAMeasurement and the
 * PX4Flow, IMU, magnetometer and compass samples (KalmanFilter.cpp:84-229) -- each a complete estimatePositionKF at
 * its own timeLag over the rows it carries. Here the state AND the latched samples stay in registers from event to
 * event; every event forms its rows as k_step_planar<true, ...> does (kfpos_k_misc.hip) and runs the unchanged
 * step_planar8<true> (kfpos_core_planar.h), so the launch computes bit for bit what as many kfpos_step_sensor_dev /
 * kfpos_step_toa_dev launches would.
 */
#include "kfpos_kernels.h"

namespace {

/* AS = -8: compile-time anchor loops over the LDS-resident ranging epoch; AS = 0: run-time anchor loop -- the two the
 * handle's single ranging call runs once it has latched samples. Sensor events stage nothing. An event's sample is fetched
 * where the event runs: fetched one event ahead, the full sensor period measured 5 % slower. */
template <typename REAL, typename MREAL, int AS>
__global__ __launch_bounds__(WAVE) void k_events_planar(const kfpos_k::PevArgs ev) {
    extern __shared__ double lds[];
    const KArgs &a = ev.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    const Params pr = make_params(a);
    const int n = a.n_steps;
    /* wave-uniform, and kept as an integer the optimiser cannot see through (k_events_imu9): the branches on it are
     * scalar branches, the ordinals selected by it scalar registers */
    auto kind_of = [&](int e) -> int { return opaque_uniform(kfpos_kinds4_at(ev.kinds, e)); };

    Tag8 tg;
    tg.xy[0] = (a.pos + 0 * T)[t32];
    tg.xy[1] = (a.pos + 1 * T)[t32];
    tg.z = (a.pos + 2 * T)[t32];
    tg.vel[0] = (a.vel + 0 * T)[t32];
    tg.vel[1] = (a.vel + 1 * T)[t32];
    tg.ang = (a.vel + 2 * T)[t32];
    tg.om = (a.vel + 3 * T)[t32];
    const uint32_t fl = a.flags[t32];
    /* the latched rows this tag has, loaded once; rows it does not have are never read by an event that carries them
     * (rows is formed from lt.has), and never written back unless this launch samples their kind */
    Latch8 lt;
    lt.has = (fl >> PLANAR_HAS_SHIFT) & (ROW_PX4 | ROW_IMU | ROW_MAG);
#pragma unroll
    for (int k = 0; k < 5; ++k) lt.px4[k] = (lt.has & ROW_PX4) ? (a.platch + k * T)[t32] : 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) lt.imu[k] = (lt.has & ROW_IMU) ? (a.platch + (5 + k) * T)[t32] : 0.0;
#pragma unroll
    for (int k = 0; k < 2; ++k) lt.mag[k] = (lt.has & ROW_MAG) ? (a.platch + (13 + k) * T)[t32] : 0.0;
#pragma unroll
    for (int k = 0; k < 36; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, 36, T, t32);

    /* the predicted covariance is parked in LDS, [36][lane], behind the epoch scratch (k_step_planar) */
    const CovSpill8 park{lds + 3 * (size_t)(AS < 0 ? -AS : a.A) * WAVE + lane, WAVE};
    typename std::conditional<(AS < 0), StaticScratch<(AS < 0 ? -AS : 1)>, Scratch>::type sc;
    sc.r = sc.e = sc.w = nullptr; /* a sensor event reads no anchor row */
    sc.stride = WAVE;

    uint32_t s = 0, sampled = 0; /* sampled: kinds this lane latched in this launch (ROW_*) */
    bool ran = false;            /* an event of this launch ran on this lane */
    /* running ordinals of the next event of each kind, one byte each (a launch has at most 128 events): wave-uniform,
     * and advanced by integer arithmetic alone -- selected by a comparison they would become vector registers */
    unsigned long long cnt = 0;
    for (int e = 0; e < n; ++e) {
        const int kind = kind_of(e);
        const int ord = opaque_uniform((int)((cnt >> (kind * 8)) & 0xFFull)); /* this event's ordinal within its kind */
        cnt += 1ull << (kind * 8);
        const double dt = a.dt_steps[opaque_uniform(e)];
        const bool more = e + 1 < n;
        const uint32_t tl = (uint32_t)opaque_lane(t);
        uint32_t rows;
        bool drop = false;
        if (kind == KFPOS_SENSOR_PX4FLOW) { /* KalmanFilter.cpp:102-128; a sample of quality 0 is dropped on entry */
            const double *sp = ev.sens[0] + (size_t)ord * ev.stride_sens[0];
            double f[5], m[5];
#pragma unroll
            for (int k = 0; k < 5; ++k) f[k] = (sp + k * T)[tl];
            drop = !px4_sample(pr, f, m);
            if (!drop) {
#pragma unroll
                for (int k = 0; k < 5; ++k) lt.px4[k] = m[k];
                lt.has |= ROW_PX4;
                sampled |= ROW_PX4;
            }
            rows = ROW_PX4;
        } else if (kind == KFPOS_SENSOR_IMU) { /* :139-170 */
            const double *sp = ev.sens[1] + (size_t)ord * ev.stride_sens[1];
            double w3[3], cw[9], la[3], ca[9];
#pragma unroll
            for (int k = 0; k < 3; ++k) { w3[k] = (sp + k * T)[tl]; la[k] = (sp + (12 + k) * T)[tl]; }
#pragma unroll
            for (int k = 0; k < 9; ++k) { cw[k] = (sp + (3 + k) * T)[tl]; ca[k] = (sp + (15 + k) * T)[tl]; }
            imu_sample8(pr, w3, cw, la, ca, lt.imu);
            lt.has |= ROW_IMU;
            sampled |= ROW_IMU;
            rows = ROW_IMU;
        } else if (kind == KFPOS_SENSOR_MAG) { /* :188 */
            const double *sp = ev.sens[2] + (size_t)ord * ev.stride_sens[2];
            lt.mag[0] = atan2((sp + 1 * T)[tl], (sp + 0 * T)[tl]) - pr.mag_offset;
            lt.mag[1] = pr.mag_cov;
            lt.has |= ROW_MAG;
            sampled |= ROW_MAG;
            rows = ROW_MAG;
        } else if (kind == KFPOS_SENSOR_COMPASS) { /* :207; carries the PX4Flow and IMU rows latched before it */
            const double *sp = ev.sens[3] + (size_t)ord * ev.stride_sens[3];
            lt.mag[0] = normalize_angle(sp[tl]);
            lt.mag[1] = pr.mag_cov;
            rows = ROW_MAG | (lt.has & (ROW_PX4 | ROW_IMU));
            lt.has |= ROW_MAG;
            sampled |= ROW_MAG;
        } else { /* newTOAMeasurement: everything latched rides along (:84-98) */
            if constexpr (AS < 0) sc = stage_epoch_lds_n<MREAL, -AS>(a, lds, lane, tl, ord);
            else sc = stage_epoch_lds<MREAL>(a, lds, lane, tl, ord);
            rows = ROW_RANGING | lt.has;
        }
        if (!drop) {
            s = step_planar8<true>(tg, sc, pr, dt, rows, lt, park);
            ran = true;
        } else {
            s = ST_SKIPPED; /* the lane sits the event out: what skipped_lane() reports */
        }
        if (a.traj) { /* the pose a per-event caller would have read back; a dropped lane's is the untouched position */
            double *tp = a.traj + (size_t)opaque_uniform(e) * 3 * T;
            (tp + 0 * T)[tl] = tg.xy[0];
            (tp + 1 * T)[tl] = tg.xy[1];
            (tp + 2 * T)[tl] = tg.z;
        }
        if (ev.status_events || !more) { /* the status word a single call would have returned for this event */
            bool fin = isfinite(tg.xy[0]) & isfinite(tg.xy[1]) & isfinite(tg.z) & isfinite(tg.vel[0]) &
                       isfinite(tg.vel[1]) & isfinite(tg.ang) & isfinite(tg.om);
#pragma unroll
            for (int k = 0; k < 36; ++k) fin &= isfinite(tg.P.a[k]);
            const bool waiting = !a.use_init_pos && isnan(tg.xy[0]); /* (open text: nonfinite_state() here changes the kernel's code) */
            if (!drop && !fin && !waiting) s |= ST_NONFINITE;
            if (ev.status_events) (ev.status_events + (size_t)opaque_uniform(e) * T)[tl] = s;
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what single launches would have kept in HBM */
            if (more) {
#pragma unroll
                for (int k = 0; k < 36; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }

    (a.pos + 0 * T)[t32] = tg.xy[0];
    (a.pos + 1 * T)[t32] = tg.xy[1];
    (a.pos + 2 * T)[t32] = tg.z;
    (a.vel + 0 * T)[t32] = tg.vel[0];
    (a.vel + 1 * T)[t32] = tg.vel[1];
    (a.vel + 2 * T)[t32] = tg.ang;
    (a.vel + 3 * T)[t32] = tg.om;
#pragma unroll
    for (int k = 0; k < 36; ++k) stcov<REAL>(a.P, k, 36, T, t32, tg.P.a[k]);
    /* only the latch rows of kinds this lane sampled in this launch: the others keep whatever HBM holds */
    if (sampled & ROW_PX4) {
#pragma unroll
        for (int k = 0; k < 5; ++k) (a.platch + k * T)[t32] = lt.px4[k];
    }
    if (sampled & ROW_IMU) {
#pragma unroll
        for (int k = 0; k < 8; ++k) (a.platch + (5 + k) * T)[t32] = lt.imu[k];
    }
    if (sampled & ROW_MAG) {
        (a.platch + 13 * T)[t32] = lt.mag[0];
        (a.platch + 14 * T)[t32] = lt.mag[1];
    }
    /* a lane none of whose events ran (dropped PX4Flow samples only) is left as found, FL_STARTED included */
    if (ran) a.flags[t32] = fl | FL_STARTED | (lt.has << PLANAR_HAS_SHIFT);
    if (a.status) a.status[t32] = s;
}

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::planar_events_kernel_t planarev_of(int as) {
    if (as == -8) return k_events_planar<REAL, MREAL, -8>;
    return k_events_planar<REAL, MREAL, 0>;
}
kfpos_k::planar_events_kernel_t kfpos_k::planar_events_kernel(int st, int as) {
    return KFPOS_BY_STORAGE(st, planarev_of, as);
}
