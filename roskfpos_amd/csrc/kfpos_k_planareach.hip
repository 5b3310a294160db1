/*
 * kfpos_k_planareach.hip -- k_events_planar_each: a multi-sensor event schedule of the 8-state planar filter in one
 * launch in which every tag has a timeline of its own (kfpos_run_planar_events_each_dev). A slot's kind is shared by the
 * bank; who takes part in it, and at which timeLag, is per tag: dt_each[e][t] < 0 means tag t sits slot e out, exactly
 * as a single call with a per-tag dt array treats it (k_step_planar, kfpos_k_misc.hip: KFPOS_ST_SKIPPED, nothing of the
 * tag changes, the slot's sample is not latched). The state AND the latched samples stay in registers from slot to slot
 * and every event a tag runs forms its rows as k_step_planar<true, ...> does and runs the unchanged step_planar8<true>
 * (kfpos_core_planar.h), so the launch computes bit for bit what as many kfpos_step_sensor_dev / kfpos_step_toa_dev
 * launches with that dt array would. k_events_planar (kfpos_k_planarev.hip) is the form with one timeline for all tags.
 */
#include "kfpos_kernels.h"

/* 1: a lane's dt is fetched one slot ahead (the library); 0: where the slot runs -- the A/B build behind the figures in
 * profiles/HISTORY.md (hipcc -DKFPOS_PLANAREACH_DT_AHEAD=0, loaded through KFPOS_LIB_PATH) */
#ifndef KFPOS_PLANAREACH_DT_AHEAD
#define KFPOS_PLANAREACH_DT_AHEAD 1
#endif

namespace {

/* AS = -8: compile-time anchor loops over the LDS-resident ranging epoch; AS = 0: run-time anchor loop (as
 * k_events_planar). A slot's sample is fetched where the slot runs, under the lane's participation (k_events_planar
 * measured samples fetched one event ahead as a loss); the lane's dt is fetched one slot AHEAD, for two registers: the
 * participation branch hangs on it. Fetched where the slot runs, the phase-grouped bank measured 5 % slower and the
 * synchronous one 2 %. */
template <typename REAL, typename MREAL, int AS>
__global__ __launch_bounds__(WAVE) void k_events_planar_each(const kfpos_k::PevEachArgs ev) {
    extern __shared__ double lds[];
    const KArgs &a = ev.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    const Params pr = make_params(a);
    const int n = a.n_steps;
    /* wave-uniform, and kept as an integer the optimiser cannot see through (k_events_planar): the branches on it are
     * scalar branches, the ordinals selected by it scalar registers */
    auto kind_of = [&](int e) -> int { return opaque_uniform(kfpos_kinds4_at(ev.kinds, e)); };
    auto load_dt = [&](int e) -> double { return (ev.dt_each + (size_t)e * T)[(uint32_t)opaque_lane(t)]; };

    constexpr bool DT_AHEAD = KFPOS_PLANAREACH_DT_AHEAD != 0;
    double dt_next = DT_AHEAD ? load_dt(0) : 0.0;
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
     * (rows is formed from lt.has), and never written back unless the lane samples their kind in this launch */
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

    uint32_t sampled = 0; /* per lane: kinds this lane latched in this launch (ROW_*) */
    bool ran = false;     /* per lane: an event of this launch ran on this lane */
    /* running ordinals of the next slot of each kind, one byte each (a launch has at most 128 slots): wave-uniform, they
     * count SLOTS whoever takes part, and are advanced by integer arithmetic alone -- selected by a comparison they
     * would become vector registers (k_events_planar) */
    unsigned long long cnt = 0;
    for (int e = 0; e < n; ++e) {
        const int kind = kind_of(e);
        const int ord = opaque_uniform((int)((cnt >> (kind * 8)) & 0xFFull)); /* this slot's ordinal within its kind */
        cnt += 1ull << (kind * 8);
        const double dt = DT_AHEAD ? dt_next : load_dt(opaque_uniform(e));
        const bool more = e + 1 < n;
        if (DT_AHEAD && more) dt_next = load_dt(opaque_uniform(e + 1));
        const uint32_t tl = (uint32_t)opaque_lane(t);
        const bool run = !(dt < 0.0); /* THE predicate of the single calls: a NaN dt runs the event */
        const bool last_status = !more && a.status;
        /* A wavefront in which nobody has anything in this slot passes it uniformly: no staging, no sample loads, no
         * step -- only the rows every slot writes, below. (One way round the loop: with a `continue` here the loop has
         * two back edges, and every instantiation took some 35 registers more.) */
        const bool any = __builtin_amdgcn_ballot_w64(run) != 0; /* wave-uniform */
        uint32_t rows = 0;
        bool go = run; /* the lane runs this slot's event: present, and its sample not dropped */
        uint32_t s = ST_SKIPPED; /* the lane sits the slot out: what skipped_lane() reports */
        if (any) {
        if (kind == KFPOS_SENSOR_PX4FLOW) { /* KalmanFilter.cpp:102-128; a sample of quality 0 is dropped on entry */
            if (run) { /* dt is looked at ahead of the sample (k_step_planar): an absent lane latches nothing */
                const double *sp = ev.sens[0] + (size_t)ord * ev.stride_sens[0];
                double f[5], m[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) f[k] = (sp + k * T)[tl];
                go = px4_sample(pr, f, m);
                if (go) {
#pragma unroll
                    for (int k = 0; k < 5; ++k) lt.px4[k] = m[k];
                    lt.has |= ROW_PX4;
                    sampled |= ROW_PX4;
                }
            }
            rows = ROW_PX4;
        } else if (kind == KFPOS_SENSOR_IMU) { /* :139-170 */
            if (run) {
                const double *sp = ev.sens[1] + (size_t)ord * ev.stride_sens[1];
                double w3[3], cw[9], la[3], ca[9];
#pragma unroll
                for (int k = 0; k < 3; ++k) { w3[k] = (sp + k * T)[tl]; la[k] = (sp + (12 + k) * T)[tl]; }
#pragma unroll
                for (int k = 0; k < 9; ++k) { cw[k] = (sp + (3 + k) * T)[tl]; ca[k] = (sp + (15 + k) * T)[tl]; }
                imu_sample8(pr, w3, cw, la, ca, lt.imu);
                lt.has |= ROW_IMU;
                sampled |= ROW_IMU;
            }
            rows = ROW_IMU;
        } else if (kind == KFPOS_SENSOR_MAG) { /* :188 */
            if (run) {
                const double *sp = ev.sens[2] + (size_t)ord * ev.stride_sens[2];
                lt.mag[0] = atan2((sp + 1 * T)[tl], (sp + 0 * T)[tl]) - pr.mag_offset;
                lt.mag[1] = pr.mag_cov;
                lt.has |= ROW_MAG;
                sampled |= ROW_MAG;
            }
            rows = ROW_MAG;
        } else if (kind == KFPOS_SENSOR_COMPASS) { /* :207; carries the PX4Flow and IMU rows the tag latched before it */
            rows = ROW_MAG | (lt.has & (ROW_PX4 | ROW_IMU));
            if (run) {
                const double *sp = ev.sens[3] + (size_t)ord * ev.stride_sens[3];
                lt.mag[0] = normalize_angle(sp[tl]);
                lt.mag[1] = pr.mag_cov;
                lt.has |= ROW_MAG;
                sampled |= ROW_MAG;
            }
        } else { /* newTOAMeasurement: everything the tag has latched rides along (:84-98). The whole wavefront stages,
                  * absent lanes included: their entries are loaded and never used */
            if constexpr (AS < 0) sc = stage_epoch_lds_n<MREAL, -AS>(a, lds, lane, tl, ord);
            else sc = stage_epoch_lds<MREAL>(a, lds, lane, tl, ord);
            rows = ROW_RANGING | lt.has;
        }
        if (go) {
            s = step_planar8<true>(tg, sc, pr, dt, rows, lt, park);
            ran = true;
        }
        }
        if (a.traj) { /* the pose a per-slot caller would have read back; a lane that sat out: the untouched position */
            double *tp = a.traj + (size_t)opaque_uniform(e) * 3 * T;
            (tp + 0 * T)[tl] = tg.xy[0];
            (tp + 1 * T)[tl] = tg.xy[1];
            (tp + 2 * T)[tl] = tg.z;
        }
        if (ev.status_events || last_status) { /* the status word a single call would have returned for this slot */
            if (any) {
                bool fin = isfinite(tg.xy[0]) & isfinite(tg.xy[1]) & isfinite(tg.z) & isfinite(tg.vel[0]) &
                           isfinite(tg.vel[1]) & isfinite(tg.ang) & isfinite(tg.om);
#pragma unroll
                for (int k = 0; k < 36; ++k) fin &= isfinite(tg.P.a[k]);
                const bool waiting = !a.use_init_pos && isnan(tg.xy[0]); /* (open text: nonfinite_state() here changes the kernel's code) */
                if (go && !fin && !waiting) s |= ST_NONFINITE;
            }
            if (ev.status_events) (ev.status_events + (size_t)opaque_uniform(e) * T)[tl] = s;
            if (last_status) a.status[tl] = s;
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what the single launch of this event would have kept in HBM */
            if (more && go) { /* only lanes that ran it */
#pragma unroll
                for (int k = 0; k < 36; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }

    if (!ran) return; /* a tag that ran nothing keeps every stored byte, FL_STARTED and compact covariance planes included */
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
    a.flags[t32] = fl | FL_STARTED | (lt.has << PLANAR_HAS_SHIFT);
}

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::planar_events_each_kernel_t planareach_of(int as) {
    if (as == -8) return k_events_planar_each<REAL, MREAL, -8>;
    return k_events_planar_each<REAL, MREAL, 0>;
}
kfpos_k::planar_events_each_kernel_t kfpos_k::planar_events_each_kernel(int st, int as) {
    return KFPOS_BY_STORAGE(st, planareach_of, as);
}
