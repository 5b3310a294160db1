/*
 * kfpos_k_imu9each.hip -- k_events_imu9_each: an event schedule of the 9-state filter in one launch in which every tag
 * has a timeline of its own (kfpos_run_events_each_dev). A slot's kind is shared by the bank; who takes part in it, and
 * at which timeLag, is per tag: dt_each[e][t] < 0 means tag t sits slot e out, exactly as a single call with a per-tag
 * dt array treats it (KFPOS_ST_SKIPPED, nothing of the tag changes). The state stays in registers from slot to slot and
 * every event a tag runs is the per-tag text of the single calls (step_imu9_state<true> / <false> + step_imu9_cov,
 * kfpos_core_imu9.h), so the launch computes bit for bit what as many kfpos_step_imu_dev / kfpos_step_toa_dev launches
 * with that dt array would. k_events_imu9 (kfpos_k_imu9ev.hip) is the form with one timeline for all tags.
 */
#include "kfpos_kernels.h"

namespace {

/* AS = 8: the ranging epoch in registers; AS = 0: run-time anchor loop over an LDS-resident epoch (as k_events_imu9) */
template <typename REAL, typename MREAL, int AS>
__global__ __launch_bounds__(WAVE) void k_events_imu9_each(const kfpos_k::EvEachArgs ev) {
    extern __shared__ double lds[];
    const KArgs &a = ev.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    const Params pr = make_params(a);
    /* the next slot's per-lane dt and accelerometer sample are fetched one slot AHEAD where k_events_imu9 fetches ahead
     * (same rule). Its ranging epoch is not: the rule holds for two register-resident instantiations only, <double,
     * float, 8> and <p48, float, 8> (the run-time-loop form stages its epoch per slot), and in both the 16 registers of
     * an epoch fetched ahead do not fit beside the per-lane dts and masks -- they spilled inside the loop, 52 / 68
     * bytes per lane -- so the ranges of the next slot are fetched between two slots */
    constexpr bool AHEAD = sizeof(MREAL) == 4 && !std::is_same<REAL, float>::value;
    /* every 8-anchor instantiation spills inside the slot loop with the peeled Gauss-Newton text (step_imu9_state's
     * PEEL): every instantiation of this kernel keeps the unpeeled text it always compiled */
    constexpr bool PEEL = false;
    constexpr int NA = AS > 0 ? AS : 1;
    const int n = a.n_steps;
    /* the kind is wave-uniform and kept as an integer the optimiser cannot see through: carried round the loop as a
     * boolean it becomes a lane mask, and the ordinals selected by it vector registers (k_events_imu9) */
    auto is_toa = [&](int e) -> int { return opaque_uniform(kfpos_kinds1_at(ev.kinds, e)); };
    auto load_dt = [&](int e) -> double { return (ev.dt_each + (size_t)e * T)[(uint32_t)opaque_lane(t)]; };

    /* load order = order of first use, as in k_step_imu9 */
    uint32_t fl = a.flags[t32];
    double dt_next = load_dt(0);
    RawEpoch<MREAL, NA> raw;
    RawImu<MREAL> rawi;
    int toa = is_toa(0);
    if (toa) {
        if constexpr (AS > 0) fetch_epoch<MREAL, AS>(a, t, 0, raw);
    } else {
        fetch_imu<MREAL>(a, t, 0, rawi);
    }
    Tag9 tg;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tg.pos[k] = (a.pos + k * T)[t32];
        tg.vel[k] = (a.vel + k * T)[t32];
    }
    const CovPark9 park{lds + (AS == 0 ? 3 * (size_t)a.A * WAVE : 0) + lane, WAVE};
    Imu imu;
    imu.ci = park.a + 66 * WAVE;
    imu.ci_stride = WAVE;
    /* TWO whiteners per lane, one place for them. Until a lane's own first sample in this launch its ranging events
     * re-fuse what the tag had latched before, with THAT sample's covariance: imu.ci then holds the whitener of the six
     * latched entries, rebuilt as k_step_imu9 rebuilds it. From that sample on the tag uses the call's one covariance.
     * A second area of 12 entries per lane would take the workgroup from 39.2 to 45.2 KB of LDS, and only three of
     * them instead of four fit a CU's 160 KB -- a 65 536-tag bank then runs in two rounds -- so the lane whitens `cov`
     * again at its first sample instead (ci_is_cov says whether it has to: not where nothing was latched, nor where
     * the latch holds the very six entries of `cov`, which is what every launch of a call after the first finds). */
    const bool any_imu = a.cov != nullptr; /* wave-uniform: the host passes cov only where the launch has an IMU slot */
    MREAL rawc[9];
    if (any_imu) fetch_imu_cov<MREAL>(a, t, 0, rawc);
    imu.has = (fl & FL_HAS_IMU) != 0;
    double cl[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    if (imu.has) {
#pragma unroll
        for (int k = 0; k < 3; ++k) imu.acc[k] = ldrow<MREAL>(a.imu_acc, k, T, t32);
        cl[0] = ldrow<MREAL>(a.imu_cov, 0, T, t32);
        cl[3] = ldrow<MREAL>(a.imu_cov, 1, T, t32);
        cl[4] = ldrow<MREAL>(a.imu_cov, 2, T, t32);
        cl[6] = ldrow<MREAL>(a.imu_cov, 3, T, t32);
        cl[7] = ldrow<MREAL>(a.imu_cov, 4, T, t32);
        cl[8] = ldrow<MREAL>(a.imu_cov, 5, T, t32);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) imu.acc[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, 45, T, t32);
    /* Diagonal form of the gain iteration's pass (same bits, k_step_imu9): only where EVERY whitener a lane of this
     * wavefront may use in this launch -- the call's of every lane, the latched one of a lane that has a sample -- has
     * zeros off its diagonal. */
    bool mine = true;
    bool ci_is_cov = false; /* per lane: imu.ci holds the whitener of `cov` */
    if (any_imu) {
        double cv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) cv[k] = (double)rawc[k];
        imu_whitener(cv, imu.ci, imu.ci_stride);
        mine = imu.Wi(1) == 0.0 && imu.Wi(2) == 0.0 && imu.Wi(4) == 0.0;
        ci_is_cov = !imu.has || (cl[0] == cv[0] && cl[3] == cv[3] && cl[4] == cv[4] && cl[6] == cv[6] &&
                                 cl[7] == cv[7] && cl[8] == cv[8]);
    }
    if (imu.has && !ci_is_cov) {
        imu_whitener(cl, imu.ci, imu.ci_stride);
        mine = mine && imu.Wi(1) == 0.0 && imu.Wi(2) == 0.0 && imu.Wi(4) == 0.0;
    }
    bool diag = false;
    if (a.imu9_diag) diag = __builtin_amdgcn_ballot_w64(mine) == __builtin_amdgcn_ballot_w64(true);

    __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0): everything loaded so far, outside the loop (k_step_imu9) */
    uint32_t s = 0;
    int it = 0, ii = 0;   /* running ordinals of the next ranging epoch / accelerometer sample: wave-uniform */
    bool sampled = false; /* per lane: an IMU event of this tag has run in this launch */
    bool ran = false;     /* per lane: any event of this tag has run in this launch */
    for (int e = 0; e < n; ++e) {
        const double dt = dt_next;
        const bool more = e + 1 < n;
        int toa_next = 0;
        if (more) toa_next = is_toa(opaque_uniform(e + 1));
        const int cur = it; /* a ranging slot's ordinal; it / ii name the next slot's of either kind from here on */
        (void)cur;
        it += toa;
        ii += 1 - toa;
        /* the inputs of slot e + 1 for EVERY lane, whoever takes part in slot e: its dt and its three accelerometer
         * words (fetch_small), or its ranges (fetch_epoch) */
        auto fetch_small = [&]() {
            if (!more) return;
            dt_next = load_dt(opaque_uniform(e + 1));
            if (!toa_next) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(ii), rawi);
        };
        auto fetch_epoch_next = [&]() {
            if constexpr (AS > 0) {
                if (more && toa_next) fetch_epoch<MREAL, AS>(a, opaque_lane(t), opaque_uniform(it), raw);
            }
        };
        const bool run = !(dt < 0.0); /* THE predicate of the single calls: a NaN dt runs the event */
        const bool last_status = !more && a.status;
        if (__builtin_amdgcn_ballot_w64(run) == 0) {
            /* nobody in this wavefront has anything in this slot: past the step, uniformly */
            fetch_small();
            fetch_epoch_next();
            if (a.traj) {
#pragma unroll
                for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
            }
            if (ev.status_events) (ev.status_events + (size_t)opaque_uniform(e) * T)[t32] = ST_SKIPPED;
            if (last_status) a.status[t32] = ST_SKIPPED;
            toa = toa_next;
            continue;
        }
        Iekf9Out o;
        bool update = false;
        if (toa) { /* newTOAMeasurement: ranging epoch, re-fusing whatever sample the tag has latched */
            if constexpr (AS > 0) {
                RegScratch<AS> sc;
                unpack_epoch<MREAL, AS>(raw, sc);
                if constexpr (AHEAD) fetch_small();
                if (run) update = step_imu9_state<true, true, false, true, PEEL>(tg, sc, pr, dt, imu, park, imu9_fast(diag, imu.has), o, s);
            } else {
                Scratch sc = stage_epoch_lds<MREAL>(a, lds, lane, t, opaque_uniform(cur)); /* the whole wavefront */
                if constexpr (AHEAD) fetch_small();
                if (run) update = step_imu9_state<true, true, false, true, PEEL>(tg, sc, pr, dt, imu, park, imu9_fast(diag, imu.has), o, s);
            }
        } else { /* newIMUMeasurement: latch the sample, predict + IMU-only update */
            if (run) {
#pragma unroll
                for (int k = 0; k < 3; ++k) imu.acc[k] = (double)rawi.acc[k];
                imu.has = true;
                if (!ci_is_cov) { /* from here on this tag fuses with the call's covariance */
                    MREAL rc[9];
                    fetch_imu_cov<MREAL>(a, opaque_lane(t), 0, rc);
                    double cv[9];
#pragma unroll
                    for (int k = 0; k < 9; ++k) cv[k] = (double)rc[k];
                    imu_whitener(cv, imu.ci, imu.ci_stride);
                    ci_is_cov = true;
                }
                sampled = true;
            }
            if constexpr (AHEAD) fetch_small();
            Scratch sc{nullptr, nullptr, nullptr, WAVE};
            if (run) update = step_imu9_state<false, true, false, true, PEEL>(tg, sc, pr, dt, imu, park, imu9_fast(diag, imu.has), o, s);
        }
        ran |= run;
        /* the pose store between the state part and the covariance part (k_step_imu9); a lane that sits the slot out
         * reports its untouched position */
        if (a.traj) {
#pragma unroll
            for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
        }
        if (update) s = step_imu9_cov(tg, o, imu);
        if constexpr (!AHEAD) fetch_small();
        fetch_epoch_next();
        if (ev.status_events || last_status) { /* the status word a single call would have returned for this slot */
            uint32_t w = ST_SKIPPED;
            if (run) {
                bool fin = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) fin &= isfinite(tg.pos[k]) & isfinite(tg.vel[k]);
#pragma unroll
                for (int k = 0; k < 45; ++k) fin &= isfinite(tg.P.a[k]);
                w = nonfinite_state(fin, a.use_init_pos, tg.pos[0]) ? (s | ST_NONFINITE) : s;
            }
            if (ev.status_events) (ev.status_events + (size_t)opaque_uniform(e) * T)[t32] = w;
            if (last_status) a.status[t32] = w;
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what the single launch of this event would have kept in HBM */
            if (more && run) {
#pragma unroll
                for (int k = 0; k < 45; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
        toa = toa_next;
    }

    if (!ran) return; /* a tag that ran nothing keeps every stored byte */
    if (sampled) { /* the last sample and its covariance stay latched (lastImuMeasurement, KalmanFilterTOAIMU.cpp:78-89) */
#pragma unroll
        for (int k = 0; k < 3; ++k) strow<MREAL>(a.imu_acc, k, T, t32, imu.acc[k]);
        fetch_imu_cov<MREAL>(a, t, 0, rawc); /* read again rather than kept in nine registers across the loop */
        double cv[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) cv[k] = (double)rawc[k];
        latch_imu_cov<MREAL>(a, T, t32, cv);
        fl |= FL_HAS_IMU;
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        (a.pos + k * T)[t32] = tg.pos[k];
        (a.vel + k * T)[t32] = tg.vel[k];
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) stcov<REAL>(a.P, k, 45, T, t32, tg.P.a[k]);
    a.flags[t32] = fl | FL_STARTED;
}

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::events_each_kernel_t imu9each_of(int as) {
    if (as == 8) return k_events_imu9_each<REAL, MREAL, 8>;
    return k_events_imu9_each<REAL, MREAL, 0>;
}
kfpos_k::events_each_kernel_t kfpos_k::imu9_events_each_kernel(int st, int as) {
    return KFPOS_BY_STORAGE(st, imu9each_of, as);
}
