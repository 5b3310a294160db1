/*
 * kfpos_k_imu9ev.hip -- k_events_imu9: an IMU-rate event schedule of the 9-state filter in one launch
 * (kfpos_run_events_dev). The reference node runs newIMUMeasurement at the IMU's rate -- each one a complete
 * estimatePositionKF(false, ...) at its own timeLag: predict, IMU-only update -- and newTOAMeasurement re-fuses the
 * latched sample (KalmanFilterTOAIMU.cpp:49-92). Here the state stays in registers from event to event; every event
 * runs the per-tag text of the single calls (step_imu9_state<true> / <false> + step_imu9_cov, kfpos_core_imu9.h), so
 * the launch computes bit for bit what as many kfpos_step_imu_dev / kfpos_step_toa_dev launches would.
 */
#include "kfpos_kernels.h"

namespace {

/* AS = 8: the ranging epoch in registers; AS = 0: run-time anchor loop over an LDS-resident epoch (k_step_imu9's two) */
template <typename REAL, typename MREAL, int AS>
__global__ __launch_bounds__(WAVE) void k_events_imu9(const kfpos_k::EvArgs ev) {
    extern __shared__ double lds[];
    const KArgs &a = ev.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    const Params pr = make_params(a);
    /* the next event's inputs are fetched one event AHEAD where k_step_imu9 has the registers for that (same rule) */
    constexpr bool AHEAD = sizeof(MREAL) == 4 && !std::is_same<REAL, float>::value;
    constexpr int NA = AS > 0 ? AS : 1;
    const int n = a.n_steps;
    /* wave-uniform, and kept as an integer the optimiser cannot see through: carried round the loop as a boolean it
     * becomes a lane mask, and the ordinals selected by it vector registers */
    auto is_toa = [&](int e) -> int { return opaque_uniform(kfpos_kinds1_at(ev.kinds, e)); };

    /* load order = order of first use, as in k_step_imu9 */
    uint32_t fl = a.flags[t32];
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
    /* ONE covariance for the call, whitened once per launch. A sample latched before this launch carries it too (the
     * host sends ranging events that precede the call's first sample down kfpos_run_trace_dev's path), and the latch
     * keeps exactly the six entries the whitener reads, in the type they arrived in: reloading it gives these bits. */
    MREAL rawc[9];
    fetch_imu_cov<MREAL>(a, t, 0, rawc);
    imu.has = (fl & FL_HAS_IMU) != 0;
    if (imu.has) {
#pragma unroll
        for (int k = 0; k < 3; ++k) imu.acc[k] = ldrow<MREAL>(a.imu_acc, k, T, t32);
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) imu.acc[k] = 0.0;
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, 45, T, t32);
    double cv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) cv[k] = (double)rawc[k];
    imu_whitener(cv, imu.ci, imu.ci_stride);
    /* <double, float, 8> sits at the register limit: with B^-1 and Sigma^-1 held across the trips of the gain iteration
     * it spills inside the event loop, so its trips read them as before (make check's scratch rule decides) */
    constexpr bool HOLD = !(std::is_same<REAL, double>::value && sizeof(MREAL) == 4 && AS == 8);
    /* <p48, float, 8> spills inside the event loop with the select forms of the epoch's weights (step_imu9_state's
     * SELECTS): every instantiation of this kernel keeps the conditional text it always compiled. The same goes for the
     * peeled Gauss-Newton text (PEEL), with which all four 8-anchor instantiations spill */
    constexpr bool PEEL = false;
    bool diag = false; /* the diagonal form of the gain iteration's pass: same bits (k_step_imu9) */
    if (a.imu9_diag) {
        const bool mine = imu.Wi(1) == 0.0 && imu.Wi(2) == 0.0 && imu.Wi(4) == 0.0;
        diag = __builtin_amdgcn_ballot_w64(mine) == __builtin_amdgcn_ballot_w64(true);
    }

    double dt_next = a.dt_steps[0];
    __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0): everything loaded so far, outside the loop (k_step_imu9) */
    uint32_t s = 0;
    int it = 0, ii = 0;   /* running ordinals of the next ranging epoch / accelerometer sample: wave-uniform */
    int sampled = 0;      /* an IMU event has run in this launch */
    for (int e = 0; e < n; ++e) {
        const double dt = dt_next;
        const bool more = e + 1 < n;
        int toa_next = 0;
        if (more) {
            dt_next = a.dt_steps[opaque_uniform(e + 1)];
            toa_next = is_toa(opaque_uniform(e + 1));
        }
        const int mine = it; /* a ranging event's ordinal; it / ii name the next event's of either kind from here on */
        (void)mine;
        it += toa;
        ii += 1 - toa;
        /* the inputs of event e + 1: its ranges, or its three accelerometer words */
        auto fetch_next = [&]() {
            if (!more) return;
            if (toa_next) {
                if constexpr (AS > 0) fetch_epoch<MREAL, AS>(a, opaque_lane(t), opaque_uniform(it), raw);
            } else {
                fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(ii), rawi);
            }
        };
        Iekf9Out o;
        bool update;
        if (toa) { /* newTOAMeasurement: ranging epoch, re-fusing whatever sample is latched */
            if constexpr (AS > 0) {
                RegScratch<AS> sc;
                unpack_epoch<MREAL, AS>(raw, sc);
                if constexpr (AHEAD) fetch_next();
                update = step_imu9_state<true, HOLD, false, false, PEEL>(tg, sc, pr, dt, imu, park, imu9_fast(diag, imu.has), o, s);
            } else {
                Scratch sc = stage_epoch_lds<MREAL>(a, lds, lane, t, opaque_uniform(mine)); /* staged per event */
                if constexpr (AHEAD) fetch_next();
                update = step_imu9_state<true, HOLD, false, false, PEEL>(tg, sc, pr, dt, imu, park, imu9_fast(diag, imu.has), o, s);
            }
        } else { /* newIMUMeasurement: latch the sample, predict + IMU-only update */
#pragma unroll
            for (int k = 0; k < 3; ++k) imu.acc[k] = (double)rawi.acc[k];
            imu.has = true;
            sampled = 1;
            if constexpr (AHEAD) fetch_next();
            Scratch sc{nullptr, nullptr, nullptr, WAVE};
            update = step_imu9_state<false, HOLD, false, false, PEEL>(tg, sc, pr, dt, imu, park, imu9_fast(diag, imu.has), o, s);
        }
        /* the pose store between the state part and the covariance part (k_step_imu9) */
        if (a.traj) {
#pragma unroll
            for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
        }
        if (update) s = step_imu9_cov(tg, o, imu);
        if constexpr (!AHEAD) fetch_next();
        if (ev.status_events && more) { /* the status word a single call would have returned for this event */
            bool fin = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) fin &= isfinite(tg.pos[k]) & isfinite(tg.vel[k]);
#pragma unroll
            for (int k = 0; k < 45; ++k) fin &= isfinite(tg.P.a[k]);
            const bool waiting = !a.use_init_pos && isnan(tg.pos[0]); /* (open text: nonfinite_state() here changes the kernel's code) */
            (ev.status_events + (size_t)opaque_uniform(e) * T)[t32] = (!fin && !waiting) ? (s | ST_NONFINITE) : s;
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what single launches would have kept in HBM */
            if (more) {
#pragma unroll
                for (int k = 0; k < 45; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
        toa = toa_next;
    }

    if (sampled) { /* the last sample and its covariance stay latched (lastImuMeasurement, KalmanFilterTOAIMU.cpp:78-89) */
#pragma unroll
        for (int k = 0; k < 3; ++k) strow<MREAL>(a.imu_acc, k, T, t32, imu.acc[k]);
        fetch_imu_cov<MREAL>(a, t, 0, rawc); /* read again rather than kept in nine registers across the loop */
#pragma unroll
        for (int k = 0; k < 9; ++k) cv[k] = (double)rawc[k];
        latch_imu_cov<MREAL>(a, T, t32, cv);
        fl |= FL_HAS_IMU;
    }
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        (a.pos + k * T)[t32] = tg.pos[k];
        (a.vel + k * T)[t32] = tg.vel[k];
        fin &= isfinite(tg.pos[k]) & isfinite(tg.vel[k]);
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) {
        stcov<REAL>(a.P, k, 45, T, t32, tg.P.a[k]);
        fin &= isfinite(tg.P.a[k]);
    }
    if (nonfinite_state(fin, a.use_init_pos, tg.pos[0])) s |= ST_NONFINITE;
    a.flags[t32] = fl | FL_STARTED;
    if (ev.status_events) (ev.status_events + (size_t)(n - 1) * T)[t32] = s;
    if (a.status) a.status[t32] = s;
}

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::events_kernel_t imu9ev_of(int as) {
    if (as == 8) return k_events_imu9<REAL, MREAL, 8>;
    return k_events_imu9<REAL, MREAL, 0>;
}
kfpos_k::events_kernel_t kfpos_k::imu9_events_kernel(int st, int as) {
    return KFPOS_BY_STORAGE(st, imu9ev_of, as);
}
