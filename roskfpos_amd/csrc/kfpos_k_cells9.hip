/*
 * kfpos_k_cells9.hip -- k_cells_imu9: the 9-state UWB + IMU ranging round (MODE_TOA, MODE_FUSED) of a bank with anchor
 * cells (kfpos_set_anchor_cells). IMU-only rounds read no anchor and stay with k_step_imu9.
 */
#include "kfpos_kernels.h"

namespace {

typedef const __attribute__((address_space(4))) double *cell_table_t;
typedef const __attribute__((address_space(4))) int32_t *cell_map_t;

/* k_step_imu9 (kfpos_k_imu9.hip) in the plain order of an epoch -- step_imu9_state + step_imu9_cov, the branch every
 * instantiation but the bench kernel takes there -- without the pairs' tail and without the rotated loop, both of which
 * compute the same bits as this form. The one difference: the anchor table is the table of the workgroup's
 * cell, cell_xyz + cell_of_block[blockIdx.x] * cell_stride in device memory, read through a pointer in the constant
 * address space (wave-uniform: scalar loads), not KArgs::anchors. Loads, stores and the arithmetic of a lane are
 * k_step_imu9's, so a block of cell c computes bit for bit what k_step_imu9 computes for its rows with cell c's table in
 * KArgs::anchors. The host has checked every entry of cell_of_block against n_cells. */
template <typename REAL, typename MREAL, int AS>
__global__ __launch_bounds__(WAVE) void k_cells_imu9(const kfpos_k::CellArgs c) {
    extern __shared__ double lds[];
    const KArgs &a = c.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    Params pr = make_params(a);
    const int cell = ((cell_map_t)c.cell_of_block)[blockIdx.x];
    pr.anchors = (const double *)((cell_table_t)c.cell_xyz + (size_t)cell * c.cell_stride);
    /* fetching one epoch AHEAD and the peeled Gauss-Newton text: the rules of k_step_imu9 */
    constexpr bool AHEAD = sizeof(MREAL) == 4 && !std::is_same<REAL, float>::value;
    constexpr bool PEEL = AS != 8 || AHEAD;
    constexpr bool IMU_WITH_EPOCH = AHEAD && AS > 0;
    const bool fresh_imu = a.mode != MODE_TOA;
    constexpr int NA = AS > 0 ? AS : 1;
    double dt_tag = a.dt_shared; /* the dt of a single-epoch call */
    if (a.n_steps == 1 && a.dt) {
        dt_tag = a.dt[t32];
        if (dt_tag < 0.0) { /* no epoch / sample for this tag in this call */
            skipped_lane(a, t, true);
            return;
        }
    }

    /* load order = order of first use (k_step_imu9): flags, epoch, position, velocity, IMU sample, covariance */
    uint32_t fl = a.flags[t32];
    RawEpoch<MREAL, NA> raw;
    RawImu<MREAL> rawi;
    if constexpr (AS > 0) fetch_epoch<MREAL, AS>(a, t, 0, raw);
    Tag9 tg;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tg.pos[k] = (a.pos + k * T)[t32];
        tg.vel[k] = (a.vel + k * T)[t32];
    }
    /* the covariance and B^-1 wait in LDS while the gain iteration runs, the accelerometer whitener for the whole
     * launch: [78][lane], behind the generic kernel's epoch scratch */
    const CovPark9 park{lds + (AS == 0 ? 3 * (size_t)a.A * WAVE : 0) + lane, WAVE};
    Imu imu;
    imu.has = false;
    imu.ci = park.a + 66 * WAVE;
    imu.ci_stride = WAVE;
    double cv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    MREAL rawc[9];
    if (fresh_imu) {
        fetch_imu<MREAL>(a, t, 0, rawi);
        fetch_imu_cov<MREAL>(a, t, 0, rawc);
    } else if (fl & FL_HAS_IMU) { /* re-fuse the latched sample (KalmanFilterTOAIMU.cpp:68-72) */
        imu.has = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) imu.acc[k] = ldrow<MREAL>(a.imu_acc, k, T, t32);
        cv[0] = ldrow<MREAL>(a.imu_cov, 0, T, t32);
        cv[3] = ldrow<MREAL>(a.imu_cov, 1, T, t32);
        cv[4] = ldrow<MREAL>(a.imu_cov, 2, T, t32);
        cv[6] = ldrow<MREAL>(a.imu_cov, 3, T, t32);
        cv[7] = ldrow<MREAL>(a.imu_cov, 4, T, t32);
        cv[8] = ldrow<MREAL>(a.imu_cov, 5, T, t32);
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, 45, T, t32);
    if (fresh_imu) { /* the covariance of the first (usually: of every) epoch of this launch */
        imu.has = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) cv[k] = (double)rawc[k];
        if (a.latch) latch_imu_cov<MREAL>(a, T, t32, cv);
    }
    if (imu.has) imu_whitener(cv, imu.ci, imu.ci_stride);
    /* the diagonal form of the gain iteration's pass, decided per launch and per wavefront as in k_step_imu9 */
    bool diag = false;
    if (a.imu9_diag) {
        const bool mine = !imu.has || (imu.Wi(1) == 0.0 && imu.Wi(2) == 0.0 && imu.Wi(4) == 0.0);
        diag = __builtin_amdgcn_ballot_w64(mine) == __builtin_amdgcn_ballot_w64(true);
    }
    const bool fast = imu9_fast(diag, imu.has);

    const bool multi = a.n_steps > 1; /* wave-uniform: dt sits in the kernel arguments, read one epoch ahead */
    double dt_next = multi ? a.dt_steps[0] : dt_tag;
    __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0): everything loaded so far has arrived before the loop (k_step_imu9) */
    uint32_t s = 0;
    for (int e = 0; e < a.n_steps; ++e) { /* the state stays in registers from epoch to epoch */
        const double dt = dt_next;
        if (multi && e + 1 < a.n_steps) dt_next = a.dt_steps[opaque_uniform(e + 1)];
        if (fresh_imu) { /* fresh sample: newIMUMeasurement latches it (KalmanFilterTOAIMU.cpp:78-89) */
#pragma unroll
            for (int k = 0; k < 3; ++k) imu.acc[k] = (double)rawi.acc[k];
            if constexpr (AHEAD && !IMU_WITH_EPOCH) {
                if (e + 1 < a.n_steps) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
            }
        }
        /* the step in two parts with the pose store between them (k_step_imu9) */
        Iekf9Out o;
        auto finish = [&](bool update) {
            if (a.traj) {
#pragma unroll
                for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
            }
            if (update) s = step_imu9_cov(tg, o, imu);
        };
        if constexpr (AS > 0) {
            RegScratch<AS> sc;
            unpack_epoch<MREAL, AS>(raw, sc);
            if (e + 1 < a.n_steps) {
                if constexpr (AHEAD) {
                    fetch_epoch<MREAL, AS>(a, opaque_lane(t), opaque_uniform(e + 1), raw);
                    if constexpr (IMU_WITH_EPOCH) {
                        if (fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
                    }
                }
            }
            finish(step_imu9_state<true, true, false, true, PEEL>(tg, sc, pr, dt, imu, park, fast, o, s));
            if constexpr (!AHEAD) { /* 8-byte measurements: the next epoch is fetched when this one is over */
                if (e + 1 < a.n_steps) {
                    if (fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
                    fetch_epoch<MREAL, AS>(a, opaque_lane(t), opaque_uniform(e + 1), raw);
                }
            }
        } else {
            Scratch sc = stage_epoch_lds<MREAL>(a, lds, lane, t, opaque_uniform(e));
            finish(step_imu9_state<true, true, false, true, PEEL>(tg, sc, pr, dt, imu, park, fast, o, s));
            if constexpr (!AHEAD) { /* the ranges are staged per epoch above; the next accelerometer sample is not */
                if (e + 1 < a.n_steps && fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
            }
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what n single-epoch launches would have kept in HBM */
            if (e + 1 < a.n_steps) {
#pragma unroll
                for (int k = 0; k < 45; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }

    if (fresh_imu && a.latch) { /* the last epoch's sample stays latched (lastImuMeasurement, KalmanFilterTOAIMU.cpp:78-89) */
#pragma unroll
        for (int k = 0; k < 3; ++k) strow<MREAL>(a.imu_acc, k, T, t32, imu.acc[k]);
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
    const bool waiting = !a.use_init_pos && isnan(tg.pos[0]);
    if (!fin && !waiting) s |= ST_NONFINITE;
    a.flags[t32] = fl | FL_STARTED;
    if (a.status) a.status[t32] = s;
}

} // namespace

template <typename REAL, typename MREAL>
static kfpos_k::cells_kernel_t cells_imu9_of(int as) {
    if (as == 8) return k_cells_imu9<REAL, MREAL, 8>;
    return k_cells_imu9<REAL, MREAL, 0>;
}
kfpos_k::cells_kernel_t kfpos_k::cells_imu9_kernel(int st, int as) { return KFPOS_BY_STORAGE(st, cells_imu9_of, as); }
