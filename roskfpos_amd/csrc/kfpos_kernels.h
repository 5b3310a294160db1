/*
 * kfpos_kernels.h -- the device side of what the kernel translation units of libkfpos_hip.so share: the helpers that
 * bring a tag's state and an epoch into registers / LDS (component-major HBM) and take the state back out. The
 * kernel-argument blocks, the selectors and the list of translation units: kfpos_kargs.h. No host unit includes this
 * header, and it includes nothing of the host side (the handle, kfpos_host.h).
 *
 * Execution model: ONE FILTER PER LANE, 64 filters per wavefront, one wavefront per workgroup.
 *  - The whole per-tag state (position, velocity, packed covariance: 21 / 36 / 45 doubles) lives in
 *    VGPRs/AGPRs for the duration of a step -- and across the epochs of a multi-epoch launch; every array
 *    index in kfpos_core.h is a compile-time constant after unrolling. At 65 536 tags there is exactly one
 *    wavefront per SIMD (1024 waves on 256 CUs x 4 SIMDs), so the 512-register file per lane is free to use.
 *    No kernel may spill to scratch inside a loop (checked at build time, tools/check_scratch.py).
 *  - HBM layout is component-major ([component][tag]): lane l of a wave reads element
 *    base + tag0 + l, so every state / measurement access is one fully coalesced
 *    512-byte (f64) or 256-byte (f32 / int32) wave transaction, each byte touched once.
 *  - The epoch's measurements -- range in metres (the integer-mm wire value converted once, with the
 *    reference's exact `(double) mm / 1000`, Posgenerator.cpp:484), errorEstimation, working weight (1/e for
 *    the ML sweeps, 1/R for the IEKF sweeps) -- live in registers for 8 anchors (RegScratch) and per lane in
 *    LDS otherwise, [anchor][lane] (lane-consecutive 8-byte words: conflict-free ds_read_b64), with
 *    compile-time anchor loops for 16 anchors (StaticScratch) and a run-time loop for every other count. The
 *    inner sweeps (2-4 ML + 3-20 IEKF per step) then touch only registers / LDS + SGPRs, never HBM.
 *  - Anchor coordinates are wave-uniform: they travel in the kernel-argument segment and are read
 *    with scalar loads into SGPRs.
 *  - No MFMA: the largest dense object is 9x9 per filter; lanes are independent filters, so there is nothing to
 *    shuffle and no barrier (the exception: the 8-lanes-per-tag kernel of small banks, kfpos_k_coop.hip).
 */
#ifndef KFPOS_KERNELS_H
#define KFPOS_KERNELS_H

#include <cmath>

#include "kfpos_kargs.h" /* defines KFPOS_HD for the two below */
#include "kfpos_core.h"
#include "kfpos_stored.h" /* ldrow, strow, ldcov, stcov, round_cov, KFPOS_BY_STORAGE; kfpos_p48.h */

namespace {

using namespace kfpos;

/* (The loops that bring a tag's covariance in, take it out with the finite check, store a pose row and round between two
 * epochs stay open text in every kernel: behind a helper that is handed the tag's state, in each of the forms tried, every
 * kernel that called it came out with other code -- profiles/HISTORY.md, "Kernel headers". What takes scalars alone can
 * be shared: ldcov / stcov / round_cov, and nonfinite_state below.) */
/* is a state that is `fin`ite or not an error? Not while the tag still waits for its ML initialisation (no start position
 * given, first coordinate NaN): the one place that says what KFPOS_ST_NONFINITE means */
__device__ inline bool nonfinite_state(bool fin, int use_init_pos, double pos0) {
    const bool waiting = !use_init_pos && isnan(pos0);
    return !fin && !waiting;
}

template <class P>
__device__ inline P make_params_of(const KArgs &a) {
    P pr;
    pr.anchors = a.anchors;
    pr.n_anchors = a.A;
    pr.accel_noise = a.accel_noise;
    pr.jolt = a.jolt;
    pr.cost_threshold = a.cost_threshold;
    pr.ignore_worst = a.ignore_worst;
    pr.top_n = a.top_n;
    pr.ml_variant = a.ml_variant;
    pr.use_init_pos = a.use_init_pos;
    pr.use_fixed_height = a.use_fixed_height;
    pr.imu_fixed_cov_acc = a.imu_fixed_cov_acc;
    pr.imu_fixed_cov_w = a.imu_fixed_cov_w;
    pr.px4_height = a.px4_height;
    pr.px4_arm_p1 = a.px4_arm_p1;
    pr.px4_arm_p2 = a.px4_arm_p2;
    pr.px4_cov_vel = a.px4_cov_vel;
    pr.px4_cov_gyro_z = a.px4_cov_gyro_z;
    pr.imu_cov_acc = a.imu_cov_acc;
    pr.imu_cov_w = a.imu_cov_w;
    pr.mag_offset = a.mag_offset;
    pr.mag_cov = a.mag_cov;
    return pr;
}
__device__ inline Params make_params(const KArgs &a) { return make_params_of<Params>(a); }
/* the anchor table of this workgroup's cell: what Params::anchors points at in a kernel built around CellArgs */
__device__ inline const double *cell_anchors(const CellArgs &c) {
    const int cell = ((kfpos_k::cell_map_t)c.cell_of_block)[blockIdx.x];
    return (const double *)((kfpos_k::cell_table_t)c.cell_xyz + (size_t)cell * c.cell_stride);
}

/* The 6-state selector table, once for every kernel family that has these forms (k_step_toa6 around either argument
 * block: kfpos_k_toa6.inc; k_trace_toa6_each: kfpos_k_toa6each.inc): FAM::kernel<SYMM, REAL, MREAL, AS, HEUR>() is the
 * family's instantiation. heur: 0 = the bank has no outlier heuristic (BASELINE configs 2 and 4), 1 = top-N only
 * (config 5), 2 = leave-one-out (with or without top-N). 0 and 1 get instantiations with no leave-one-out loop compiled
 * in: 13 % faster at 8 anchors. Combinations that run the AS = 0 form because their own would touch scratch memory
 * inside the epoch loop (make check): DESIGN.md section 6 lists them. */
template <class FAM, bool SYMM, typename REAL, typename MREAL>
auto toa6_table(int as, int heur) -> decltype(FAM::template kernel<SYMM, REAL, MREAL, 0, 0>()) {
    if constexpr (SYMM) {
        if (as == 8) return heur ? FAM::template kernel<true, REAL, MREAL, 8, 2>() : FAM::template kernel<true, REAL, MREAL, 8, 0>();
    } else {
        /* non-symmetric layout (ML initialisation): its SVD path needs the registers a resident epoch would take
         * (148-180 bytes/lane of scratch otherwise), so the 8-anchor epoch goes to LDS, loops still compile-time */
        if (as == 8) {
            if (!heur) return FAM::template kernel<false, REAL, MREAL, -8, 0>();
            /* (leave-one-out with the 48-bit covariance: the host never asks -- kfpos_create -- and the instantiation
             * is not built: it would access scratch memory inside its epoch loop) */
            if constexpr (!std::is_same<REAL, p48>::value) return FAM::template kernel<false, REAL, MREAL, -8, 2>();
        }
    }
    if (as == -16) return heur == 1 ? FAM::template kernel<SYMM, REAL, MREAL, -16, 1>() : FAM::template kernel<SYMM, REAL, MREAL, -16, 2>();
    return heur ? FAM::template kernel<SYMM, REAL, MREAL, 0, 2>() : FAM::template kernel<SYMM, REAL, MREAL, 0, 0>();
}

/* Raw epoch of one tag as it sits in HBM: fetched one epoch ahead in multi-epoch launches, so its
 * latency hides behind the previous epoch's arithmetic. */
template <typename MREAL, int AS>
struct RawEpoch {
    int32_t mm[AS];
    MREAL e[AS];
};
template <typename MREAL, int AS>
__device__ inline void fetch_epoch(const KArgs &a, size_t t, int s, RawEpoch<MREAL, AS> &raw) {
    const int32_t *rp = a.ranges + (size_t)s * a.stride_ranges;
    const MREAL *ep = (const MREAL *)a.err + (size_t)s * a.stride_err;
#pragma unroll
    for (int k = 0; k < AS; ++k) { /* all loads first: one latency, not AS of them */
        raw.mm[k] = (rp + (size_t)k * a.T)[(uint32_t)t];
        raw.e[k] = (ep + (size_t)k * a.T)[(uint32_t)t];
    }
}
template <typename MREAL, int AS>
__device__ inline void unpack_epoch(const RawEpoch<MREAL, AS> &raw, RegScratch<AS> &sc) {
#pragma unroll
    for (int k = 0; k < AS; ++k) {
        sc.r[k] = raw.mm[k] > 0 ? kf_mm_to_m(raw.mm[k]) : 0.0; /* Posgenerator.cpp:483-484 */
        sc.e[k] = (double)raw.e[k];
        sc.w[k] = 0.0;
    }
}
/* generic anchor count: epoch s -> per-lane LDS scratch */
template <typename MREAL>
__device__ inline Scratch stage_epoch_lds(const KArgs &a, double *lds, int lane, size_t t, int s) {
    Scratch sc;
    sc.r = lds + lane;
    sc.e = lds + (size_t)a.A * WAVE + lane;
    sc.w = lds + 2 * (size_t)a.A * WAVE + lane;
    sc.stride = WAVE;
    const int32_t *rp = a.ranges + (size_t)s * a.stride_ranges;
    const MREAL *ep = (const MREAL *)a.err + (size_t)s * a.stride_err;
    for (int k = 0; k < a.A; ++k) {
        const int32_t mm = (rp + (size_t)k * a.T)[(uint32_t)t];
        sc.r[k * WAVE] = mm > 0 ? kf_mm_to_m(mm) : 0.0;
        sc.e[k * WAVE] = (double)(ep + (size_t)k * a.T)[(uint32_t)t];
    }
    return sc;
}
/* anchor count known at compile time: all 2 N loads first, then the conversions and the LDS stores */
template <typename MREAL, int N>
__device__ inline StaticScratch<N> stage_epoch_lds_n(const KArgs &a, double *lds, int lane, size_t t, int s) {
    StaticScratch<N> sc;
    sc.r = lds + lane;
    sc.e = lds + (size_t)N * WAVE + lane;
    sc.w = lds + 2 * (size_t)N * WAVE + lane;
    sc.stride = WAVE;
    RawEpoch<MREAL, N> raw;
    fetch_epoch<MREAL, N>(a, t, s, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sc.r[k * WAVE] = raw.mm[k] > 0 ? kf_mm_to_m(raw.mm[k]) : 0.0;
        sc.e[k * WAVE] = (double)raw.e[k];
    }
    return sc;
}
/* ---- 9-state kernels (kfpos_k_imu9.inc, kfpos_k_imu9ev.hip): the accelerometer sample and its covariance ---- */
/* The acceleration sample is fetched one epoch ahead like the ranges. Its covariance is loaded and whitened ONCE per
 * launch: a multi-epoch launch always has one covariance array for all its epochs (stride_cov = 0: a sensor with a
 * fixed covariance); a trace with a covariance per epoch is replayed one epoch per launch (kfpos_run_trace_dev). */
template <typename MREAL>
struct RawImu {
    MREAL acc[3];
};
template <typename MREAL>
__device__ inline void fetch_imu(const KArgs &a, size_t t, int s, RawImu<MREAL> &raw) {
    const MREAL *ap = (const MREAL *)a.accel + (size_t)s * a.stride_accel;
#pragma unroll
    for (int k = 0; k < 3; ++k) raw.acc[k] = (ap + (size_t)k * a.T)[(uint32_t)t];
}
template <typename MREAL>
__device__ inline void fetch_imu_cov(const KArgs &a, size_t t, int s, MREAL raw[9]) {
    const MREAL *cp = (const MREAL *)a.cov + (size_t)s * a.stride_cov;
#pragma unroll
    for (int k = 0; k < 9; ++k) raw[k] = (cp + (size_t)k * a.T)[(uint32_t)t];
}
template <typename MREAL>
__device__ inline void latch_imu_cov(const KArgs &a, size_t T, uint32_t t32, const double cv[9]) {
    strow<MREAL>(a.imu_cov, 0, T, t32, cv[0]);
    strow<MREAL>(a.imu_cov, 1, T, t32, cv[3]);
    strow<MREAL>(a.imu_cov, 2, T, t32, cv[4]);
    strow<MREAL>(a.imu_cov, 3, T, t32, cv[6]);
    strow<MREAL>(a.imu_cov, 4, T, t32, cv[7]);
    strow<MREAL>(a.imu_cov, 5, T, t32, cv[8]);
}

/* step_imu9_state's `fast`: the wavefront's accelerometer covariances are diagonal (diag: decided per launch) and every
 * lane that is about to run the step has a sample -- one ballot over the lanes that are here */
__device__ inline bool imu9_fast(bool diag, bool has) {
    return diag && __builtin_amdgcn_ballot_w64(!has) == 0;
}
/* A wave-uniform epoch index the optimiser cannot see through: addresses derived from it are formed anew in every
 * epoch (a few scalar instructions) instead of living as two dozen running row pointers across the whole epoch loop,
 * where they exhaust the scalar registers and end up as spilled 64-bit per-lane addresses. */
__device__ inline int opaque_uniform(int v) {
    asm volatile("" : "+s"(v));
    return v;
}
/* the same for the lane's tag index: its per-array 64-bit addresses are then formed where they are used instead of
 * being carried (spilled) across the epoch loop */
__device__ inline size_t opaque_lane(size_t t) {
    uint32_t v = (uint32_t)t;
    asm volatile("" : "+v"(v));
    return v;
}
/* the same with 4-byte errorEstimations kept as they are: LDS = r [N][lane] f64 | w [N][lane] f64 | e [N][lane] f32 */
template <int N>
__device__ inline StaticScratchF<N> stage_epoch_lds_nf(const KArgs &a, double *lds, int lane, size_t t, int s) {
    StaticScratchF<N> sc;
    sc.r = lds + lane;
    sc.w = lds + (size_t)N * WAVE + lane;
    sc.e = (float *)(lds + 2 * (size_t)N * WAVE) + lane;
    sc.stride = WAVE;
    RawEpoch<float, N> raw;
    fetch_epoch<float, N>(a, t, s, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sc.r[k * WAVE] = raw.mm[k] > 0 ? kf_mm_to_m(raw.mm[k]) : 0.0;
        sc.e[k * WAVE] = raw.e[k];
    }
    return sc;
}
/* doubles of LDS the epoch of a compile-time-count kernel takes per workgroup */
template <typename MREAL, int N>
constexpr size_t static_epoch_doubles() { return kfpos_plan::static_epoch_doubles(sizeof(MREAL), N); }
__device__ inline double epoch_dt(const KArgs &a, size_t t, int s) {
    return a.n_steps > 1 ? a.dt_steps[s] : (a.dt ? a.dt[(uint32_t)t] : a.dt_shared);
}

/* a lane that sits a call out (dt < 0, or a dropped PX4Flow sample) still reports where its tag is: the trajectory /
 * pose output of the call carries the untouched position (what getPose at timeLag 0 would return) */
__device__ inline void skipped_lane(const KArgs &a, size_t t, bool write) {
    if (!write) return;
    if (a.status) a.status[t] = ST_SKIPPED;
    if (a.traj) {
#pragma unroll
        for (int k = 0; k < 3; ++k) (a.traj + (size_t)k * a.T)[(uint32_t)t] = (a.pos + (size_t)k * a.T)[(uint32_t)t];
    }
}

} // namespace
#endif /* KFPOS_KERNELS_H */
