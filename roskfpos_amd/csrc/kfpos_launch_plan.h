/*
 * kfpos_launch_plan.h -- launch selection: which instantiation a handle runs for a launch, over how many workgroups, with
 * how many bytes of dynamic LDS. One function from (what the handle is, what is launched) to a Plan; the host units map a
 * Plan to a function pointer through the selectors of kfpos_kargs.h and launch it, and compute neither a form nor a
 * byte count themselves. Pure arithmetic: no HIP header, g++ compiles it alone (tests/launch/launch_driver.cpp walks
 * every configuration against a table read from the kernels). The plan takes no tag count: a row-list step of n tags
 * runs the whole bank's kernel by signature.
 */
#ifndef KFPOS_LAUNCH_PLAN_H
#define KFPOS_LAUNCH_PLAN_H

#include <cstddef>

#include "../../include/kfpos.h"

namespace kfpos_k {
constexpr int COOP_LANES = 8; /* kfpos_k_coop.hip: one tag per group of 8 lanes */
constexpr int COOP_TAGS_PER_WAVE = 64 / COOP_LANES;
} // namespace kfpos_k

namespace kfpos_plan {

constexpr int LANES = 64; /* lanes per workgroup = one wavefront = one tag each, but for the 8-lanes-per-tag kernel */

/* ---- doubles of LDS per workgroup, as the kernels address them: the epoch first, the park behind it ---- */
/* the run-time loop's epoch of max_anchors: range, errorEstimation, weight, [anchor][lane] */
constexpr size_t loop_epoch_doubles(int max_anchors) { return (size_t)3 * max_anchors * LANES; }
/* the epoch of a compile-time-count kernel; the 6-state ones keep 4-byte errorEstimations as they are: 20 bytes per
 * anchor and lane */
constexpr size_t static_epoch_doubles(size_t msz, int n) { return msz == 4 ? (size_t)n * LANES * 5 / 2 : (size_t)n * LANES * 3; }
/* 36 per lane: CovSpill8 (planar), Pinv6 (6-state, non-symmetric layout) */
constexpr size_t PARK_DOUBLES = 36 * LANES;
/* CovPark9: the 9-state covariance (45) and B^-1 (21) during the gain iteration, the accelerometer whitener and Sigma^-1
 * (12), a lane-addressable copy of 8 anchors at [78 * LANES]: 39.2 KB per wavefront, four wavefronts per CU; beside the
 * run-time loop's epoch of up to 64 anchors 96 + 39.2 = 135.2 KB of the CU's 160 */
constexpr size_t PARK9_DOUBLES = 78 * LANES + 24;
/* k_step_toa6_w2: covariance entries per lane parked during the ML solve -- what 160 KB / 8 leave next to the epoch */
constexpr int toa6_w2_park(size_t msz) { return msz == 4 ? 19 : 15; }

/* what the decision depends on. kfpos_policy.h derives them from a configuration (environment, device, the 8 192-tag
 * limit of coop, p48 + full + leave-one-out = force_generic) and says which combinations exist: producible() */
struct Inputs {
    int model, storage, max_anchors;
    bool full, ignore_worst, top_n;
    bool force_generic, coop, two_waves, planar_sensors;
};

/* what is launched. STEP_IMU_ONLY exists for the 9-state filter, STEP_SENSOR for the planar one (elsewhere they plan as
 * STEP_RANGING); the replays of shared and of per-tag timelines take the same plan */
enum Launch : int { STEP_RANGING, STEP_IMU_ONLY, STEP_SENSOR, TRACE6_EACH, EVENTS9, EVENTS_PLANAR };

struct Plan {
    int as, heur;                     /* the selectors' arguments (kfpos_kargs.h) ... */
    bool sensors, ranging, two_waves; /* ... planar_kernel, imu9_kernel, toa6_sym_kernel */
    int tags_per_group;
    size_t epoch_doubles, park_doubles;
    size_t park_offset() const { return epoch_doubles; }
    size_t bytes() const { return (epoch_doubles + park_doubles) * sizeof(double); }
    int groups(int n_tags) const { return (n_tags + tags_per_group - 1) / tags_per_group; }
};

/* Anchor-count specialisation. 8 anchors (BASELINE configs 2-4): epoch in registers (RegScratch), as = 8. 16 anchors
 * (config 5, 6-state): a register-resident epoch costs 96 more live registers and spills to scratch, which is no faster
 * than the run-time loop (measured in round 1), so the epoch stays in LDS and only the anchor loops are compile-time, in
 * groups of 8 (StaticScratch): as = -16. Everything else: 0, the run-time loop. Where an 8-anchor kernel needs the
 * registers for something else -- the SVD of the non-symmetric layout, the planar filter's sensor rows, a second
 * wavefront on the SIMD -- its selector answers as = 8 with the compile-time loops over an LDS-resident epoch.
 * "No scratch" is a PERFORMANCE rule of this library (checked at build time), not a correctness crutch: round 1 saw
 * wrong, run-to-run varying positions from a work-in-progress build of the spilling 16-anchor kernel and dropped it
 * without a diagnosis. Round 2 could not reproduce that with the committed sources of either round -- the library as it
 * stood before that commit and today's kernels with the register-resident 16-anchor instantiations re-enabled
 * (236-960 bytes/lane of scratch) match the oracle and repeat bit for bit on full, partially filled and
 * skipped-lane wavefronts (tools/exp/, profiles/r02b_*) -- and a MemorySanitizer build of the kernel body with every
 * undefined input poisoned is clean (tests/emu/msan_audit.sh). DESIGN.md section 2. */
inline Plan plan(Inputs in, Launch what) {
    const bool toa = in.model == KFPOS_MODEL_TOA, imu9 = in.model == KFPOS_MODEL_TOA_IMU, planar = in.model == KFPOS_MODEL_PLANAR;
    const size_t msz = in.storage == KFPOS_STORE_F64 ? 8 : 4;
    Plan p{};
    p.ranging = true;
    p.tags_per_group = LANES;
    if (toa && in.coop) { /* 8 lanes per tag: no epoch scratch, no park (a coop handle's trace runs single calls) */
        p.tags_per_group = kfpos_k::COOP_TAGS_PER_WAVE;
        return p;
    }
    const bool sensor_call = planar && what == STEP_SENSOR;
    p.ranging = !(imu9 && what == STEP_IMU_ONLY);
    /* ranging epochs carry the latched samples once there are some; a replay latches them itself */
    p.sensors = planar && (in.planar_sensors || sensor_call || what == EVENTS_PLANAR);
    /* heur: 0 = the bank has no outlier heuristic (BASELINE configs 2 and 4), 1 = top-N only (config 5), 2 =
     * leave-one-out (with or without top-N) */
    p.heur = !toa ? 0 : in.ignore_worst ? 2 : in.top_n ? 1 : 0;
    p.as = (in.force_generic || sensor_call) ? 0 : in.max_anchors == 8 ? 8 : (in.max_anchors == 16 && toa) ? -16 : 0;
    /* the plain 8-anchor symmetric bank with more wavefronts than SIMDs: the 256-register build (k_step_toa6_w2). The
     * per-tag trace of such a bank runs the register form: the same bits */
    p.two_waves = in.two_waves && toa && !in.full && p.as == 8 && p.heur == 0 && what != TRACE6_EACH;
    const bool lds8 = p.as == 8 && ((toa && in.full) || p.two_waves || p.sensors);
    if (!p.ranging || sensor_call) p.epoch_doubles = 0;
    else if (p.as == 0) p.epoch_doubles = loop_epoch_doubles(in.max_anchors);
    else if (p.as == -16 || lds8) p.epoch_doubles = static_epoch_doubles(toa ? msz : 8, p.as == 8 ? 8 : 16);
    p.park_doubles = imu9 ? PARK9_DOUBLES : ((toa && in.full) || p.sensors) ? PARK_DOUBLES : p.two_waves ? (size_t)toa6_w2_park(msz) * LANES : 0;
    if (what == EVENTS_PLANAR && p.as == 8) p.as = -8; /* the planar replay selectors are handed the form itself */
    return p;
}

} // namespace kfpos_plan
#endif /* KFPOS_LAUNCH_PLAN_H */
