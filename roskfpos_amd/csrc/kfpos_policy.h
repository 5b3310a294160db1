/*
 * kfpos_policy.h -- what kfpos_create decides before it allocates anything: which configurations it refuses, and the
 * launch policy of the handle, a function of (configuration, wavefront slots of the device, KFPOS_* environment). Every
 * rule and the measurement behind it is stated here and nowhere else; the handle keeps the result (kfpos_handle::policy),
 * and kfpos_launch_plan.h turns it into kernel forms. Pure: no HIP header, the environment through a getter, g++ compiles
 * it alone (tests/policy/policy_driver.cpp walks it against a table read off the rules).
 */
#ifndef KFPOS_POLICY_H
#define KFPOS_POLICY_H

#include <cstddef>
#include <cstdio>
#include <cstdlib>

#include "../../include/kfpos.h"
#include "kfpos_launch_plan.h"

namespace kfpos_policy {

/* why kfpos_create refuses this configuration (KFPOS_ERR_ARG, the text behind kfpos_last_error), or null */
inline const char *config_refusal(const kfpos_config &cfg) {
    if (cfg.model != KFPOS_MODEL_TOA && cfg.model != KFPOS_MODEL_TOA_IMU && cfg.model != KFPOS_MODEL_ML &&
        cfg.model != KFPOS_MODEL_PLANAR)
        return "kfpos_config.model is not one of KFPOS_MODEL_*";
    if (cfg.storage != KFPOS_STORE_F64 && cfg.storage != KFPOS_STORE_F32 && cfg.storage != KFPOS_STORE_MIXED &&
        cfg.storage != KFPOS_STORE_P48)
        return "kfpos_config.storage is not one of KFPOS_STORE_*";
    if (cfg.n_tags < 1) return "kfpos_config.n_tags must be >= 1";
    if (cfg.max_anchors < 1 || cfg.max_anchors > KFPOS_MAX_ANCHORS)
        return "kfpos_config.max_anchors must be 1..64 (MAX_NUM_ANCS, Posgenerator.h:74)";
    if (cfg.top_n < 0) return "kfpos_config.top_n must be >= 0";
    if (cfg.ml_variant != KFPOS_ML_NORMAL && cfg.ml_variant != KFPOS_ML_IGNORE_N && cfg.ml_variant != KFPOS_ML_BEST)
        return "kfpos_config.ml_variant is not one of KFPOS_ML_*";
    if (cfg.ml_variant != KFPOS_ML_NORMAL && cfg.model != KFPOS_MODEL_ML)
        return "kfpos_config.ml_variant belongs to KFPOS_MODEL_ML (MLLocation's variants, MLLocation.h:5-7)";
    if ((cfg.model == KFPOS_MODEL_TOA_IMU && (cfg.top_n || cfg.ignore_worst)) ||
        (cfg.model == KFPOS_MODEL_ML && cfg.ignore_worst) ||
        (cfg.model == KFPOS_MODEL_PLANAR && (cfg.top_n || cfg.ignore_worst)))
        return "ignore_worst exists for the 6-state filter only, top_n for the 6-state filter and the ML estimator";
    return nullptr;
}

/* COV_FULL layout: the 6-state filter with ML initialisation (non-symmetric P) */
inline bool full_layout(const kfpos_config &cfg) { return cfg.model == KFPOS_MODEL_TOA && !cfg.use_init_pos; }

/* The meeting points of the 9-state pairs' tail (iekf9_next_meet): after `first` solves, after every solve up to
 * `dense_until`, then every 4. Default 8,10: after 8, 9 and 10 solves (8,8 = the schedule before this one: 8, then every
 * 4; the counters of profiles/imu9_pairs_meet_pmc.json chose it; profiles/HISTORY.md, "Where the lanes meet"). MAX: the cap
 * of the gain iteration. */
constexpr int PAIR9_MEET_FIRST = 8, PAIR9_MEET_DENSE_UNTIL = 10, PAIR9_MEET_MAX = 20;
inline bool pair9_meet_ok(int first, int dense_until) { return 1 <= first && first <= dense_until && dense_until <= PAIR9_MEET_MAX; }
constexpr const char *PAIR9_MEET_REFUSAL = "KFPOS_PAIR9_MEET must be first,dense_until with 1 <= first <= dense_until <= 20";

constexpr int TRACE_CHUNK_MAX = 128; /* KFPOS_TRACE_CHUNK (kfpos_kargs.h): the dt values of a launch travel in its arguments */

struct Policy {
    bool force_generic;    /* always the run-time-loop (LDS-staged) kernel */
    bool two_waves;        /* the plain 6-state bank has more wavefronts than the device has slots: the two-wavefront build */
    bool pair9;            /* 9-state bank, 8 anchors: iekf9_pairs for the tail of the gain iteration; bit-identical either way */
    int pair9_first, pair9_dense_until; /* ... and where the lanes of a wavefront meet to look for the hand-over */
    bool imu9_diag;        /* 9-state bank: wavefronts with diagonal accelerometer covariances take the diagonal form of the gain iteration (bit-identical) */
    bool coop;             /* small plain 6-state bank: one tag per 8 lanes (k_step_toa6_coop). kfpos_set_anchor_cells turns it off: the one mutation after kfpos_create */
    int trace_chunk;       /* epochs, events or slots per launch of the replay entry points, 1..TRACE_CHUNK_MAX */
    size_t small_bank_elems; /* elements of the range matrix (n_tags x max_anchors) up to which a bank is "small": one mapped block instead of staging copies */
    size_t slot_split_bytes; /* H2D copies of a streaming slot from this size on travel as two halves on two streams (0: never) */
};

/* The policy of a handle. wave_slots: multiProcessorCount * 4, or 0 where the device's properties could not be read
 * (never two-waves). env: getenv. false: KFPOS_PAIR9_MEET is not two integers that pair9_meet_ok (PAIR9_MEET_REFUSAL). */
inline bool policy(const kfpos_config &cfg, size_t wave_slots, const char *(*env)(const char *), Policy *out) {
    auto is = [&](const char *name, char c) {
        const char *e = env(name);
        return e && e[0] == c;
    };
    Policy p = {};
    /* KFPOS_GENERIC_KERNEL=1: A/B measurements, tests. One combination has no anchor-count-specialised kernel: ML start
     * (36-entry covariance + its SVD scratchpad) with leave-one-out and the 48-bit covariance -- the LDS-resident
     * 8-anchor instantiation would touch scratch memory inside its epoch loop (make check), the run-time-loop kernel does not */
    p.force_generic = is("KFPOS_GENERIC_KERNEL", '1') || (full_layout(cfg) && cfg.ignore_worst && cfg.storage == KFPOS_STORE_P48);
    /* more wavefronts than 4 per CU (KFPOS_ONE_WAVE_BUILD=1: never) */
    p.two_waves = !is("KFPOS_ONE_WAVE_BUILD", '1') && wave_slots > 0 &&
                  ((size_t)cfg.n_tags + kfpos_plan::LANES - 1) / kfpos_plan::LANES > wave_slots;
    /* on where it was measured to win -- the two kernels whose pair trips read registers only (4-byte measurements with
     * an 8- or 6-byte covariance: 2.8 % fewer cycles per epoch); the other two storage modes keep it opt-in.
     * KFPOS_PAIR9=0 / =1 overrides either way (profiles/HISTORY.md, "The pairs' tail") */
    const char *np = env("KFPOS_PAIR9");
    p.pair9 = np && np[0] ? np[0] == '1' : (cfg.storage == KFPOS_STORE_MIXED || cfg.storage == KFPOS_STORE_P48);
    /* KFPOS_PAIR9_MEET=first,dense_until; unset or empty = the default */
    p.pair9_first = PAIR9_MEET_FIRST;
    p.pair9_dense_until = PAIR9_MEET_DENSE_UNTIL;
    const char *pm = env("KFPOS_PAIR9_MEET");
    char rest = 0;
    if (pm && pm[0] && (std::sscanf(pm, "%d,%d%c", &p.pair9_first, &p.pair9_dense_until, &rest) != 2 ||
                        !pair9_meet_ok(p.pair9_first, p.pair9_dense_until)))
        return false;
    p.imu9_diag = !is("KFPOS_IMU9_DIAG", '0');
    /* up to 8 192 tags (1024 groups-of-8 wavefronts = one per SIMD) 8 lanes per tag pay off: 4.4-5.0 us per epoch
     * against 7.5 us; at 16 384 the one-tag-per-lane grid wins again (7.7 vs 8.3 us, measured). KFPOS_NO_COOP=1 disables */
    p.coop = !is("KFPOS_NO_COOP", '1') && !p.force_generic && cfg.model == KFPOS_MODEL_TOA && cfg.use_init_pos &&
             !cfg.ignore_worst && !cfg.top_n && cfg.max_anchors <= kfpos_k::COOP_LANES && cfg.n_tags <= 8192;
    const char *c = env("KFPOS_TRACE_CHUNK_STEPS");
    const int n = c ? std::atoi(c) : TRACE_CHUNK_MAX;
    p.trace_chunk = n < 1 ? 1 : (n > TRACE_CHUNK_MAX ? TRACE_CHUNK_MAX : n);
    const char *sb = env("KFPOS_SMALL_BANK_ELEMS");
    p.small_bank_elems = sb ? (size_t)std::atol(sb) : 4096;
    /* off: measured slower inside the pipeline (profiles/r02i_*) */
    const char *ss = env("KFPOS_SLOT_SPLIT_BYTES");
    p.slot_split_bytes = ss ? (size_t)std::atol(ss) : 0;
    *out = p;
    return true;
}

/* what launch selection depends on (kfpos_launch_plan.h): the configuration, the policy, and what the handle has become */
inline kfpos_plan::Inputs plan_inputs(const kfpos_config &cfg, const Policy &p, bool full, bool planar_sensors) {
    return {cfg.model, cfg.storage, cfg.max_anchors, full, cfg.ignore_worst != 0, cfg.top_n != 0,
            p.force_generic, p.coop, p.two_waves, planar_sensors};
}

/* The invariant of config_refusal and policy(): every Inputs an accepted configuration can lead to satisfies it (and
 * tests/launch/launch_driver.cpp sweeps exactly the Inputs that do). */
inline bool producible(const kfpos_plan::Inputs &in) {
    const bool toa = in.model == KFPOS_MODEL_TOA;
    if (in.full && !toa) return false; /* the non-symmetric layout: 6-state, ML start */
    if ((in.ignore_worst && !toa) || (in.top_n && !toa && in.model != KFPOS_MODEL_ML)) return false;
    if (in.coop && (!toa || in.force_generic || in.full || in.ignore_worst || in.top_n || in.max_anchors > kfpos_k::COOP_LANES)) return false;
    if (in.full && in.ignore_worst && in.storage == KFPOS_STORE_P48 && !in.force_generic) return false;
    return !in.planar_sensors || in.model == KFPOS_MODEL_PLANAR;
}

} // namespace kfpos_policy
#endif /* KFPOS_POLICY_H */
