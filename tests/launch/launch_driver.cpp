/* launch_driver.cpp -- roskfpos_amd/csrc/kfpos_launch_plan.h against what the kernels address, read from their sources and
 * written out here per form (not computed with the header's helpers). Every configuration kfpos_create can produce, every
 * kind of launch it can make; prints "OK <configurations>" or the first disagreement. tests/test_launch_plan.py builds it
 * with the address and undefined-behaviour sanitizers. */
#include <cstdio>
#include <cstdlib>

#include "kfpos_launch_plan.h"
#include "kfpos_policy.h"

using namespace kfpos_plan;

struct Expect {
    int as, heur;
    bool sensors, ranging, two_waves;
    int tags_per_group;
    size_t epoch, park; /* doubles per workgroup of 64 lanes */
};

/* the table: what each kernel form reads and writes of `extern __shared__ double lds[]` */
static Expect expect(const Inputs &in, Launch what) {
    const bool e4 = in.storage != KFPOS_STORE_F64, spec8 = in.max_anchors == 8 && !in.force_generic;
    const size_t loop = (size_t)192 * in.max_anchors; /* [3][max_anchors][64] */
    Expect x = {0, 0, false, true, false, 64, 0, 0};
    switch (in.model) {
    case KFPOS_MODEL_TOA:
        if (in.coop) { /* k_step_toa6_coop: no dynamic LDS, 8 tags per wavefront */
            x.tags_per_group = 8;
            return x;
        }
        x.heur = in.ignore_worst ? 2 : (in.top_n ? 1 : 0);
        x.park = in.full ? 2304 : 0; /* Pinv6 [36][64] behind the epoch */
        if (spec8) {
            x.as = 8;
            x.two_waves = in.two_waves && !in.full && x.heur == 0 && what != TRACE6_EACH;
            if (in.full || x.two_waves) x.epoch = e4 ? 1280 : 1536; /* r, w f64 | e f32, or r, e, w f64: [8][64] each */
            if (x.two_waves) x.park = e4 ? 64 * 19 : 64 * 15;
        } else if (in.max_anchors == 16 && !in.force_generic) {
            x.as = -16;
            x.epoch = e4 ? 2560 : 3072;
        } else {
            x.epoch = loop;
        }
        return x;
    case KFPOS_MODEL_TOA_IMU:
        x.park = 5016; /* CovPark9 [78][64] + the anchor table [24] */
        x.as = spec8 ? 8 : 0;
        x.ranging = what != STEP_IMU_ONLY;
        x.epoch = (x.ranging && !spec8) ? loop : 0;
        return x;
    case KFPOS_MODEL_ML:
        x.as = spec8 ? 8 : 0;
        x.epoch = spec8 ? 0 : loop;
        return x;
    default: /* KFPOS_MODEL_PLANAR */
        x.sensors = in.planar_sensors || what != STEP_RANGING;
        x.park = x.sensors ? 2304 : 0; /* CovSpill8 [36][64] behind the epoch */
        if (what == STEP_SENSOR) return x; /* as = 0, no epoch */
        x.as = spec8 ? (what == EVENTS_PLANAR ? -8 : 8) : 0;
        x.epoch = spec8 ? (x.sensors ? 1536 : 0) : loop; /* [3][8][64], 4-byte measurements widened */
        return x;
    }
}

static const char *const model_name[4] = {"toa", "toa_imu", "ml", "planar"};
static const char *const launch_name[6] = {"step_ranging", "step_imu_only", "step_sensor", "trace6_each", "events9", "events_planar"};

static int fail(const Inputs &in, Launch what, const char *why, const Plan &p) {
    std::printf("FAIL %s: model=%s storage=%d anchors=%d full=%d loo=%d topn=%d generic=%d coop=%d two_waves=%d sensors=%d launch=%s\n"
                "  plan: as=%d heur=%d sensors=%d ranging=%d two_waves=%d tags_per_group=%d epoch=%zu park=%zu bytes=%zu\n",
                why, model_name[in.model], in.storage, in.max_anchors, in.full, in.ignore_worst, in.top_n, in.force_generic, in.coop,
                in.two_waves, in.planar_sensors, launch_name[what], p.as, p.heur, p.sensors, p.ranging, p.two_waves,
                p.tags_per_group, p.epoch_doubles, p.park_doubles, p.bytes());
    return 1;
}

int main() {
    static_assert(KFPOS_MODEL_TOA == 0 && KFPOS_MODEL_TOA_IMU == 1 && KFPOS_MODEL_ML == 2 && KFPOS_MODEL_PLANAR == 3, "model_name");
    const int models[4] = {KFPOS_MODEL_TOA, KFPOS_MODEL_TOA_IMU, KFPOS_MODEL_ML, KFPOS_MODEL_PLANAR};
    const int storages[4] = {KFPOS_STORE_F64, KFPOS_STORE_F32, KFPOS_STORE_MIXED, KFPOS_STORE_P48};
    const int anchors[11] = {1, 7, 8, 9, 16, 17, 30, 31, 42, 43, 64};
    long ran = 0;
    size_t worst = 0;
    for (int model : models)
    for (int storage : storages)
    for (int A : anchors)
    for (int bits = 0; bits < 128; ++bits)
    for (int w = 0; w < 6; ++w) {
        const Inputs in = {model, storage, A, (bits & 1) != 0, (bits & 2) != 0, (bits & 4) != 0,
                           (bits & 8) != 0, (bits & 16) != 0, (bits & 32) != 0, (bits & 64) != 0};
        const Launch what = (Launch)w;
        const bool toa = model == KFPOS_MODEL_TOA, imu9 = model == KFPOS_MODEL_TOA_IMU, planar = model == KFPOS_MODEL_PLANAR;
        if (!kfpos_policy::producible(in)) continue; /* what kfpos_create refuses or never produces */
        /* launches no entry point makes */
        if ((what == STEP_IMU_ONLY || what == EVENTS9) && !imu9) continue;
        if ((what == STEP_SENSOR || what == EVENTS_PLANAR) && !planar) continue;
        if (what == TRACE6_EACH && (!toa || in.coop)) continue;           /* a coop handle's trace runs single calls */
        ++ran;
        const Plan p = plan(in, what);
        const Expect x = expect(in, what);
        const size_t bytes = (x.epoch + x.park) * 8;
        if (p.as != x.as || p.heur != x.heur || p.sensors != x.sensors || p.ranging != x.ranging || p.two_waves != x.two_waves)
            return fail(in, what, "selector arguments", p);
        if (p.tags_per_group != x.tags_per_group || p.groups(65) != (x.tags_per_group == 8 ? 9 : 2) || p.groups(64) != 64 / x.tags_per_group)
            return fail(in, what, "grid", p);
        if (p.epoch_doubles != x.epoch || p.park_doubles != x.park || p.bytes() != bytes) return fail(in, what, "LDS bytes", p);
        if (p.park_offset() != x.epoch) return fail(in, what, "park offset", p);
        if (p.bytes() > 160 * 1024) return fail(in, what, "more than a CU's LDS", p);
        if (p.bytes() > worst) worst = p.bytes();
        /* over 64 KB: the run-time loop's epoch alone from 43 anchors, with a 36-per-lane park behind it from 31, with
         * the 9-state park from 17 -- and nothing else */
        const bool loop_form = x.epoch == (size_t)192 * A;
        const int first_over = x.park == 5016 ? 17 : (x.park == 2304 ? 31 : 43);
        if ((p.bytes() > 64 * 1024) != (loop_form && A >= first_over)) return fail(in, what, "the set of plans over 64 KB", p);
        if (loop_form && A + 1 == first_over && p.bytes() != (x.park == 5016 ? 64704u : 64512u)) return fail(in, what, "last count under 64 KB", p);
        if (loop_form && A == first_over && p.bytes() != (x.park == 5016 ? 66240u : 66048u)) return fail(in, what, "first count over 64 KB", p);
        /* the rules in words */
        if (in.coop && (p.bytes() != 0 || p.tags_per_group != 8)) return fail(in, what, "coop: no LDS, 8 tags per group", p);
        if (what == STEP_SENSOR && p.as != 0) return fail(in, what, "a sensor call has as = 0", p);
        if (p.as == -16 && !toa) return fail(in, what, "-16 exists for the 6-state filter only", p);
        if (p.two_waves && !(toa && A == 8 && !in.full && !in.ignore_worst && !in.top_n && !in.force_generic && !in.coop && what == STEP_RANGING))
            return fail(in, what, "two-waves is the plain 8-anchor symmetric bank's", p);
        const bool no_epoch = what == STEP_IMU_ONLY || what == STEP_SENSOR;
        if (in.force_generic && (p.as != 0 || p.epoch_doubles != (no_epoch ? 0 : (size_t)192 * A)))
            return fail(in, what, "force_generic is the run-time form wherever there is an epoch", p);
    }
    if (worst != 138432) { /* 9-state at 64 anchors */
        std::printf("FAIL the largest plan takes %zu bytes\n", worst);
        return 1;
    }
    std::printf("OK %ld\n", ran);
    return 0;
}
