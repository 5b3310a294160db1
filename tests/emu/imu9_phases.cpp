/*
 * imu9_phases.cpp -- TEST INFRASTRUCTURE ONLY (tests/test_imu9_phases_emu.py builds and runs it with g++).
 *
 * kfpos_core_imu9.h has the 9-state step twice: step_imu9_state, whose covariance travels in registers, and the phase
 * functions step_imu9_head + step_imu9_state_parked, whose covariance lives in the park between two epochs (the epoch
 * loop of k_step_imu9). Both are made of the same statements, and nothing but this program ties the two texts together:
 * it runs one tag through a sequence of epochs both ways and compares position, velocity, covariance and status word
 * of every epoch as bytes, over every way a step can end -- ML initialisation, fewer than four ranges (waiting and
 * started), update skipped, the (I + M B) form, the information form -- with and without an accelerometer sample, in
 * the fast and in the per-lane form of the pass. Exit status 0: the same bytes everywhere, and every way was taken.
 */
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../roskfpos_amd/csrc/kfpos_core.h"

using namespace kfpos;

static const double ANCHORS[24] = {0, 0, 3, 10, 0, 3, 10, 8, 3, 0, 8, 3, 0, 0, 0.3, 10, 0, 0.2, 10, 8, 0.4, 0, 8, 0.1};

struct Case {
    const char *name;
    bool init;     /* fixed start (use_init_pos) or NaN start */
    bool has_imu, fast;
    int few_until; /* fewer than four ranges in epochs [0, few_until) */
    bool zero_err; /* errorEstimation 0: the update is skipped in every epoch */
    int epochs;
};

static void epoch_of(const Case &c, int e, RegScratch<8> &sc, double acc[3]) {
    const double p[3] = {3.0 + 0.11 * e, 2.5 + 0.07 * e, 1.2 + 0.01 * e};
    for (int a = 0; a < 8; ++a) {
        const double dx = p[0] - ANCHORS[3 * a], dy = p[1] - ANCHORS[3 * a + 1], dz = p[2] - ANCHORS[3 * a + 2];
        const int32_t mm = (int32_t)(1000.0 * std::sqrt(dx * dx + dy * dy + dz * dz)) + ((7 * e + 13 * a) % 41) - 20;
        const bool absent = (e < c.few_until && a >= 3) || (e == 5 && a == 1);
        sc.r[a] = absent ? 0.0 : kf_mm_to_m(mm);
        sc.e[a] = c.zero_err ? 0.0 : (double)(float)(0.05 + 0.01 * ((a + e) % 3));
        sc.w[a] = 0.0;
    }
    acc[0] = 0.02 * ((e % 5) - 2); acc[1] = -0.015 * ((e % 3) - 1); acc[2] = 0.01 * (e % 2);
}

static bool same(const Tag9 &a, const Tag9 &b) {
    return !std::memcmp(a.pos, b.pos, sizeof a.pos) && !std::memcmp(a.vel, b.vel, sizeof a.vel) &&
           !std::memcmp(a.P.a, b.P.a, sizeof a.P.a);
}

int main() {
    const Case cases[] = {
        {"fixed start, sample, per-lane form", true, true, false, 0, false, 14},
        {"fixed start, sample, fast form", true, true, true, 0, false, 14},
        {"fixed start, no sample", true, false, false, 0, false, 14},
        {"fixed start, few ranges while started", true, true, true, 2, false, 10},
        {"NaN start, initialises in epoch 3", false, true, true, 3, false, 12},
        {"NaN start, never starts", false, true, false, 99, false, 6},
        {"errorEstimation 0: update skipped", true, true, true, 0, true, 6},
    };
    unsigned seen = 0; /* 1 ML init, 2 few ranges while waiting, 4 update skipped, 8 (I + M B) form, 16 information form,
                          32 few ranges while started */
    int bad = 0;
    for (const Case &c : cases) {
        Params pr;
        pr.anchors = ANCHORS;
        pr.n_anchors = 8;
        pr.accel_noise = 0.5; pr.jolt = 0.5; pr.cost_threshold = 0.5;
        pr.ignore_worst = 0; pr.top_n = 0; pr.use_init_pos = c.init ? 1 : 0;
        Tag9 ta, tb;
        std::memset(&ta, 0, sizeof ta);
        for (int k = 0; k < 3; ++k) ta.pos[k] = c.init ? (k == 0 ? 3.0 : k == 1 ? 2.5 : 1.2) : NAN;
        tb = ta;
        double ci[12];
        Imu imu;
        imu.has = c.has_imu;
        imu.ci = ci;
        imu.ci_stride = 1;
        const double cov[9] = {0.04, 0, 0, 0, 0.05, 0, 0, 0, 0.06};
        imu_whitener(cov, imu.ci, imu.ci_stride);
        double park_a[66], park_b[66];
        const CovPark9 pa{park_a, 1}, pb{park_b, 1};
        auto dt_of = [](int e) { return 0.03 + 0.01 * (e % 5); };
        bool invertible = step_imu9_head(tb, pr, dt_of(0), pb); /* the prologue */
        for (int e = 0; e < c.epochs; ++e) {
            RegScratch<8> sa, sb;
            epoch_of(c, e, sa, imu.acc);
            sb = sa;
            const double dt = dt_of(e);
            const bool waiting = !imu9_started(ta, pr);
            Iekf9Out oa, ob;
            uint32_t st_a = 0, st_b = 0;
            if (step_imu9_state<true>(ta, sa, pr, dt, imu, pa, c.fast, oa, st_a)) st_a = step_imu9_cov(ta, oa, imu);
            if (step_imu9_state_parked<true>(tb, sb, pr, dt, imu, pb, c.fast, invertible, ob, st_b)) {
                st_b = step_imu9_cov(tb, ob, imu);
                seen |= invertible ? 16u : 8u;
            }
            const uint32_t fl = st_a & 0xFFu;
            if (fl & ST_ML_INIT) seen |= 1u;
            if ((fl & ST_FEW_RANGES) && waiting) seen |= 2u;
            if ((fl & ST_FEW_RANGES) && !waiting) seen |= 32u;
            if (fl & ST_UPDATE_SKIPPED) seen |= 4u;
            if (st_a != st_b || !same(ta, tb)) {
                std::printf("%s: epoch %d differs (status %08x / %08x)\n", c.name, e, st_a, st_b);
                ++bad;
                break;
            }
            if (e + 1 < c.epochs) invertible = step_imu9_head(tb, pr, dt_of(e + 1), pb);
        }
        if (!c.init && c.few_until < c.epochs && !std::isfinite(ta.pos[0])) {
            std::printf("%s: the tag never started\n", c.name);
            ++bad;
        }
    }
    if (seen != 63u) {
        std::printf("not every way through a step was taken: %02x of 3f\n", seen);
        ++bad;
    }
    std::printf("%s\n", bad ? "FAILED" : "the phase functions leave the same bytes as step_imu9_state");
    return bad ? 1 : 0;
}
