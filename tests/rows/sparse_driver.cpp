/*
 * sparse_driver.cpp -- BatchedRangingNode::setSparseRounds (kfpos_ingest.h): one seeded message stream feeds a node
 * that assembles whole-bank rounds and a node that assembles row-list rounds, each on a handle of its own. After every
 * poll() the two banks must hold the same bytes (kfpos_get_state + flags, kfpos_get_latch, kfpos_get_height) and have
 * made the same number of estimator calls; at the end the status words delivered for every call must be the same
 * sequence of (row, kind, status).
 *
 * The stream: tags report asynchronously (each with a period of 1-3 epochs and seeded drop-outs, some first heard late);
 * a tag whose next sequence number comes more than 50 ms after its last message is flushed by its timer AND by the new
 * sequence number (the reference's double flush); poll() is left out in some epochs, so that a tag's second epoch meets
 * a round that already holds its first and waits in the overflow arena; the 9-state bank gets IMU samples and the planar
 * bank all four sensors for seeded subsets of the tags, in between the ranging messages.
 *
 *   sparse_driver toa6 | imu9 | planar  [seed]      prints OK on success
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <tuple>
#include <vector>

#include "kfpos_ingest.h"

using kfpos_host::BatchedRangingNode;

static int failures = 0;
#define EXPECT(cond, ...)                          \
    do {                                           \
        if (!(cond)) {                             \
            if (++failures <= 20) {                \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);          \
                std::printf("\n");                 \
            }                                      \
        }                                          \
    } while (0)

static void chk(int rc, const char *what) {
    if (rc != KFPOS_OK) {
        std::printf("FAIL %s: %s %s\n", what, kfpos_strerror(rc), kfpos_last_error());
        std::exit(2);
    }
}

/* SplitMix64: the stream is a pure function of the seed */
struct Rng {
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double uni() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
};

struct Snapshot {
    std::vector<double> x, P, latch, height;
    std::vector<uint32_t> flags;
};
static Snapshot snapshot(kfpos_handle *h, int T) {
    Snapshot s;
    const int n = kfpos_state_dim(h), L = kfpos_latch_dim(h);
    s.x.resize((size_t)T * n);
    s.P.resize((size_t)T * n * n);
    s.flags.resize(T);
    chk(kfpos_get_state(h, s.x.data(), s.P.data(), s.flags.data()), "kfpos_get_state");
    s.latch.resize((size_t)T * L);
    if (L) chk(kfpos_get_latch(h, s.latch.data()), "kfpos_get_latch");
    if (n == 8) {
        s.height.resize(T);
        chk(kfpos_get_height(h, s.height.data()), "kfpos_get_height");
    }
    return s;
}
template <typename V>
static bool same_bytes(const V &a, const V &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

static int run(int model, unsigned seed) {
    constexpr int kTags = 150, kAnchors = 8, kEpochs = 60; /* 1200 range elements: the small bank's mapped block serves
                                                               the synchronous sensor calls, the slots are staged */
    double anchors[kAnchors * 3];
    std::vector<int> anchorIds, tagIds;
    for (int a = 0; a < kAnchors; ++a) {
        anchors[3 * a + 0] = 10.0 * (a & 1);
        anchors[3 * a + 1] = 10.0 * ((a >> 1) & 1);
        anchors[3 * a + 2] = 0.3 + 2.7 * ((a >> 2) & 1);
        anchorIds.push_back(100 + a);
    }
    for (int t = 0; t < kTags; ++t) tagIds.push_back(0x1000 + 3 * t);
    auto make = [&]() {
        kfpos_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.model = model;
        cfg.n_tags = kTags;
        cfg.max_anchors = kAnchors;
        cfg.storage = model == KFPOS_MODEL_TOA_IMU ? KFPOS_STORE_MIXED : KFPOS_STORE_F64;
        cfg.accel_noise = 0.5;
        cfg.jolt = 0.5;
        cfg.cost_threshold = 0.5;
        cfg.use_init_pos = 1;
        cfg.init_pos[0] = 5.0;
        cfg.init_pos[1] = 5.0;
        cfg.init_pos[2] = 1.0;
        kfpos_handle *h = nullptr;
        chk(kfpos_create(&cfg, &h), "kfpos_create");
        chk(kfpos_set_anchors(h, anchors, anchorIds.data(), kAnchors), "kfpos_set_anchors");
        if (model == KFPOS_MODEL_PLANAR) {
            kfpos_planar_config pc;
            std::memset(&pc, 0, sizeof(pc));
            pc.use_fixed_height = 1;
            pc.fixed_height = 1.0;
            pc.init_angle = 0.3;
            pc.px4_height = 1.0;
            pc.px4_arm_p1 = 0.05;
            pc.px4_arm_p2 = -0.02;
            pc.px4_cov_velocity = 0.002;
            pc.px4_cov_gyro_z = 0.001;
            pc.imu_cov_acc = 0.02;
            pc.imu_use_fixed_cov_ang_vel_z = 1;
            pc.imu_cov_ang_vel_z = 0.0005;
            pc.mag_angle_offset = 0.1;
            pc.mag_cov = 0.01;
            chk(kfpos_set_planar(h, &pc), "kfpos_set_planar");
        }
        return h;
    };
    kfpos_handle *hd = make(), *hs = make();
    BatchedRangingNode dense(hd, tagIds, anchorIds), sparse(hs, tagIds, anchorIds);
    sparse.setSparseRounds(true);
    EXPECT(!dense.sparseRounds() && sparse.sparseRounds(), "setSparseRounds");
    typedef std::tuple<int, int, uint32_t> Word;
    std::vector<Word> wd, ws;
    dense.setStatusSink([&](int row, int kind, uint32_t st) { wd.emplace_back(row, kind, st); });
    sparse.setStatusSink([&](int row, int kind, uint32_t st) { ws.emplace_back(row, kind, st); });

    auto range_mm = [&](int t, int a, int k) {
        const double ang = 0.02 * k + 0.01 * t, rho = 1.0 + (t & 3);
        const double p[3] = {5.0 + rho * std::cos(ang), 5.0 + rho * std::sin(ang), 1.0};
        double d2 = 0.0;
        for (int c = 0; c < 3; ++c) d2 += (p[c] - anchors[3 * a + c]) * (p[c] - anchors[3 * a + c]);
        return std::sqrt(d2) * 1000.0 + 30.0 * std::sin(12.9898 * (t + 1) + 78.233 * (a + 1) + 3.7 * k);
    };
    Rng rng{seed * 0x1234567ull + 99};
    long reports = 0, calls_d = 0, calls_s = 0;
    for (int k = 0; k < kEpochs; ++k) {
        const double t0 = 10.0 + 0.05 * k;
        for (int t = 0; t < kTags; ++t) {
            const int period = 1 + t % 3, first = (t % 7 == 3) ? 20 : 0; /* some tags are first heard at epoch 20 */
            const bool speaks = k >= first && k % period == 0 && rng.uni() > 0.1;
            const int id = tagIds[t];
            const double tt = t0 + 0.00002 * t;
            if (model != KFPOS_MODEL_TOA && rng.uni() < 0.4) { /* a sensor sample in front of the ranging messages */
                const double w[3] = {0.01 * std::sin(0.1 * k + t), 0.0, 0.02 * std::cos(0.07 * k)};
                const double acc[3] = {0.1 * std::sin(0.3 * k + t), 0.1 * std::cos(0.2 * k + t), 0.01};
                const double cw[9] = {1e-4, 0, 0, 0, 1e-4, 0, 0, 0, 1e-4};
                const double ca[9] = {0.01, 0.002, 0, 0.002, 0.01, 0, 0, 0, 0.01};
                const int which = model == KFPOS_MODEL_PLANAR ? (int)(rng.next() % 4) : 0;
                for (BatchedRangingNode *n : {&dense, &sparse}) {
                    if (which == 0) n->onImu(tt, id, w, cw, acc, ca);
                    else if (which == 1) n->onPX4Flow(tt, id, 0.001 * std::sin(0.1 * k), 0.001 * std::cos(0.1 * k), 0.0005, 10000.0, (k + t) % 5 == 0 ? 0 : 200);
                    else if (which == 2) n->onCompass(tt, id, 0.3 + 0.01 * k);
                    else {
                        const double f[3] = {std::cos(0.3 + 0.01 * k), std::sin(0.3 + 0.01 * k), 0.1};
                        n->onMag(tt, id, f);
                    }
                }
            }
            if (!speaks) continue;
            ++reports;
            for (int a = 0; a < kAnchors; ++a) {
                if (rng.uni() < 0.05) continue; /* a lost ranging */
                const double r = range_mm(t, a, k), e = 0.0025 * (1 + (a & 1));
                dense.onRanging(tt + 0.0007 * a, 100 + a, id, r, e, k & 0xff);
                sparse.onRanging(tt + 0.0007 * a, 100 + a, id, r, e, k & 0xff);
            }
        }
        if (k % 4 == 1) continue; /* no poll in this epoch: the next epoch's flushes meet a round that is still open */
        const double now = t0 + 0.045;
        const int cd = dense.poll(now), cs = sparse.poll(now);
        calls_d += cd;
        calls_s += cs;
        EXPECT(cd == cs, "epoch %d: poll() made %d estimator calls in whole-bank mode, %d in sparse mode", k, cd, cs);
        const Snapshot a = snapshot(hd, kTags), b = snapshot(hs, kTags);
        EXPECT(same_bytes(a.x, b.x), "epoch %d: x differs", k);
        EXPECT(same_bytes(a.P, b.P), "epoch %d: P differs", k);
        EXPECT(same_bytes(a.flags, b.flags), "epoch %d: flags differ", k);
        EXPECT(same_bytes(a.latch, b.latch), "epoch %d: latches differ", k);
        EXPECT(same_bytes(a.height, b.height), "epoch %d: heights differ", k);
        for (int t = 0; t < kTags; ++t)
            EXPECT(dense.started(t) == sparse.started(t) && dense.sinceLastEstimate(t, now) == sparse.sinceLastEstimate(t, now),
                   "epoch %d: estimator clock of row %d", k, t);
    }
    dense.deliverStatuses();
    sparse.deliverStatuses();
    EXPECT(dense.overflowCalls() == sparse.overflowCalls() && dense.overflowCalls() > 0, "overflow calls: %llu vs %llu",
           (unsigned long long)dense.overflowCalls(), (unsigned long long)sparse.overflowCalls());
    /* sensor samples on a 6-state bank never reach the estimator; ranging epochs: double flushes make more calls than
     * there were reports */
    EXPECT(model != KFPOS_MODEL_TOA || calls_d > reports, "no double flush in the stream: %ld calls for %ld reports", calls_d, reports);
    EXPECT(calls_d == calls_s && (long)wd.size() == calls_d, "%ld / %ld calls, %zu status words", calls_d, calls_s, wd.size());
    EXPECT(wd.size() == ws.size(), "status words delivered: %zu vs %zu", wd.size(), ws.size());
    for (size_t i = 0; i < wd.size() && i < ws.size(); ++i)
        EXPECT(wd[i] == ws[i], "status word %zu: row %d kind %d %08x vs row %d kind %d %08x", i, std::get<0>(wd[i]),
               std::get<1>(wd[i]), std::get<2>(wd[i]), std::get<0>(ws[i]), std::get<1>(ws[i]), std::get<2>(ws[i]));
    long started = 0;
    for (int t = 0; t < kTags; ++t) started += dense.started(t);
    EXPECT(started == kTags, "%ld of %d tags ever reached the estimator", started, kTags);
    /* switching back is legal when nothing is pending, and the next round is a whole-bank one again */
    sparse.setSparseRounds(false);
    for (int t = 0; t < kTags; t += 2)
        for (int a = 0; a < kAnchors; ++a)
            for (BatchedRangingNode *n : {&dense, &sparse})
                n->onRanging(20.0 + 0.0007 * a, 100 + a, tagIds[t], range_mm(t, a, kEpochs), 0.0025, kEpochs & 0xff);
    EXPECT(dense.poll(20.06) == sparse.poll(20.06), "poll after switching back");
    {
        const Snapshot a = snapshot(hd, kTags), b = snapshot(hs, kTags);
        EXPECT(same_bytes(a.x, b.x) && same_bytes(a.P, b.P) && same_bytes(a.flags, b.flags), "after switching back");
    }
    std::printf("model %d: %ld reports, %ld estimator calls, %llu of them through the overflow arena, %zu status words\n", model,
                reports, calls_d, (unsigned long long)dense.overflowCalls(), wd.size());
    kfpos_destroy(hd);
    kfpos_destroy(hs);
    return failures;
}

int main(int argc, char **argv) {
    int bad = 1;
    try {
        const std::string what = argc >= 2 ? argv[1] : "";
        const unsigned seed = argc >= 3 ? (unsigned)std::atoi(argv[2]) : 1u;
        if (what == "toa6") bad = run(KFPOS_MODEL_TOA, seed);
        else if (what == "imu9") bad = run(KFPOS_MODEL_TOA_IMU, seed);
        else if (what == "planar") bad = run(KFPOS_MODEL_PLANAR, seed);
        else std::printf("usage: sparse_driver toa6 | imu9 | planar [seed]\n");
    } catch (const std::exception &e) {
        std::printf("FAIL exception: %s\n", e.what());
        bad = 1;
    }
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
