/*
 * ingest_d16_driver.cpp -- BatchedRangingNode::setDeltaRanges (kfpos_ingest.h): one seeded message stream feeds a node
 * whose whole-bank ranging rounds carry int32 ranges and a node whose rounds carry int16 codes (KFPOS_SLOT_RANGES_D16),
 * each on a handle of its own. After every poll() the two banks must hold the same bytes (kfpos_get_state + flags) and
 * have made the same number of estimator calls; at the end the status words delivered for every call must be the same
 * sequence of (row, kind, status).
 *
 * The stream: tags report asynchronously (periods of 1-3 epochs, seeded drop-outs, lost rangings), one tag stays silent
 * for twenty epochs and comes back (its base is where it left it), some ranges jump by 40 m for one epoch (escapes up
 * and back down), poll() is left out in some epochs (overflow rounds), the 9-state bank gets IMU samples in between. A
 * third of the rows is free at first and admitted with bindRows in the middle; a few rows are released and bound to new
 * tag ids (a row's base then belongs to the tag before: only a longer escape list, never another result).
 *
 *   ingest_d16_driver toa6 | imu9  [seed]      prints OK on success
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
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        if (!(cond)) {                                           \
            if (++failures <= 20) {                              \
                std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
                std::printf(__VA_ARGS__);                        \
                std::printf("\n");                               \
            }                                                    \
        }                                                        \
    } while (0)

static void chk(int rc, const char *what) {
    if (rc != KFPOS_OK) {
        std::printf("FAIL %s: %s %s\n", what, kfpos_strerror(rc), kfpos_last_error());
        std::exit(2);
    }
}

struct Rng { /* SplitMix64 */
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
    std::vector<double> x, P;
    std::vector<uint32_t> flags;
};
static Snapshot snapshot(kfpos_handle *h, int T) {
    Snapshot s;
    const int n = kfpos_state_dim(h);
    s.x.resize((size_t)T * n);
    s.P.resize((size_t)T * n * n);
    s.flags.resize(T);
    chk(kfpos_get_state(h, s.x.data(), s.P.data(), s.flags.data()), "kfpos_get_state");
    return s;
}
template <typename V>
static bool same_bytes(const V &a, const V &b) {
    return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) == 0);
}

static int run(int model, unsigned seed) {
    constexpr int kTags = 150, kAnchors = 8, kEpochs = 60, kFirst = 100, kAdmit = 26, kSilent = 5;
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
        return h;
    };
    kfpos_handle *hp = make(), *hd = make();
    BatchedRangingNode plain(hp, kTags, anchorIds), delta(hd, kTags, anchorIds);
    delta.setDeltaRanges(true);
    EXPECT(!plain.deltaRanges() && delta.deltaRanges(), "setDeltaRanges");
    BatchedRangingNode *const both[2] = {&plain, &delta};
    typedef std::tuple<int, int, uint32_t> Word;
    std::vector<Word> wp, wd;
    plain.setStatusSink([&](int row, int kind, uint32_t st) { wp.emplace_back(row, kind, st); });
    delta.setStatusSink([&](int row, int kind, uint32_t st) { wd.emplace_back(row, kind, st); });
    {
        std::vector<int> rows;
        for (int t = 0; t < kFirst; ++t) rows.push_back(t);
        for (BatchedRangingNode *n : both) n->bindRows(rows.data(), tagIds.data(), kFirst, nullptr);
    }

    auto range_mm = [&](int t, int a, int k) {
        const double ang = 0.02 * k + 0.01 * t, rho = 1.0 + (t & 3);
        const double p[3] = {5.0 + rho * std::cos(ang), 5.0 + rho * std::sin(ang), 1.0};
        double d2 = 0.0;
        for (int c = 0; c < 3; ++c) d2 += (p[c] - anchors[3 * a + c]) * (p[c] - anchors[3 * a + c]);
        const double jump = (5 * t + 3 * a + k) % 89 == 0 ? 40000.0 : 0.0; /* an NLOS excursion of one epoch */
        return std::sqrt(d2) * 1000.0 + 30.0 * std::sin(12.9898 * (t + 1) + 78.233 * (a + 1) + 3.7 * k) + jump;
    };
    Rng rng{seed * 0x7654321ull + 17};
    long reports = 0, calls_p = 0, calls_d = 0, silent_epochs = 0;
    int bound = kFirst;
    for (int k = 0; k < kEpochs; ++k) {
        const double t0 = 10.0 + 0.05 * k;
        for (int t = 0; t < bound; ++t) {
            const int period = 1 + t % 3;
            bool speaks = k % period == 0 && rng.uni() > 0.1;
            if (t == kSilent && k >= 10 && k < 30) { /* silent for twenty epochs */
                silent_epochs += speaks;
                speaks = false;
            }
            const int id = tagIds[t];
            const double tt = t0 + 0.00002 * t;
            if (model == KFPOS_MODEL_TOA_IMU && rng.uni() < 0.4) {
                const double w[3] = {0.01 * std::sin(0.1 * k + t), 0.0, 0.02 * std::cos(0.07 * k)};
                const double acc[3] = {0.1 * std::sin(0.3 * k + t), 0.1 * std::cos(0.2 * k + t), 0.01};
                const double cw[9] = {1e-4, 0, 0, 0, 1e-4, 0, 0, 0, 1e-4};
                const double ca[9] = {0.01, 0.002, 0, 0.002, 0.01, 0, 0, 0, 0.01};
                for (BatchedRangingNode *n : both) n->onImu(tt, id, w, cw, acc, ca);
            }
            if (!speaks) continue;
            ++reports;
            for (int a = 0; a < kAnchors; ++a) {
                if (rng.uni() < 0.05) continue; /* a lost ranging */
                const double r = range_mm(t, a, k), e = 0.0025 * (1 + (a & 1));
                for (BatchedRangingNode *n : both) n->onRanging(tt + 0.0007 * a, 100 + a, id, r, e, k & 0xff);
            }
        }
        if (k % 4 == 1) continue; /* no poll in this epoch: the next epoch's flushes meet a round that is still open */
        const double now = t0 + 0.045;
        const int cp = plain.poll(now), cd = delta.poll(now);
        calls_p += cp;
        calls_d += cd;
        EXPECT(cp == cd, "epoch %d: poll() made %d estimator calls with int32 ranges, %d with codes", k, cp, cd);
        const Snapshot a = snapshot(hp, kTags), b = snapshot(hd, kTags);
        EXPECT(same_bytes(a.x, b.x), "epoch %d: x differs", k);
        EXPECT(same_bytes(a.P, b.P), "epoch %d: P differs", k);
        EXPECT(same_bytes(a.flags, b.flags), "epoch %d: flags differ", k);
        if (k == kAdmit) { /* right after poll(): the free rows are admitted, a few bound rows change hands */
            std::vector<int> rows, ids;
            for (int t = kFirst; t < kTags; ++t) {
                rows.push_back(t);
                ids.push_back(tagIds[t]);
            }
            const int swap[3] = {7, 40, 93};
            for (int r : swap) {
                tagIds[r] += 0x100000; /* the row's next tag */
                rows.push_back(r);
                ids.push_back(tagIds[r]);
            }
            for (BatchedRangingNode *n : both) {
                n->releaseRows(swap, 3);
                n->bindRows(rows.data(), ids.data(), (int)rows.size(), nullptr);
            }
            bound = kTags;
        }
    }
    plain.deliverStatuses();
    delta.deliverStatuses();
    EXPECT(silent_epochs > 0, "the silent tag would not have spoken anyway");
    EXPECT(plain.overflowCalls() == delta.overflowCalls() && plain.overflowCalls() > 0, "overflow calls: %llu vs %llu",
           (unsigned long long)plain.overflowCalls(), (unsigned long long)delta.overflowCalls());
    EXPECT(calls_p == calls_d && (long)wp.size() == calls_p, "%ld / %ld calls, %zu status words", calls_p, calls_d, wp.size());
    EXPECT(wp.size() == wd.size(), "status words delivered: %zu vs %zu", wp.size(), wd.size());
    for (size_t i = 0; i < wp.size() && i < wd.size(); ++i)
        EXPECT(wp[i] == wd[i], "status word %zu: row %d kind %d %08x vs row %d kind %d %08x", i, std::get<0>(wp[i]),
               std::get<1>(wp[i]), std::get<2>(wp[i]), std::get<0>(wd[i]), std::get<1>(wd[i]), std::get<2>(wd[i]));
    /* sparse rounds ignore the switch; switching either off is legal when nothing is pending */
    delta.setSparseRounds(true);
    for (int round = 0; round < 2; ++round) {
        for (int t = 0; t < kTags; t += 2)
            for (int a = 0; a < kAnchors; ++a)
                for (BatchedRangingNode *n : both)
                    n->onRanging(20.0 + round + 0.0007 * a, 100 + a, tagIds[t], range_mm(t, a, kEpochs + round), 0.0025, (kEpochs + round) & 0xff);
        EXPECT(plain.poll(20.06 + round) == delta.poll(20.06 + round), "poll after switching");
        const Snapshot a = snapshot(hp, kTags), b = snapshot(hd, kTags);
        EXPECT(same_bytes(a.x, b.x) && same_bytes(a.P, b.P) && same_bytes(a.flags, b.flags), "after switching, round %d", round);
        delta.setSparseRounds(false);
        delta.setDeltaRanges(round == 0); /* a D16 round once more, then plain */
    }
    std::printf("model %d: %ld reports, %ld estimator calls, %llu of them through the overflow arena, %zu status words\n", model,
                reports, calls_p, (unsigned long long)plain.overflowCalls(), wp.size());
    kfpos_destroy(hp);
    kfpos_destroy(hd);
    return failures;
}

int main(int argc, char **argv) {
    int bad = 1;
    try {
        const std::string what = argc >= 2 ? argv[1] : "";
        const unsigned seed = argc >= 3 ? (unsigned)std::atoi(argv[2]) : 1u;
        if (what == "toa6") bad = run(KFPOS_MODEL_TOA, seed);
        else if (what == "imu9") bad = run(KFPOS_MODEL_TOA_IMU, seed);
        else std::printf("usage: ingest_d16_driver toa6 | imu9 [seed]\n");
    } catch (const std::exception &e) {
        std::printf("FAIL exception: %s\n", e.what());
        bad = 1;
    }
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
