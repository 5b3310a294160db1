/*
 * lifecycle_driver.cpp -- test driver for the reusable rows of kfpos_ingest.h (tests/test_ingest_lifecycle.py builds it
 * against libkfpos_hip.so the way the csrc Makefile builds kfpos_replay).
 *
 *   lifecycle_driver idmap <seed>   FlatIdMap with erase against std::map (no GPU)
 *   lifecycle_driver node           BatchedRangingNode: release a row, bind another tag into it (GPU)
 *
 * Prints one line per finding and "OK" at the end; exit status 0 only if everything held.
 */
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "kfpos_ingest.h"

using kfpos_host::BatchedRangingNode;
using kfpos_host::FlatIdMap;

static int failures = 0;
#define EXPECT(cond, ...)                     \
    do {                                      \
        if (!(cond)) {                        \
            ++failures;                       \
            std::printf("FAIL %s: ", #cond);  \
            std::printf(__VA_ARGS__);         \
            std::printf("\n");                \
        }                                     \
    } while (0)

/* ------------------------------------------------------------------ FlatIdMap */
/* the map's hash, restated here only to PICK ids that share a home slot (capacity 256 for 64 reserved ids) */
static size_t home_slot(int id, size_t mask) { return ((uint64_t)(uint32_t)id * 0x9E3779B97F4A7C15ull >> 32) & mask; }

static int run_idmap(unsigned seed) {
    constexpr int kRows = 64;
    std::mt19937 rng(seed);
    /* the pool: scattered ids, negative ids, and a cluster of 24 ids that all hash to one slot */
    std::vector<int> pool;
    for (int i = 0; i < 120; ++i) pool.push_back((int)(rng() % 100000) - 20000);
    const size_t target = home_slot(pool[0], 255);
    for (int id = 1, found = 0; found < 24; ++id)
        if (home_slot(id * 7919, 255) == target) {
            pool.push_back(id * 7919);
            ++found;
        }
    FlatIdMap m;
    std::map<int, int> ref;
    m.reserve(kRows);
    auto compare = [&](const char *after, int step) {
        for (int id : pool) {
            const auto it = ref.find(id);
            const int want = it == ref.end() ? -1 : it->second;
            EXPECT(m.find(id) == want, "after %s (step %d): find(%d) = %d, std::map says %d", after, step, id, m.find(id), want);
        }
        EXPECT(m.size() == ref.size(), "after %s (step %d): size %zu vs %zu", after, step, m.size(), ref.size());
    };
    std::vector<int> erased;
    size_t limit = kRows;
    long probes = 0, lookups = 0;
    for (int step = 0; step < 6000 && failures == 0; ++step) {
        const unsigned op = rng() % 100;
        if (op < 2) { /* build: positions = indices, a repeated id keeps its last position */
            std::vector<int> ids;
            const int n = 1 + (int)(rng() % kRows);
            for (int i = 0; i < n; ++i) ids.push_back(pool[rng() % pool.size()]);
            m.build(ids); /* (sized for its own list: until the next build the sequence lives within n ids) */
            limit = (size_t)n;
            ref.clear();
            for (int i = 0; i < n; ++i) ref[ids[i]] = i;
            compare("build", step);
        } else if (op < 45) { /* insert: a new id, a present id (new value), or one erased earlier */
            int id = pool[rng() % pool.size()];
            if (!erased.empty() && rng() % 3 == 0) id = erased[rng() % erased.size()];
            if (ref.size() >= limit && !ref.count(id)) continue;
            const int v = (int)(rng() % kRows);
            m.insert(id, v);
            ref[id] = v;
            compare("insert", step);
        } else if (op < 85) { /* erase: mostly present ids, among them members of the colliding cluster */
            int id = pool[rng() % pool.size()];
            if (!ref.empty() && rng() % 4 != 0) {
                auto it = ref.begin();
                std::advance(it, rng() % ref.size());
                id = it->first;
            }
            const bool was = ref.erase(id) > 0;
            EXPECT(m.erase(id) == was, "erase(%d) at step %d", id, step);
            if (was) erased.push_back(id);
            compare("erase", step);
        } else {
            for (const auto &kv : ref) {
                probes += m.probes(kv.first);
                ++lookups;
            }
        }
    }
    /* fill the cluster completely, take out every other member, put them back: still exact */
    m.reserve(kRows);
    ref.clear();
    for (size_t i = 120; i < pool.size(); ++i) { m.insert(pool[i], (int)i); ref[pool[i]] = (int)i; }
    for (size_t i = 120; i < pool.size(); i += 2) { m.erase(pool[i]); ref.erase(pool[i]); }
    compare("cluster erase", -1);
    for (size_t i = 120; i < pool.size(); i += 2) { m.insert(pool[i], 7); ref[pool[i]] = 7; }
    compare("cluster re-insert", -1);
    /* no tombstones: after all that churn a lookup of a present id still takes about one probe outside the cluster */
    m.reserve(kRows);
    for (int i = 0; i < 60; ++i) m.insert(pool[i], i);
    for (int round = 0; round < 200; ++round)
        for (int i = 0; i < 60; i += 3) { m.erase(pool[i]); m.insert(pool[i], i); }
    long p2 = 0;
    for (int i = 0; i < 60; ++i) p2 += m.probes(pool[i]);
    EXPECT(p2 <= 60 * 2, "mean probes after churn %.2f", p2 / 60.0);
    std::printf("idmap: %ld lookups, %.3f probes each during the random sequence; %.3f after churn\n", lookups,
                lookups ? (double)probes / lookups : 0.0, p2 / 60.0);
    return failures;
}

/* ------------------------------------------------------------------ BatchedRangingNode */
static void chk(int rc, const char *what) {
    if (rc != KFPOS_OK) {
        std::printf("FAIL %s: %s %s\n", what, kfpos_strerror(rc), kfpos_last_error());
        std::exit(2);
    }
}

struct Pose {
    std::vector<double> pos, cov;
    std::vector<uint32_t> st;
};
static Pose poses(kfpos_handle *h, const BatchedRangingNode &node, double now) {
    const int T = node.rows();
    std::vector<double> dt(T);
    for (int r = 0; r < T; ++r) dt[r] = node.sinceLastEstimate(r, now);
    Pose p;
    p.pos.resize(3 * T);
    p.cov.resize(9 * T);
    p.st.resize(T);
    chk(kfpos_get_pose_each(h, dt.data(), p.pos.data(), p.cov.data(), nullptr, p.st.data()), "kfpos_get_pose_each");
    return p;
}
static bool same_row(const Pose &a, const Pose &b, int row) {
    return std::memcmp(&a.pos[3 * row], &b.pos[3 * row], 3 * sizeof(double)) == 0 &&
           std::memcmp(&a.cov[9 * row], &b.cov[9 * row], 9 * sizeof(double)) == 0 && a.st[row] == b.st[row];
}

static int run_node() {
    constexpr int kRows = 6, kAnchors = 8;
    const int A = 0xA1, B = 0xB2, C = 0xC3, D = 0xD4, E = 0xE5;
    double anchors[kAnchors * 3];
    std::vector<int> anchorIds;
    for (int a = 0; a < kAnchors; ++a) {
        anchors[3 * a + 0] = 10.0 * (a & 1);
        anchors[3 * a + 1] = 10.0 * ((a >> 1) & 1);
        anchors[3 * a + 2] = 0.3 + 2.7 * ((a >> 2) & 1);
        anchorIds.push_back(100 + a);
    }
    auto make = [&]() {
        kfpos_config cfg;
        std::memset(&cfg, 0, sizeof(cfg));
        cfg.model = KFPOS_MODEL_TOA;
        cfg.n_tags = kRows;
        cfg.max_anchors = kAnchors;
        cfg.storage = KFPOS_STORE_F64;
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
    /* a tag's range to an anchor at epoch k: a circle around the room's centre, a deterministic wobble as noise */
    auto range_mm = [&](int tag, int a, int k) {
        const double ang = 0.02 * k + 0.001 * tag, rho = 1.0 + (tag & 3);
        const double p[3] = {5.0 + rho * std::cos(ang), 5.0 + rho * std::sin(ang), 1.0 + 0.1 * std::sin(0.05 * k)};
        double d2 = 0.0;
        for (int c = 0; c < 3; ++c) d2 += (p[c] - anchors[3 * a + c]) * (p[c] - anchors[3 * a + c]);
        return std::sqrt(d2) * 1000.0 + 30.0 * std::sin(12.9898 * (tag + 1) + 78.233 * (a + 1) + 3.7 * k);
    };
    auto feed = [&](BatchedRangingNode &n, int tag, int k) {
        const double t0 = 10.0 + 0.05 * k;
        for (int a = 0; a < kAnchors; ++a)
            n.onRanging(t0 + 0.0007 * a + 0.00001 * (tag & 0xf), 100 + a, tag, range_mm(tag, a, k), 0.0025, k & 0xff);
    };

    kfpos_handle *h1 = make(), *h2 = make(), *h3 = make();
    const int rb = 2; /* the row that changes hands */
    /* node 1: six free rows, a-d admitted in one batch; node 3: the same, nothing is ever released */
    BatchedRangingNode n1(h1, kRows, anchorIds), n3(h3, kRows, anchorIds);
    const int rows4[4] = {0, rb, 4, 5}, ids4[4] = {A, B, C, D};
    n1.bindRows(rows4, ids4, 4, nullptr);
    n3.bindRows(rows4, ids4, 4, nullptr);
    EXPECT(n1.rowOf(B) == rb && n1.rowOf(E) == -1 && n1.rowOf(A) == 0 && !n1.bound(1) && n1.bound(rb), "rowOf after bindRows");
    /* node 2: a fresh handle, built with e in that row from the start; it only ever hears e */
    BatchedRangingNode n2(h2, std::vector<int>{-101, -102, E, -104, -105, -106}, anchorIds);

    int k = 0;
    for (; k < 40; ++k) {
        for (int tag : {A, B, C, D}) { feed(n1, tag, k); feed(n3, tag, k); }
        if (k == 20) { /* a flushed epoch is waiting for poll(): neither call is legal now */
            bool threw = false;
            try { n1.releaseRows(&rb, 1); } catch (const std::logic_error &) { threw = true; }
            EXPECT(threw, "releaseRows with a call pending did not throw std::logic_error");
            threw = false;
            const int r1 = 1;
            try { n1.bindRows(&r1, &E, 1, nullptr); } catch (const std::logic_error &) { threw = true; }
            EXPECT(threw, "bindRows with a call pending did not throw std::logic_error");
            EXPECT(n1.rowOf(B) == rb && n1.rowOf(E) == -1, "a refused call changed the map");
        }
        const double now = 10.0 + 0.05 * k + 0.04;
        n1.poll(now);
        n3.poll(now);
        const Pose p1 = poses(h1, n1, now), p3 = poses(h3, n3, now);
        for (int r : rows4) EXPECT(same_row(p1, p3, r), "epoch %d row %d: the twin nodes differ before any release", k, r);
    }
    /* right after poll(): b leaves, e takes its row */
    n1.releaseRows(&rb, 1);
    EXPECT(n1.rowOf(B) == -1 && !n1.bound(rb) && !n1.started(rb), "after releaseRows");
    {
        bool threw = false;
        try { n1.bindRows(&rb, &A, 1, nullptr); } catch (const std::logic_error &) { threw = true; } /* a is bound */
        EXPECT(threw, "bindRows of a bound id did not throw");
        threw = false;
        const int r0 = 0;
        try { n1.bindRows(&r0, &E, 1, nullptr); } catch (const std::logic_error &) { threw = true; } /* row 0 is taken */
        EXPECT(threw, "bindRows into a bound row did not throw");
    }
    n1.bindRows(&rb, &E, 1, nullptr);
    EXPECT(n1.rowOf(E) == rb && n1.rowOf(B) == -1 && n1.bound(rb), "after bindRows");
    {
        const Pose p1 = poses(h1, n1, 10.0 + 0.05 * 39 + 0.045), p2 = poses(h2, n2, 10.0 + 0.05 * 39 + 0.045);
        EXPECT(same_row(p1, p2, rb) && p1.st[rb] == KFPOS_ST_NOT_STARTED, "the re-bound row is not a fresh tag: status %08x", p1.st[rb]);
    }
    int started_at = -1;
    for (; k < 70; ++k) {
        for (int tag : {A, B, C, D}) feed(n3, tag, k);
        for (int tag : {A, B, C, D, E}) feed(n1, tag, k); /* b keeps talking: not one of ours any more */
        feed(n2, E, k);
        const double now = 10.0 + 0.05 * k + 0.04;
        n1.poll(now);
        n2.poll(now);
        n3.poll(now);
        const Pose p1 = poses(h1, n1, now), p2 = poses(h2, n2, now), p3 = poses(h3, n3, now);
        EXPECT(same_row(p1, p2, rb), "epoch %d: row %d (tag e) differs from the node that had e from the start: %.17g vs %.17g, status %08x vs %08x",
               k, rb, p1.pos[3 * rb], p2.pos[3 * rb], p1.st[rb], p2.st[rb]);
        for (int r : {0, 4, 5}) EXPECT(same_row(p1, p3, r), "epoch %d row %d differs from the run in which nothing was released", k, r);
        if (started_at < 0 && n1.started(rb)) started_at = k;
        EXPECT(n1.started(rb) == n2.started(rb), "epoch %d: estimator clocks of e differ", k);
    }
    EXPECT(started_at == 41, "e's first estimator call came at epoch %d, expected 41 (its second sequence number flushes the first)", started_at);
    {
        const Pose p1 = poses(h1, n1, 10.0 + 0.05 * 70);
        EXPECT(p1.st[rb] == 0 && std::isfinite(p1.pos[3 * rb]), "e is not tracked: status %08x", p1.st[rb]);
        EXPECT(p1.st[1] == KFPOS_ST_NOT_STARTED && p1.st[3] == KFPOS_ST_NOT_STARTED, "the rows that were never bound have started");
    }
    kfpos_destroy(h1);
    kfpos_destroy(h2);
    kfpos_destroy(h3);
    return failures;
}

int main(int argc, char **argv) {
    int bad = 1;
    try {
        if (argc >= 2 && std::string(argv[1]) == "idmap") bad = run_idmap(argc >= 3 ? (unsigned)std::atoi(argv[2]) : 1u);
        else if (argc >= 2 && std::string(argv[1]) == "node") bad = run_node();
        else std::printf("usage: lifecycle_driver idmap <seed> | node\n");
    } catch (const std::exception &e) {
        std::printf("FAIL exception: %s\n", e.what());
        bad = 1;
    }
    if (!bad) std::printf("OK\n");
    return bad ? 1 : 0;
}
