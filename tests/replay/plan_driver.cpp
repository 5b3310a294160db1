// Stand-alone checks of roskfpos_amd/csrc/kfpos_replay_plan.h: the two wire formats of `kinds` and the cut of a schedule
// into launches. No GPU, no library: tests/test_replay_plan.py builds this file with g++ and the sanitizers and runs it.
//   plan_driver                                 every check below; prints OK, exit status 0
//   plan_driver starts CHUNK N_KINDS DIGITS     the first event of every launch for the schedule DIGITS (one kind per
//                                               character), its leading ranging events taken by the ranging path
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "kfpos_replay_plan.h"

namespace {

int fails = 0;
#define CHECK(cond, ...)                                     \
    do {                                                     \
        if (!(cond)) {                                       \
            if (++fails <= 20) {                             \
                std::printf("FAILED %s: ", #cond);           \
                std::printf(__VA_ARGS__);                    \
                std::printf("\n");                           \
            }                                                \
        }                                                    \
    } while (0)

int ranging_kind(int n_kinds) { return n_kinds == 2 ? 1 : 0; }   // KFPOS_EVENT_TOA, KFPOS_PLANAR_EVENT_TOA

// events ahead of the first one that is no ranging: what the shared-timeline entry points send down the ranging path
int lead_of(const std::vector<uint8_t> &kinds, int n_kinds) {
    int lead = 0;
    while (lead < (int)kinds.size() && kinds[lead] == ranging_kind(n_kinds)) ++lead;
    return lead;
}

// ahead[e * n_kinds + k]: events of kind k in kinds[0..e), counted one by one
std::vector<size_t> count_ahead(const std::vector<uint8_t> &kinds, int n_kinds) {
    std::vector<size_t> ahead((kinds.size() + 1) * n_kinds, 0);
    for (size_t e = 0; e < kinds.size(); ++e)
        for (int k = 0; k < n_kinds; ++k) ahead[(e + 1) * n_kinds + k] = ahead[e * n_kinds + k] + (kinds[e] == k ? 1 : 0);
    return ahead;
}

void check_cut(const std::vector<uint8_t> &kinds, const std::vector<size_t> &ahead, int first, int chunk, int n_kinds, const char *what) {
    const int n_events = (int)kinds.size();
    size_t brute[KFPOS_PLAN_MAX_KINDS];
    // the vector's own buffer, exactly n_events long: AddressSanitizer sees a read past the schedule
    int expect = first, launches = 0;
    for (kfpos_replay_cut c(kinds.data(), n_events, first, chunk, n_kinds); c.next();) {
        ++launches;
        CHECK(c.e0 == expect, "%s n=%d chunk=%d kinds=%d first=%d: launch at %d, expected %d", what, n_events, chunk, n_kinds, first, c.e0, expect);
        CHECK(c.n >= 1 && c.n <= chunk && c.e0 + c.n <= n_events, "%s n=%d chunk=%d: launch of %d events at %d", what, n_events, chunk, c.n, c.e0);
        CHECK(c.last() == (c.e0 + c.n == n_events), "%s n=%d chunk=%d: last() at %d", what, n_events, chunk, c.e0);
        for (int k = 0; k < n_kinds; ++k) brute[k] = ahead[(size_t)c.e0 * n_kinds + k] - ahead[(size_t)first * n_kinds + k];
        brute[ranging_kind(n_kinds)] += (size_t)first;   // the lead: one ranging input each
        for (int k = 0; k < n_kinds; ++k)
            CHECK(c.ord[k] == brute[k], "%s n=%d chunk=%d first=%d: ord[%d] = %zu at %d, counted %zu", what, n_events, chunk, first, k, c.ord[k], c.e0, brute[k]);
        if (c.n < 1) return;   // no progress: reported above
        expect = c.e0 + c.n;
    }
    CHECK(expect == (first < n_events ? n_events : first), "%s n=%d chunk=%d first=%d: the launches end at %d", what, n_events, chunk, first, expect);
    CHECK(launches == (n_events > first ? (n_events - first + chunk - 1) / chunk : 0), "%s n=%d chunk=%d first=%d: %d launches", what, n_events, chunk, first, launches);
}

void cut_checks() {
    std::mt19937 rng(20261019);
    const int chunks[] = {1, 7, 64, 127, 128};
    for (int n_kinds : {2, 5}) {
        const uint8_t toa = (uint8_t)ranging_kind(n_kinds), other = toa ? 0 : 2;
        for (int n = 0; n <= 300; ++n) {
            std::vector<std::pair<const char *, std::vector<uint8_t>>> cases;
            cases.push_back({"all ranging", std::vector<uint8_t>(n, toa)});
            cases.push_back({"no ranging", std::vector<uint8_t>(n, other)});
            for (int at : {0, 1, n - 1}) {   // the first event that is no ranging
                if (at < 0 || at >= n) continue;
                std::vector<uint8_t> k(n, toa);
                k[at] = other;
                for (int e = at + 1; e < n; ++e) k[e] = (uint8_t)(rng() % n_kinds);
                cases.push_back({at == 0 ? "first other event at 0" : at == 1 ? "first other event at 1" : "first other event last", k});
            }
            for (int seed = 0; seed < 3; ++seed) {
                std::vector<uint8_t> k(n);
                for (auto &v : k) v = (uint8_t)(rng() % n_kinds);
                cases.push_back({"seeded", k});
            }
            for (const auto &c : cases) {
                const std::vector<size_t> ahead = count_ahead(c.second, n_kinds);
                for (int chunk : chunks) {
                    check_cut(c.second, ahead, lead_of(c.second, n_kinds), chunk, n_kinds, c.first);   // the shared-timeline forms
                    check_cut(c.second, ahead, 0, chunk, n_kinds, c.first);                            // the per-tag forms
                }
            }
        }
    }
    // the 6-state per-tag form: no kinds, nothing to count
    for (int n = 0; n <= 300; ++n)
        for (int chunk : chunks) {
            int expect = 0;
            for (kfpos_replay_cut c(nullptr, n, 0, chunk, 0); c.next(); expect = c.e0 + c.n)
                CHECK(c.e0 == expect && c.n >= 1 && c.n <= chunk, "no kinds n=%d chunk=%d: launch of %d at %d", n, chunk, c.n, c.e0);
            CHECK(expect == n, "no kinds n=%d chunk=%d: the launches end at %d", n, chunk, expect);
        }
}

void format_checks() {
    std::mt19937 rng(7);
    for (int n = 1; n <= KFPOS_PLAN_MAX_EVENTS; ++n)
        for (int rep = 0; rep < 4; ++rep) {
            std::vector<uint8_t> k1(n), k4(n);   // exactly n long: a packer that reads further is caught
            for (int e = 0; e < n; ++e) {
                k1[e] = rep == 0 ? 1 : (uint8_t)(rng() % 2);
                k4[e] = rep == 0 ? 4 : (uint8_t)(rng() % 5);
            }
            unsigned long long w1[KFPOS_KINDS1_WORDS];
            uint32_t w4[KFPOS_KINDS4_WORDS];
            std::memset(w1, 0xFF, sizeof(w1));   // the packers clear what they do not set
            std::memset(w4, 0xFF, sizeof(w4));
            kfpos_kinds1_pack(w1, k1.data(), n);
            kfpos_kinds4_pack(w4, k4.data(), n);
            for (int e = 0; e < KFPOS_PLAN_MAX_EVENTS; ++e) {
                const unsigned bit = (unsigned)((w1[e / 64] >> (e % 64)) & 1ull), nibble = (w4[e / 8] >> ((e % 8) * 4)) & 0xFu;
                if (e < n) {
                    CHECK(kfpos_kinds1_at(w1, e) == k1[e], "1-bit n=%d: event %d decodes to %d, packed %d", n, e, kfpos_kinds1_at(w1, e), k1[e]);
                    CHECK(kfpos_kinds4_at(w4, e) == k4[e], "4-bit n=%d: event %d decodes to %d, packed %d", n, e, kfpos_kinds4_at(w4, e), k4[e]);
                    CHECK(nibble == k4[e], "4-bit n=%d: nibble %d holds %u, packed %d", n, e, nibble, k4[e]);
                } else {
                    CHECK(bit == 0, "1-bit n=%d: bit %d is set", n, e);
                    CHECK(nibble == 0, "4-bit n=%d: nibble %d holds %u", n, e, nibble);
                }
            }
        }
}

}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "starts")) {
        const int chunk = std::atoi(argv[2]), n_kinds = std::atoi(argv[3]);
        std::vector<uint8_t> kinds;
        for (const char *p = argv[4]; *p; ++p) kinds.push_back((uint8_t)(*p - '0'));
        for (kfpos_replay_cut c(kinds.data(), (int)kinds.size(), lead_of(kinds, n_kinds), chunk, n_kinds); c.next();)
            std::printf("%d\n", c.e0);
        return 0;
    }
    if (argc != 1) {
        std::printf("usage: plan_driver | plan_driver starts CHUNK N_KINDS DIGITS\n");
        return 1;
    }
    cut_checks();
    format_checks();
    if (fails) {
        std::printf("%d checks failed\n", fails);
        return 2;
    }
    std::printf("OK\n");
    return 0;
}
