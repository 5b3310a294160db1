/* include/kfpos_d16.h (the D16 wire format: kfpos_d16_put, kfpos_d16_decode_ref) and kfpos_layout::delta_layout of
 * roskfpos_amd/csrc/kfpos_host_layout.h. tests/test_d16_codec.py builds this with g++ and the address and
 * undefined-behaviour sanitizers; no HIP header, no library.
 *
 *   d16_driver            the checks below; prints "OK <checks>" or the failures
 *   d16_driver IN OUT     encodes and decodes the rounds of file IN and writes what came out to OUT, for the numpy
 *                         restatement of the codec (tests/d16.py) to be compared with:
 *                         IN:  int32 A, T, R; per round int32 v [A][T], uint8 skip [T]
 *                         OUT: per round int16 code [A][T], int32 n_esc, int32 esc [n_esc][2], int32 out [A][T],
 *                              int32 base [A][T] (the decoder's)
 */
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "kfpos_d16.h"
#include "kfpos_host_layout.h"

static int failures = 0, checks = 0;
static std::string where;
#define CHECK(cond)                                                                                       \
    do {                                                                                                  \
        ++checks;                                                                                         \
        if (!(cond)) {                                                                                    \
            if (++failures <= 20) std::printf("FAIL %s: %s (line %d)\n", where.c_str(), #cond, __LINE__); \
        }                                                                                                 \
    } while (0)

/* a bank's D16 state as the handle keeps it: one slot's code | esc, the encoder's mirror, and beside them what the device
 * holds: the decoder's base and the decoded matrix */
struct Bank {
    int32_t A, T;
    std::vector<int16_t> code;
    std::vector<int32_t> esc, mirror, base, out;
    int32_t n_esc = 0;
    Bank(int32_t A_, int32_t T_) : A(A_), T(T_), code((size_t)A_ * T_, 0), esc((size_t)A_ * T_ * 2, 0),
                                   mirror((size_t)A_ * T_, 0), base((size_t)A_ * T_, 0), out((size_t)A_ * T_, 12345) {}
    kfpos_delta_slot slot(int32_t capacity = -1) {
        return kfpos_delta_slot{code.data(), esc.data(), &n_esc, capacity < 0 ? A * T : capacity, mirror.data(), T, A};
    }
    /* one round: put every element of a tag that is not skipped (ascending), decode, and compare. Returns the number of
     * puts that were refused */
    int round(const std::vector<int32_t> &v, const std::vector<uint8_t> *skip = nullptr, int32_t capacity = -1) {
        const kfpos_delta_slot d = slot(capacity);
        n_esc = 0;
        int refused = 0;
        std::vector<double> dt((size_t)T, 0.05);
        for (int32_t t = 0; skip && t < T; ++t)
            if ((*skip)[t]) dt[t] = -1.0;
        for (int64_t e = 0; e < (int64_t)A * T; ++e) {
            if (skip && (*skip)[e % T]) continue;
            if (kfpos_d16_put(&d, e, v[e])) ++refused;
        }
        if (refused) return refused;
        for (int32_t k = 1; k < n_esc; ++k) CHECK(esc[2 * k] > esc[2 * (k - 1)]);
        for (int32_t k = 0; k < n_esc; ++k) CHECK(code[esc[2 * k]] == KFPOS_D16_ESCAPE);
        const std::vector<int32_t> before = base;
        kfpos_d16_decode_ref(code.data(), esc.data(), n_esc, skip ? dt.data() : nullptr, T, A, base.data(), out.data());
        for (int64_t e = 0; e < (int64_t)A * T; ++e) {
            const bool sk = skip && (*skip)[e % T];
            CHECK(out[e] == (sk ? 0 : (v[e] > 0 ? v[e] : 0)));
            if (sk || v[e] <= 0) CHECK(base[e] == before[e]);
            else CHECK(base[e] == v[e]);
        }
        CHECK(base == mirror);
        return 0;
    }
};

static void check_boundaries() {
    where = "boundaries";
    const int32_t B = 1000000;
    const int64_t deltas[5] = {-32766, -32767, -32768, 32767, 32768};
    Bank b(1, 5);
    CHECK(b.round(std::vector<int32_t>(5, B)) == 0); /* from a zero base: 1 000 000 escapes */
    CHECK(b.n_esc == 5);
    std::vector<int32_t> v(5);
    for (int k = 0; k < 5; ++k) v[k] = (int32_t)(B + deltas[k]);
    CHECK(b.round(v) == 0);
    CHECK(b.code[0] == -32766);                  /* the inner two boundaries are deltas */
    CHECK(b.code[3] == 32767);
    CHECK(b.code[1] == KFPOS_D16_ESCAPE && b.code[2] == KFPOS_D16_ESCAPE && b.code[4] == KFPOS_D16_ESCAPE);
    CHECK(b.n_esc == 3 && b.esc[0] == 1 && b.esc[2] == 2 && b.esc[4] == 4);
    CHECK(b.esc[1] == v[1] && b.esc[3] == v[2] && b.esc[5] == v[4]);
    /* from a zero base: 32767 is a delta, 32768 escapes */
    Bank z(1, 2);
    CHECK(z.round({32767, 32768}) == 0);
    CHECK(z.code[0] == 32767 && z.code[1] == KFPOS_D16_ESCAPE && z.n_esc == 1);
}

static void check_absent_and_extremes() {
    where = "absent";
    Bank b(2, 3);
    CHECK(b.round({0, -1, INT32_MIN, 5, 70000, INT32_MAX}) == 0);
    CHECK(b.code[0] == KFPOS_D16_ABSENT && b.code[1] == KFPOS_D16_ABSENT && b.code[2] == KFPOS_D16_ABSENT);
    CHECK(b.code[3] == 5 && b.code[4] == KFPOS_D16_ESCAPE && b.code[5] == KFPOS_D16_ESCAPE && b.n_esc == 2);
    /* a base near INT32_MAX with a small v: the difference is taken in 64 bits */
    CHECK(b.round({3, 0, 1, 0, 70001, 1}) == 0);
    CHECK(b.code[5] == KFPOS_D16_ESCAPE && b.code[4] == 1 && b.code[3] == KFPOS_D16_ABSENT);
    CHECK(b.mirror[5] == 1 && b.mirror[3] == 5); /* an absent element keeps its base */
    /* absent -> present: against the base kept, not against zero */
    CHECK(b.round({4, 9, 0, 6, 0, INT32_MAX}) == 0);
    CHECK(b.code[3] == 1 && b.code[0] == 1 && b.code[5] == KFPOS_D16_ESCAPE && b.code[4] == KFPOS_D16_ABSENT);
    CHECK(b.round({0, 0, 0, 0, 70002, 0}) == 0);
    CHECK(b.code[4] == 1 && b.mirror[5] == INT32_MAX);
}

static void check_skipped_tags() {
    where = "skipped";
    std::mt19937 rng(7);
    const int32_t A = 3, T = 7;
    Bank b(A, T);
    std::vector<int32_t> v((size_t)A * T);
    for (int r = 0; r < 12; ++r) {
        std::vector<uint8_t> skip(T, 0);
        for (int32_t t = 0; t < T; ++t) skip[t] = r % 3 == 2 && (t + r) % 3 == 1;
        for (auto &x : v) x = (int32_t)(rng() % 5 == 0 ? 0 : 2000 + rng() % 100000);
        for (int64_t e = 0; e < (int64_t)A * T; ++e) /* stale codes of the silent tags: anything, ESCAPE included */
            if (skip[e % T]) b.code[e] = rng() % 4 == 0 ? (int16_t)KFPOS_D16_ESCAPE : (int16_t)rng();
        where = "skipped round " + std::to_string(r);
        CHECK(b.round(v, &skip) == 0);
    }
    /* a forged entry for a silent tag is not read */
    std::vector<uint8_t> skip(T, 0);
    skip[2] = 1;
    const kfpos_delta_slot d = b.slot();
    b.n_esc = 0;
    for (int64_t e = 0; e < (int64_t)A * T; ++e)
        if (!skip[e % T]) CHECK(kfpos_d16_put(&d, e, 0) == 0);
    b.esc[0] = 2, b.esc[1] = 777777, b.n_esc = 1;
    std::vector<double> dt(T, 0.1);
    dt[2] = -1.0;
    const std::vector<int32_t> before = b.base;
    kfpos_d16_decode_ref(b.code.data(), b.esc.data(), b.n_esc, dt.data(), T, A, b.base.data(), b.out.data());
    CHECK(b.base == before && b.base == b.mirror);
    for (int32_t x : b.out) CHECK(x == 0);
}

static void check_full_list() {
    where = "full list";
    Bank b(2, 2);
    CHECK(b.round({100000, 100001, 100002, 5}, nullptr, 3) == 0); /* exactly full */
    CHECK(b.n_esc == 3);
    Bank c(2, 2);
    const kfpos_delta_slot d = c.slot(3);
    for (int64_t e = 0; e < 3; ++e) CHECK(kfpos_d16_put(&d, e, 100000 + (int32_t)e) == 0);
    c.code[3] = 77;
    CHECK(kfpos_d16_put(&d, 3, 200000) == -1); /* one beyond: refused, nothing written */
    CHECK(c.n_esc == 3 && c.code[3] == 77 && c.mirror[3] == 0);
    /* the handle's capacity, max_anchors * n_tags, holds a matrix in which everything escapes */
    Bank f(2, 3);
    CHECK(f.round(std::vector<int32_t>(6, 1 << 20)) == 0);
    CHECK(f.n_esc == 6);
}

static void check_random_sequences() {
    std::mt19937 rng(11);
    for (int32_t T : {1, 5, 64, 65})
        for (int32_t A : {1, 5, 8}) {
            Bank b(A, T);
            std::vector<int32_t> v((size_t)A * T, 0);
            for (int r = 0; r < 10; ++r) {
                where = "random T=" + std::to_string(T) + " A=" + std::to_string(A) + " round " + std::to_string(r);
                for (auto &x : v) {
                    const unsigned k = rng() % 16;
                    if (k == 0) x = 0;
                    else if (k == 1) x = (int32_t)(rng() % 0x7fffffffu) + 1; /* anywhere: jumps */
                    else if (k == 2) x = -(int32_t)(rng() % 1000);
                    else x = (x > 0 ? x : 30000) + (int32_t)(rng() % 201) - 100;
                }
                std::vector<uint8_t> skip(T, 0);
                for (auto &s : skip) s = r % 4 == 3 && rng() % 3 == 0;
                CHECK(b.round(v, r % 4 == 3 ? &skip : nullptr) == 0);
            }
        }
}

static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }
static void check_layout() {
    for (size_t T : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4099})
        for (size_t A : {(size_t)1, (size_t)5, (size_t)8, (size_t)64}) {
            where = "layout T=" + std::to_string(T) + " A=" + std::to_string(A);
            const kfpos_layout::Delta L = kfpos_layout::delta_layout(kfpos_layout::Sizes{T, A, 4, 6, 21, 8});
            const size_t n = A * T;
            CHECK(L.code % 256 == 0 && L.esc % 256 == 0);           /* aligned */
            CHECK(L.code == 0 && L.code + n * 2 <= L.esc);          /* disjoint, in this order */
            CHECK(L.esc == L.code + up256(n * 2));                  /* neighbours: one copy moves code | pairs in use */
            CHECK(L.esc + n * 8 <= L.bytes && L.bytes == L.esc + up256(n * 8)); /* inside */
        }
}

template <class E>
static bool rd(std::FILE *f, E *p, size_t n) { return std::fread(p, sizeof(E), n, f) == n; }
template <class E>
static bool wr(std::FILE *f, const E *p, size_t n) { return std::fwrite(p, sizeof(E), n, f) == n; }

static int transcode(const char *in, const char *outp) {
    std::FILE *fi = std::fopen(in, "rb"), *fo = std::fopen(outp, "wb");
    int32_t hd[3];
    if (!fi || !fo || !rd(fi, hd, 3)) return 2;
    Bank b(hd[0], hd[1]);
    const size_t n = (size_t)hd[0] * hd[1];
    std::vector<int32_t> v(n);
    std::vector<uint8_t> skip(hd[1]);
    for (int32_t r = 0; r < hd[2]; ++r) {
        if (!rd(fi, v.data(), n) || !rd(fi, skip.data(), skip.size())) return 2;
        where = "file round " + std::to_string(r);
        if (b.round(v, &skip)) return 3;
        if (!wr(fo, b.code.data(), n) || !wr(fo, &b.n_esc, 1) || !wr(fo, b.esc.data(), (size_t)b.n_esc * 2) ||
            !wr(fo, b.out.data(), n) || !wr(fo, b.base.data(), n))
            return 2;
    }
    std::fclose(fi);
    std::fclose(fo);
    return failures ? 1 : 0;
}

int main(int argc, char **argv) {
    if (argc == 3) return transcode(argv[1], argv[2]);
    check_boundaries();
    check_absent_and_extremes();
    check_skipped_tags();
    check_full_list();
    check_random_sequences();
    check_layout();
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("OK %d\n", checks);
    return 0;
}
