/* The byte layouts of roskfpos_amd/csrc/kfpos_host_layout.h (tests/test_host_layout.py builds this with g++ and the
 * address and undefined-behaviour sanitizers). For n_tags in {1, 63, 64, 65, 4096}, max_anchors in {1, 8, 16, 64},
 * measurement elements of 4 and 8 bytes and the state dimensions the handle knows with their covariance sizes: every
 * region of the mapped block, the slot block and the row-list block starts on a 256-byte boundary, regions do not
 * overlap, every region ends inside the total; the slot block keeps the two runs of neighbours the submit path copies in
 * one go; the input areas of the row-list block's slots overlap neither each other nor the work bank. */
#include <algorithm>
#include <cstdio>
#include <string>
#include <vector>

#include "kfpos_host_layout.h"

#ifndef KFPOS_N_SLOTS
#error "build with -DKFPOS_N_SLOTS=<the value of kfpos_internal.h>"
#endif

using namespace kfpos_layout;

static int failures = 0;
static std::string where;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            if (++failures <= 20) std::printf("FAIL %s: %s (line %d)\n", where.c_str(), #cond, __LINE__); \
        }                                                                              \
    } while (0)

struct Region {
    const char *name;
    size_t off, bytes;
};
static size_t up256(size_t b) { return (b + 255) & ~(size_t)255; }

/* aligned, disjoint (regions of zero bytes take no room), inside [lo, hi) */
static void check_regions(std::vector<Region> r, size_t lo, size_t hi) {
    for (const Region &a : r) {
        CHECK(a.off % 256 == 0);
        CHECK(a.off >= lo && a.off + a.bytes <= hi);
    }
    std::sort(r.begin(), r.end(), [](const Region &a, const Region &b) { return a.off != b.off ? a.off < b.off : a.bytes < b.bytes; });
    for (size_t k = 1; k < r.size(); ++k) CHECK(r[k - 1].off + r[k - 1].bytes <= r[k].off);
}

static void check_config(const Sizes &s, size_t slots) {
    const size_t T = s.T, A = s.A, m = s.m, n = (size_t)s.n;
    const size_t imu = s.n == 9 ? 1 : 0, pl = s.n == 8 ? 1 : 0;
    where = "T=" + std::to_string(T) + " A=" + std::to_string(A) + " m=" + std::to_string(m) + " n=" + std::to_string(n);

    const Mapped M = mapped_layout(s);
    check_regions({{"ranges", M.ranges, A * T * 4}, {"err", M.err, A * T * m}, {"accel", M.accel, 3 * T * m},
                   {"cov", M.cov, 9 * T * m}, {"dt", M.dt, T * 8}, {"sensor", M.sensor, 24 * T * 8},
                   {"status", M.status, T * 4}, {"out", M.out, (15 + n + n * n) * T * 8}},
                  0, M.bytes);
    /* a step of a row list parks the list in the output region */
    CHECK(M.out + T * 4 <= M.bytes);

    const Slot S = slot_layout(s);
    check_regions({{"ranges", S.ranges, A * T * 4}, {"err", S.err, A * T * m}, {"accel", S.accel, 3 * T * m},
                   {"cov", S.cov, 9 * T * m}, {"dt", S.dt, T * 8}, {"status", S.status, T * 4}, {"pos", S.pos, 3 * T * 8}},
                  0, S.bytes);
    /* one upload: ranges | err | accel | cov | dt, each right behind the one before (but for the padding) */
    CHECK(S.ranges == 0);
    CHECK(S.err == S.ranges + up256(A * T * 4));
    CHECK(S.accel == S.err + up256(A * T * m));
    CHECK(S.cov == S.accel + up256(3 * T * m));
    CHECK(S.dt == S.cov + up256(9 * T * m));
    /* one return: status | pos */
    CHECK(S.status == S.dt + up256(T * 8));
    CHECK(S.pos == S.status + up256(T * 4));
    CHECK(S.bytes == S.pos + up256(3 * T * 8));

    const size_t cap = T;
    for (size_t listed : {(size_t)1, cap / 2, cap}) {
        if (listed == 0) continue;
        where += " rows=" + std::to_string(listed);
        const Rows R = rows_layout(s, slots, cap, listed);
        std::vector<Region> all;
        for (size_t k = 0; k < slots; ++k) { /* the slots' input areas, each with its places at capacity */
            const size_t base = k * R.in_bytes;
            std::vector<Region> in = {{"rows", base + R.i_rows, cap * 4}, {"ranges", base + R.i_ranges, cap * A * 4},
                                      {"err", base + R.i_err, cap * A * m}, {"accel", base + R.i_accel, imu * cap * 3 * m},
                                      {"cov", base + R.i_cov, imu * cap * 9 * m}, {"sensor", base + R.i_sensor, pl * cap * 24 * 8},
                                      {"dt", base + R.i_dt, cap * 8}, {"status", base + R.i_status, cap * 4},
                                      {"pos", base + R.i_pos, cap * 3 * 8}};
            check_regions(in, base, base + R.in_bytes);
            all.insert(all.end(), in.begin(), in.end());
        }
        const size_t vel_rows = s.n == 8 ? 4 : (s.n == 6 ? 0 : 3);
        std::vector<Region> work = {{"pos", R.w[kfpos_k::TB_POS], 3 * listed * 8},
                                    {"vel", R.w[kfpos_k::TB_VEL], vel_rows * listed * 8},
                                    {"P", R.w[kfpos_k::TB_P], (size_t)s.psz * listed * s.rsz},
                                    {"imu_acc", R.w[kfpos_k::TB_IMU_ACC], imu * 3 * listed * m},
                                    {"imu_cov", R.w[kfpos_k::TB_IMU_COV], imu * 6 * listed * m},
                                    {"latch", R.w[kfpos_k::TB_LATCH], pl * kfpos_k::LATCH_ROWS * listed * 8},
                                    {"flags", R.w_flags, listed * 4}, {"ranges", R.w_ranges, listed * A * 4},
                                    {"err", R.w_err, listed * A * m}, {"accel", R.w_accel, imu * listed * 3 * m},
                                    {"cov", R.w_cov, imu * listed * 9 * m}, {"sensor", R.w_sensor, pl * listed * 24 * 8}};
        check_regions(work, slots * R.in_bytes, R.total); /* the work bank starts behind the last input area */
        all.insert(all.end(), work.begin(), work.end());
        check_regions(all, 0, R.total);
        /* the block is allocated for cap listed tags: any shorter list fits */
        CHECK(R.total <= rows_layout(s, slots, cap, cap).total);
        where.resize(where.rfind(" rows="));
    }
}

int main() {
    /* state dimension, stored covariance entries, bytes per entry: ML estimator; 6-state symmetric and full; planar; 9-state
     * -- in the widths the storage modes give an entry (4: float, 6: 48-bit, 8: double) */
    const int dims[5][2] = {{3, 6}, {6, 21}, {6, 36}, {8, 36}, {9, 45}};
    int configs = 0;
    for (size_t T : {(size_t)1, (size_t)63, (size_t)64, (size_t)65, (size_t)4096})
        for (size_t A : {(size_t)1, (size_t)8, (size_t)16, (size_t)64})
            for (size_t m : {(size_t)4, (size_t)8})
                for (const auto &d : dims)
                    for (int rsz : {4, 6, 8}) {
                        if (m == 8 && rsz != 8) continue; /* 8-byte measurements come with the 8-byte covariance */
                        check_config(Sizes{T, A, m, d[0], d[1], rsz}, KFPOS_N_SLOTS);
                        ++configs;
                    }
    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("OK %d\n", configs);
    return 0;
}
