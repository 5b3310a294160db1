/*
 * kfpos_host_layout.h -- the byte layouts of the three blocks the host side carves up by offset: the mapped block of a
 * small bank, the pinned / device block of a streaming slot (and its D16 block), and the device block of the row-list steps. Pure arithmetic
 * on the handle's sizes: no HIP header, g++ compiles it alone (tests/layout/layout_driver.cpp checks that the regions are
 * aligned, disjoint and inside the block -- the copy stream runs ahead of the compute stream on the strength of that).
 */
#ifndef KFPOS_HOST_LAYOUT_H
#define KFPOS_HOST_LAYOUT_H

#include <cstddef>
#include <cstdint>

namespace kfpos_k {
enum : int { TB_POS = 0, TB_VEL, TB_P, TB_IMU_ACC, TB_IMU_COV, TB_LATCH, TB_N }; /* TagArgs::buf: the bank's arrays */
constexpr int LATCH_ROWS = 15;                                                   /* planar filter: latched sample rows */
} // namespace kfpos_k

namespace kfpos_layout {

/* what a layout depends on: tags, anchor columns, bytes per measurement element, state dimension, stored covariance
 * entries per tag and bytes per entry */
struct Sizes {
    size_t T, A, m;
    int n, psz, rsz;
};

/* regions are handed out in order, each on a 256-byte boundary */
struct Bump {
    size_t off = 0;
    size_t region(size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) & ~(size_t)255;
        return o;
    }
};

/* the mapped block of a small bank: every input and output of a host-API call, component-major */
struct Mapped {
    size_t ranges, err, accel, cov, dt, sensor, status, out, bytes;
};
inline Mapped mapped_layout(const Sizes &s) {
    Bump b;
    Mapped L{};
    L.ranges = b.region(s.A * s.T * sizeof(int32_t));
    L.err = b.region(s.A * s.T * s.m);
    L.accel = b.region(3 * s.T * s.m);
    L.cov = b.region(9 * s.T * s.m);
    L.dt = b.region(s.T * sizeof(double));
    L.sensor = b.region(24 * s.T * sizeof(double));
    L.status = b.region(s.T * sizeof(uint32_t));
    L.out = b.region((size_t)(15 + s.n + s.n * s.n) * s.T * sizeof(double));
    L.bytes = b.off;
    return L;
}

/* a streaming slot, pinned host and device alike. The submit path relies on two runs of neighbours: ranges | err | accel |
 * cov | dt go up in one copy (a complete fused epoch), status | pos come back in one */
struct Slot {
    size_t ranges, err, accel, cov, dt, status, pos, bytes;
};
inline Slot slot_layout(const Sizes &s) {
    Bump b;
    Slot L{};
    L.ranges = b.region(s.A * s.T * sizeof(int32_t));
    L.err = b.region(s.A * s.T * s.m);
    L.accel = b.region(3 * s.T * s.m);
    L.cov = b.region(9 * s.T * s.m);
    L.dt = b.region(s.T * sizeof(double));
    L.status = b.region(s.T * sizeof(uint32_t));
    L.pos = b.region(3 * s.T * sizeof(double));
    L.bytes = b.off;
    return L;
}

/* the D16 block of a streaming slot (KFPOS_SLOT_RANGES_D16), pinned host and device alike, beside the slot's own block:
 * one int16 code per range element, then the escape list at full capacity ((flat index, value) int32 pairs). Neighbours,
 * so that one copy moves the codes and the pairs in use */
struct Delta {
    size_t code, esc, bytes;
};
inline Delta delta_layout(const Sizes &s) {
    Bump b;
    Delta L{};
    L.code = b.region(s.A * s.T * sizeof(int16_t));
    L.esc = b.region(s.A * s.T * 2 * sizeof(int32_t));
    L.bytes = b.off;
    return L;
}

/* the block of the row-list steps: `slots` input areas for cap listed tags each (what a round uploads and returns, at
 * fixed places), then the work bank of n <= cap tags (their state and the turned inputs at stride n) */
struct Rows {
    size_t in_bytes; /* one input area and the places inside it */
    size_t i_rows, i_ranges, i_err, i_accel, i_cov, i_sensor, i_dt, i_status, i_pos;
    size_t w[kfpos_k::TB_N], w_flags, w_ranges, w_err, w_accel, w_cov, w_sensor; /* offsets in the block */
    size_t total;
};
inline Rows rows_layout(const Sizes &s, size_t slots, size_t cap, size_t n) {
    using namespace kfpos_k;
    const size_t A = s.A, m = s.m, imu = s.n == 9 ? 1 : 0, pl = s.n == 8 ? 1 : 0;
    Bump b;
    Rows L{};
    L.i_rows = b.region(cap * sizeof(int32_t));
    L.i_ranges = b.region(cap * A * sizeof(int32_t));
    L.i_err = b.region(cap * A * m);
    L.i_accel = b.region(imu * cap * 3 * m);
    L.i_cov = b.region(imu * cap * 9 * m);
    L.i_sensor = b.region(pl * cap * 24 * sizeof(double));
    L.i_dt = b.region(cap * sizeof(double));
    L.i_status = b.region(cap * sizeof(uint32_t));
    L.i_pos = b.region(cap * 3 * sizeof(double));
    L.in_bytes = b.off;
    b.off = slots * L.in_bytes;
    L.w[TB_POS] = b.region(3 * n * sizeof(double));
    L.w[TB_VEL] = b.region((s.n == 8 ? 4 : (s.n == 6 ? 0 : 3)) * n * sizeof(double));
    L.w[TB_P] = b.region((size_t)s.psz * n * s.rsz);
    L.w[TB_IMU_ACC] = b.region(imu * 3 * n * m);
    L.w[TB_IMU_COV] = b.region(imu * 6 * n * m);
    L.w[TB_LATCH] = b.region(pl * LATCH_ROWS * n * sizeof(double));
    L.w_flags = b.region(n * sizeof(uint32_t));
    L.w_ranges = b.region(n * A * sizeof(int32_t));
    L.w_err = b.region(n * A * m);
    L.w_accel = b.region(imu * n * 3 * m);
    L.w_cov = b.region(imu * n * 9 * m);
    L.w_sensor = b.region(pl * n * 24 * sizeof(double));
    L.total = b.off;
    return L;
}

} // namespace kfpos_layout
#endif /* KFPOS_HOST_LAYOUT_H */
