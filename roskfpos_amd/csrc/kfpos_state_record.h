/*
 * kfpos_state_record.h -- the record of one tag, x (n) | P (n x n) | latch | height as include/kfpos.h documents
 * kfpos_get_state / kfpos_get_latch / kfpos_get_height, and where each of its components lives in the bank's
 * component-major arrays. The ONLY place that knows: the per-tag kernels (kfpos_k_tags.hip) are handed these tables, the
 * whole-bank accessors (kfpos_hip_state.hip) walk them on the CPU over host images of the arrays, through the element
 * codec below. No HIP header: g++ compiles it alone (tests/record/record_driver.cpp).
 */
#ifndef KFPOS_STATE_RECORD_H
#define KFPOS_STATE_RECORD_H

#include <cstddef>
#include <cstdint>

#include "kfpos_host_layout.h"
#include "kfpos_p48.h"

namespace kfpos_k {

/* One entry of the table that says where a component lives: kind = element type (TC_*), buf = index into TagArgs::buf
 * (TB_*), row = row of that component-major array. aux -- record table: 1 = the entry is stored through this component
 * (0: not stored at all, or the lower-triangle mirror of a packed entry); fresh table: what a fresh handle holds (0 =
 * zero, 1..5 = TagArgs::cst[aux - 1], 1..3 taken from TagArgs::init when that is given). */
struct TagComp {
    uint8_t kind, buf, row, aux;
};
enum : int { TC_NONE = 0, TC_F64 = 1, TC_COV = 2, TC_REAL = 3 }; /* double / stored covariance entry / kfpos_real */
constexpr int TAG_SECTIONS = 4;            /* x | P | latch | height */
constexpr int TAG_COMPS = 9 + 81 + 15 + 1; /* the longest record: no model has all of them at once */

/* packed index of the stored covariance entry (i, j) */
inline int pidx(int n, int full, int i, int j) {
    if (full) return i * n + j;
    if (i > j) { const int tt = i; i = j; j = tt; }
    return i * n - i * (i - 1) / 2 + (j - i);
}

/* kfpos_latch_dim: doubles per tag of kfpos_get_latch. The state dimension n names the model here (no kfpos.h in this
 * header): 9 = the 9-state filter, 8 = the planar filter, 3 = the ML estimator, 6 = the 6-state filter (no latch) */
inline int latch_width(int n) { return n == 9 ? 12 : (n == 8 ? LATCH_ROWS : (n == 3 ? 3 : 0)); }

/* The record, component by component: where it is stored, and whether a set stores THROUGH it (the mirror half of a
 * packed covariance is read, never written). Section s is comp[cbase[s]] .. comp[cbase[s + 1] - 1]; returns
 * cbase[TAG_SECTIONS], the length of the record. */
inline int record_table(int n, int full, TagComp comp[TAG_COMPS], int cbase[TAG_SECTIONS + 1]) {
    const int L = latch_width(n);
    int c = 0;
    auto put = [&](int kind, int buf, int row, int stored) {
        comp[c++] = TagComp{(uint8_t)kind, (uint8_t)buf, (uint8_t)row, (uint8_t)stored};
    };
    cbase[0] = c;
    for (int k = 0; k < n; ++k) {
        if (n == 8) { /* [x y vx vy 0 0 theta omega]; the height row of d_pos is its own section */
            static const int src[8] = {0, 1, 0, 1, -1, -1, 2, 3};
            if (src[k] < 0) put(TC_NONE, 0, 0, 0);
            else put(TC_F64, (k < 2) ? TB_POS : TB_VEL, src[k], 1);
        } else if (k < 3) put(TC_F64, TB_POS, k, 1);
        else if (n == 9 && k < 6) put(TC_F64, TB_VEL, k - 3, 1);
        else put(TC_NONE, 0, 0, 0); /* 6-state: the velocity is not a stored member; 9-state: a = 0 */
    }
    cbase[1] = c;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) put(TC_COV, TB_P, pidx(n, full, i, j), (full || j >= i) ? 1 : 0);
    cbase[2] = c;
    if (L == LATCH_ROWS)
        for (int k = 0; k < L; ++k) put(TC_F64, TB_LATCH, k, 1);
    else if (L == 3) /* ALGORITHM_ML: _previousEstimation, the seed of every solve */
        for (int k = 0; k < L; ++k) put(TC_F64, TB_VEL, k, 1);
    else if (L == 12) { /* acceleration [3] + the lower triangle {00,10,11,20,21,22} of its covariance, kfpos_real */
        static const int tri[3][3] = {{0, 1, 3}, {1, 2, 4}, {3, 4, 5}};
        for (int k = 0; k < 3; ++k) put(TC_REAL, TB_IMU_ACC, k, 1);
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) put(TC_REAL, TB_IMU_COV, tri[i][j], i >= j ? 1 : 0);
    }
    cbase[3] = c;
    if (n == 8) put(TC_F64, TB_POS, 2, 1);
    return cbase[TAG_SECTIONS] = c;
}

/* The stored rows of one tag, each once, and what kfpos_create (+ kfpos_set_planar) left in them: TagComp::aux = 0 zero,
 * 1..3 the start position, 4 / 5 the planar height / angle. Returns how many. */
inline int fresh_table(int n, int psz, TagComp comp[TAG_COMPS]) {
    int c = 0;
    auto put = [&](int kind, int buf, int row, int what) {
        comp[c++] = TagComp{(uint8_t)kind, (uint8_t)buf, (uint8_t)row, (uint8_t)what};
    };
    for (int k = 0; k < 3; ++k) put(TC_F64, TB_POS, k, (n == 8 && k == 2) ? 4 : 1 + k);
    if (n == 3)
        for (int k = 0; k < 3; ++k) put(TC_F64, TB_VEL, k, 1 + k); /* the solver's seed */
    if (n == 8)
        for (int k = 0; k < 4; ++k) put(TC_F64, TB_VEL, k, k == 2 ? 5 : 0); /* vx vy theta omega */
    if (n == 9)
        for (int k = 0; k < 3; ++k) put(TC_F64, TB_VEL, k, 0);
    for (int k = 0; k < psz; ++k) put(TC_COV, TB_P, k, 0);
    if (n == 9) {
        for (int k = 0; k < 3; ++k) put(TC_REAL, TB_IMU_ACC, k, 0);
        for (int k = 0; k < 6; ++k) put(TC_REAL, TB_IMU_COV, k, 0);
    }
    if (n == 8)
        for (int k = 0; k < LATCH_ROWS; ++k) put(TC_F64, TB_LATCH, k, 0);
    return c;
}

/* ---- host images: a bank array [rows][T] as it sits in device memory, copied to the host as it is ----
 * Element (row, t) of an image, by the kind of its table entry and the handle's sizes (s.T tags, s.m bytes per
 * kfpos_real, s.rsz bytes per stored covariance entry of s.psz per tag). KFPOS_STORE_P48 (kfpos_p48.h) keeps two planes:
 * [psz][T] uint32 | [psz][T] uint16. */
inline size_t elem_bytes(int kind, const kfpos_layout::Sizes &s) {
    return kind == TC_COV ? (size_t)s.rsz : (kind == TC_REAL ? s.m : sizeof(double));
}
inline double elem_load(int kind, const kfpos_layout::Sizes &s, const unsigned char *img, size_t row, size_t t) {
    const size_t k = row * s.T + t, e = elem_bytes(kind, s);
    if (e == 6) return kfpos_p48_decode(((const uint32_t *)img)[k], ((const uint16_t *)(img + (size_t)s.psz * s.T * 4))[k]);
    return e == 4 ? (double)((const float *)img)[k] : ((const double *)img)[k];
}
inline void elem_store(int kind, const kfpos_layout::Sizes &s, unsigned char *img, size_t row, size_t t, double v) {
    const size_t k = row * s.T + t, e = elem_bytes(kind, s);
    if (e == 6) /* rounded and encoded exactly as the kernels do */
        kfpos_p48_encode(kfpos_p48_round(v), &((uint32_t *)img)[k], &((uint16_t *)(img + (size_t)s.psz * s.T * 4))[k]);
    else if (e == 4) ((float *)img)[k] = (float)v;
    else ((double *)img)[k] = v;
}
/* an image that reaches down to row `hi` (a covariance image is always whole: its second plane starts behind psz rows) */
inline size_t image_bytes(int kind, const kfpos_layout::Sizes &s, int hi) {
    return (size_t)(kind == TC_COV ? s.psz : hi + 1) * s.T * elem_bytes(kind, s);
}
/* where rows lo .. hi lie in an image: one run of bytes -- the whole covariance image included --, or one per plane */
struct ByteRun {
    size_t off, bytes;
};
inline int image_runs(int kind, const kfpos_layout::Sizes &s, int lo, int hi, ByteRun run[2]) {
    const size_t T = s.T, cnt = (size_t)(hi - lo + 1) * T, e = elem_bytes(kind, s);
    if (e == 6 && (lo != 0 || hi + 1 != s.psz)) {
        run[0] = ByteRun{lo * T * 4, cnt * 4};
        run[1] = ByteRun{(size_t)s.psz * T * 4 + lo * T * 2, cnt * 2};
        return 2;
    }
    run[0] = ByteRun{lo * T * e, cnt * e};
    return 1;
}

/* ---- the walkers: one section of the record table (w entries from comp) for all s.T tags, rec = [T][w] ----
 * img[b] = the image of bank array b, for every array the section names. Tags go in blocks: a block's part of rec stays in
 * cache while each component's row of the image is walked contiguously, with the component decoded once per block and
 * not once per element (tag by tag, every element of an image lies T elements from the one before). */
constexpr size_t WALK_BLOCK = 16;
inline void record_out(const TagComp *comp, int w, const kfpos_layout::Sizes &s, const unsigned char *const img[TB_N], double *rec) {
    for (size_t t0 = 0; t0 < s.T; t0 += WALK_BLOCK)
        for (int k = 0; k < w; ++k) {
            const TagComp d = comp[k]; /* TC_NONE: a component the model does not store reads as 0 */
            for (size_t t = t0; t < s.T && t < t0 + WALK_BLOCK; ++t)
                rec[t * w + k] = d.kind == TC_NONE ? 0.0 : elem_load(d.kind, s, img[d.buf], d.row, t);
        }
}
/* a component with aux == 0 is never stored: rows of an image no entry stores through keep their bytes */
inline void record_in(const TagComp *comp, int w, const kfpos_layout::Sizes &s, unsigned char *const img[TB_N], const double *rec) {
    for (size_t t0 = 0; t0 < s.T; t0 += WALK_BLOCK)
        for (int k = 0; k < w; ++k) {
            const TagComp d = comp[k];
            for (size_t t = t0; d.aux && t < s.T && t < t0 + WALK_BLOCK; ++t) elem_store(d.kind, s, img[d.buf], d.row, t, rec[t * w + k]);
        }
}

} // namespace kfpos_k
#endif /* KFPOS_STATE_RECORD_H */
