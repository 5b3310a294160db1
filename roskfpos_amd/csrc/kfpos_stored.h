/*
 * kfpos_stored.h -- one stored element of a component-major array to and from a double: the part of kfpos_kernels.h that
 * a kernel unit which moves state and runs no filter (kfpos_k_tags.hip) includes instead, and so needs no kfpos_core*.h.
 */
#ifndef KFPOS_STORED_H
#define KFPOS_STORED_H

#include "kfpos_kargs.h" /* KFPOS_STORE_*, KFPOS_HD */
#include "kfpos_p48.h"

namespace {

/* Component-major arrays are addressed as (wave-uniform row base) + (32-bit lane offset): the row base
 * stays in SGPRs (global_load ... v_off, s[base]) and one VGPR serves every array, instead of a 64-bit
 * per-lane address kept alive for each of the 30-60 rows between the loads and the final stores. */
template <typename REAL>
__device__ inline double ldrow(const void *p, size_t row, size_t T, uint32_t t) {
    return (double)(((const REAL *)p) + row * T)[t];
}
template <typename REAL>
__device__ inline void strow(void *p, size_t row, size_t T, uint32_t t, double v) {
    (((REAL *)p) + row * T)[t] = (REAL)v;
}

/* ---- the covariance in HBM: [entries][tag] of double / float, or KFPOS_STORE_P48 ----
 * P48 (kfpos_p48.h): sign, 8 exponent bits, 39 mantissa bits -- the single that truncates the value plus the next 16
 * mantissa bits; 9e-13 relative, 6 bytes per entry. Two planes so that both stay coalesced: [entries][T] uint32 followed
 * by [entries][T] uint16; a load is two loads, a conversion and a shift-or. (The 9-state filter amplifies a 24-bit
 * covariance to 1.6e-6 m over 100 epochs of the BASELINE trace, above the 1e-6 m bar.) */
struct p48 {};
template <typename REAL>
constexpr bool cov_is_rounded() { return !std::is_same<REAL, double>::value; }
/* what the storage type keeps of a value: applied between the epochs of a multi-epoch launch, so that it computes what
 * as many single-epoch launches would (KFPOS_STORE_P48: kfpos_p48.h -- three fp64 operations per entry) */
template <typename REAL>
__device__ inline double round_cov(double v) {
    if constexpr (std::is_same<REAL, p48>::value) return kfpos_p48_round(v);
    else return (double)(REAL)v;
}
template <typename REAL>
__device__ inline double ldcov(const void *p, size_t row, size_t rows, size_t T, uint32_t t) {
    if constexpr (std::is_same<REAL, p48>::value) { /* two coalesced planes: [rows][T] uint32, then [rows][T] uint16 */
        const uint32_t hi = (((const uint32_t *)p) + row * T)[t];
        const uint32_t lo = (((const uint16_t *)(((const uint32_t *)p) + rows * T)) + row * T)[t];
        return kfpos_p48_decode(hi, lo);
    } else {
        (void)rows;
        return (double)(((const REAL *)p) + row * T)[t];
    }
}
template <typename REAL>
__device__ inline void stcov(void *p, size_t row, size_t rows, size_t T, uint32_t t, double v) {
    if constexpr (std::is_same<REAL, p48>::value) {
        uint32_t hi;
        uint16_t lo;
        kfpos_p48_encode(kfpos_p48_round(v), &hi, &lo);
        (((uint32_t *)p) + row * T)[t] = hi;
        (((uint16_t *)(((uint32_t *)p) + rows * T)) + row * T)[t] = lo;
    } else {
        (void)rows;
        (((REAL *)p) + row * T)[t] = (REAL)v;
    }
}
/* one kernel per storage mode: F<covariance type, measurement type>(args) */
#define KFPOS_BY_STORAGE(st, F, ...)                                                                          \
    ((st) == KFPOS_STORE_F32 ? F<float, float>(__VA_ARGS__)                                                   \
     : (st) == KFPOS_STORE_MIXED ? F<double, float>(__VA_ARGS__)                                              \
     : (st) == KFPOS_STORE_P48 ? F<p48, float>(__VA_ARGS__) : F<double, double>(__VA_ARGS__))

} // namespace
#endif /* KFPOS_STORED_H */
