/*
 * kfpos_host.h -- what the host units of libkfpos_hip.so share among themselves, around the handle (kfpos_internal.h) and
 * the argument blocks (kfpos_kargs.h): defined in kfpos_hip.hip unless noted, used by kfpos_hip_state.hip,
 * kfpos_hip_replay.hip and kfpos_hip_slots.hip as well. No kernel unit includes it.
 */
#ifndef KFPOS_HOST_H
#define KFPOS_HOST_H

#include <cstring>
#include <string>

#include "kfpos_internal.h"
#include "kfpos_kargs.h"

#define KFPOS_HIDDEN __attribute__((visibility("hidden")))
/* A round: what one call feeds the bank. ROUND_TOA / _IMU / _FUSED are KFPOS_SLOT_TOA / _IMU / _TOA_IMU and the
 * MODE_* of the step kernels; ROUND_SENSOR carries a KFPOS_SENSOR_* kind beside it. */
enum : int { ROUND_TOA = 0, ROUND_IMU = 1, ROUND_FUSED = 2, ROUND_SENSOR = 3 };
constexpr int ROUND_EMPTY = -1; /* Round::answer (no KFPOS_* code): one of the reference's empty virtuals -- n zero status words, KFPOS_OK */
struct Round {
    int answer;            /* KFPOS_OK: proceed; ROUND_EMPTY; KFPOS_ERR_ARG (no such kind), _MODEL, _STATE (anchors) */
    bool has_rng, has_imu; /* the inputs the kind carries, whatever the answer */
    int width, mode;       /* values per tag of a sensor sample (0: not a sensor round); KArgs::mode */
};
struct RoundIn { /* the inputs of a round, component-major device pointers */
    const int32_t *ranges;
    const void *err, *accel, *cov;
    const double *sensor;
};
/* may this handle take this kind of round? slot: a streaming round (no sensor kinds; a planar bank takes ranging only) */
KFPOS_HIDDEN Round round_check(const kfpos_handle *h, int kind, int32_t sensor_kind, bool slot);
KFPOS_HIDDEN int round_refusal(int answer); /* KFPOS_ERR_MODEL / _STATE as the call's return value, with the anchors text */
/* fill_args + the round's part of the argument block (latch = 1) */
KFPOS_HIDDEN void round_args(const kfpos_handle *h, const Round &r, const RoundIn &in, const double *dt, double dt_shared,
                             uint32_t *status, double *traj, kfpos_k::KArgs &a);
/* a call that cannot honour anchor cells, on a handle that has them: KFPOS_ERR_MODEL, and the text says why */
KFPOS_HIDDEN int cells_refusal(const char *who, const char *why);
constexpr const char *CELLS_NO_ROWS = "the compact work bank of a row list mixes rows of different cells in one wavefront, and the anchors are wave-uniform";
constexpr const char *CELLS_NO_REPLAY = "its kernel reads the one anchor table of the kernel arguments, and no cells form of it is built";
KFPOS_HIDDEN int drain_slots(kfpos_handle *h); /* kfpos_hip_slots.hip: wait for whatever the slots still have in flight */
/* row-list rounds, synchronous and streaming: the list's check (rows inside the bank, none twice), room for n listed tags
 * in the work block, and gather -> step -> scatter on stream s (a: round_args with the inputs at [.][n]) */
KFPOS_HIDDEN int rows_check(kfpos_handle *h, const char *who, const int32_t *rows, int32_t n);
KFPOS_HIDDEN int rows_reserve(kfpos_handle *h, size_t n);
KFPOS_HIDDEN int rows_step(kfpos_handle *h, hipStream_t s, const kfpos_layout::Rows &L, const int32_t *d_rows, int n, kfpos_k::KArgs &a);
KFPOS_HIDDEN void pose_bank_args(const kfpos_handle *h, kfpos_k::PoseArgs &a); /* the bank as the pose kernels read it */
inline kfpos_layout::Sizes handle_sizes(const kfpos_handle *h) {
    return {(size_t)h->cfg.n_tags, (size_t)h->cfg.max_anchors, (size_t)h->msz, h->n, h->psz, h->rsz};
}
inline kfpos_layout::Rows rows_layout(const kfpos_handle *h, size_t n) { /* the work block as it is, n tags listed */
    return kfpos_layout::rows_layout(handle_sizes(h), KFPOS_N_SLOTS, h->work_cap, n);
}
inline kfpos_plan::Inputs plan_inputs(const kfpos_handle *h) { /* kfpos_policy.h, of the handle as it is now */
    return kfpos_policy::plan_inputs(h->cfg, h->policy, h->full != 0, h->planar_sensors);
}
KFPOS_HIDDEN void fill_args(const kfpos_handle *h, kfpos_k::KArgs &a);           /* the handle's part of every argument block */
KFPOS_HIDDEN int launch_step(kfpos_handle *h, const kfpos_k::KArgs &a, hipStream_t s); /* the step kernel of the handle, a.T tags */

#define g_err (kfpos_error_text())
#define HIPCHK(expr)                                                                              \
    do {                                                                                          \
        hipError_t e_ = (expr);                                                                   \
        if (e_ != hipSuccess) {                                                                   \
            g_err = std::string(#expr) + ": " + hipGetErrorString(e_);                            \
            return KFPOS_ERR_HIP;                                                                 \
        }                                                                                         \
    } while (0)
using DevScope = KfposDevScope; /* kfpos_internal.h */

/* ---- staging (defined in kfpos_hip.hip; kfpos_hip_state.hip takes the same routes) ---- */
/* a region of the row-major staging area; regions live until the next stage_reset() (start of an API call) */
KFPOS_HIDDEN int stage_region(kfpos_handle *h, size_t bytes, void **out);
inline void stage_reset(kfpos_handle *h) { h->stage_used = 0; }
/* host row-major [n][C] -> component-major [C][n] of `esz`-byte elements: one copy (into `landing`, or a region of the
 * staging area) + a device-side turn */
KFPOS_HIDDEN int stage_in(kfpos_handle *h, void *dst, const void *src, size_t n, int C, size_t esz, void *landing = nullptr);
/* device [C][n] doubles -> host row-major [n][C] */
KFPOS_HIDDEN int stage_out(kfpos_handle *h, double *dst, const double *dsrc, size_t n, int C);
template <typename E>
inline void rows_to_cols_host(void *dst, const void *src, size_t n, int C) {
    const E *s = (const E *)src;
    E *d = (E *)dst;
    for (size_t t = 0; t < n; ++t)
        for (int c = 0; c < C; ++c) d[(size_t)c * n + t] = s[t * C + c];
}

/* ---- the route a host-buffer call takes to the device, chosen once per call ----
 * mapped (small banks, kfpos_handle::sm): inputs and outputs live in one host-pinned, device-mapped block; the CPU turns
 * the layout in place, the kernels read and write host memory over the bus, and the call ends with a synchronisation of
 * the null stream. staged: plain copies into device buffers and a layout kernel per array, ended by a device
 * synchronisation. A call names, per array, where it lives on either route (Place) and uses the operations below; it
 * never asks which route it is on. */
struct Place {
    size_t mapped; /* offset in the mapped block */
    void *dst;     /* staged: the component-major device array ... */
    void *landing; /* ... and where the row-major copy lands before its turn (null: a region of the staging area) */
};
constexpr size_t TAGS_STAGE_MAX = (size_t)16 << 20;
struct Route {
    kfpos_handle *h;
    unsigned char *host, *dev; /* the mapped block (host == null: staged; dev is then the region block() reserved) */
    size_t chunk;              /* block(): records it holds */

    void *at(const Place &p) const { return host ? dev + p.mapped : p.dst; }
    /* row-major host array [n][C] of esz-byte elements in, component-major at(p) */
    int in(const void *src, size_t n, int C, size_t esz, const Place &p) {
        if (!host) return stage_in(h, p.dst, src, n, C, esz, p.landing);
        if (esz == 4) rows_to_cols_host<uint32_t>(host + p.mapped, src, n, C);
        else rows_to_cols_host<uint64_t>(host + p.mapped, src, n, C);
        return KFPOS_OK;
    }
    /* dt of a call, validated: one value (dt_len == 1) travels in the arguments, an array goes up. null = shared */
    int dt_in(const double *dt, int32_t dt_len, size_t n, const Place &p, const double **d_dt) {
        *d_dt = dt_len == 1 ? nullptr : (const double *)at(p);
        return dt_len == 1 ? KFPOS_OK : in(dt, n, 1, sizeof(double), p);
    }
    /* component-major doubles [C][n] at device address d (inside a Place of this call) out to row-major host */
    int out(double *dst, const double *d, size_t n, int C) {
        if (!host) return stage_out(h, dst, d, n, C);
        const double *s = (const double *)(host + ((const unsigned char *)d - dev));
        for (size_t t = 0; t < n; ++t)
            for (int c = 0; c < C; ++c) dst[t * C + c] = s[(size_t)c * n + t];
        return KFPOS_OK;
    }
    /* the call's launches have completed (a mapped block's results are visible) */
    int sync() {
        HIPCHK(host ? hipStreamSynchronize(nullptr) : hipDeviceSynchronize());
        return KFPOS_OK;
    }
    /* n status words delivered, after sync() */
    int words(uint32_t *status, const Place &p, size_t n) {
        if (status && host) std::memcpy(status, host + p.mapped, sizeof(uint32_t) * n);
        else if (status) HIPCHK(hipMemcpy(status, p.dst, sizeof(uint32_t) * n, hipMemcpyDeviceToHost));
        return KFPOS_OK;
    }
    int finish(uint32_t *status, const Place &p, size_t n) {
        const int rc = sync();
        return rc ? rc : words(status, p, n);
    }
    /* staged: p.dst = `bytes` of the staging area (reserve() first where several are held at once, so that none moves
     * while another is in use); mapped: the block has its places already */
    int reserve(size_t bytes) {
        void *probe = nullptr;
        const int rc = host ? KFPOS_OK : stage_region(h, bytes, &probe);
        if (!host) stage_reset(h);
        return rc;
    }
    int region(size_t bytes, Place &p) { return host ? KFPOS_OK : stage_region(h, bytes, &p.dst); }
    /* The per-tag calls stage records: the whole mapped block, or one region of the staging area filled and emptied
     * with plain copies, addressed as dev + offset. Sized for n records of `rec` bytes, at most TAGS_STAGE_MAX: longer
     * lists go through it in chunks of `chunk` (>= 1) records. */
    int block(size_t rec, size_t n) {
        size_t cap = h->sm.bytes;
        if (!host) {
            cap = rec * n < TAGS_STAGE_MAX ? rec * n : TAGS_STAGE_MAX;
            const int rc = stage_region(h, cap, (void **)&dev);
            if (rc) return rc;
        }
        chunk = cap / rec;
        if (chunk == 0) { /* (a loop over chunks of nothing would never end) */
            g_err = "per-tag staging holds less than one tag";
            return KFPOS_ERR_STATE;
        }
        return KFPOS_OK;
    }
    hipError_t up(size_t off, const void *src, size_t bytes) const {
        if (!host) return hipMemcpy(dev + off, src, bytes, hipMemcpyHostToDevice);
        std::memcpy(host + off, src, bytes);
        return hipSuccess;
    }
    hipError_t down(void *dst, size_t off, size_t bytes) const {
        if (!host) return hipMemcpy(dst, dev + off, bytes, hipMemcpyDeviceToHost);
        std::memcpy(dst, host + off, bytes);
        return hipSuccess;
    }
};
KFPOS_HIDDEN Route route_of(kfpos_handle *h);
/* kfpos_hip_state.hip, for the row-list steps: the part of the per-tag kernels' arguments every call shares (the bank's
 * arrays), and the bounds check of a row list (every row inside [0, n_tags); unique: none twice) */
KFPOS_HIDDEN void tag_args(const kfpos_handle *h, kfpos_k::TagArgs &a);
KFPOS_HIDDEN int tags_check(const kfpos_handle *h, const char *who, const int32_t *rows, int32_t n, bool unique);

#endif /* KFPOS_HOST_H */
