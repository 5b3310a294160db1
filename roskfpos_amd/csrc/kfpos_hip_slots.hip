/*
 * kfpos_hip_slots.hip -- the streaming host API of libkfpos_hip.so (kfpos.h: kfpos_slot_*): KFPOS_N_SLOTS slots of pinned
 * host + device buffers and three streams, so that the upload of one round, the step of the one before and the return of
 * the one before that overlap (a whole-bank round may carry its ranges as int16 codes, KFPOS_SLOT_RANGES_D16: d16_*, below,
 * and kfpos_k_d16.hip). Whole-bank rounds and row-list rounds share the acquire, the round's part of the argument
 * block and the third stage; what a round may feed is decided by round_check, the row-list machinery (rows_check,
 * rows_reserve, rows_step) lives in kfpos_hip.hip, the lifecycle code it is built on in kfpos_hip_state.hip (kfpos_host.h
 * declares both).
 */
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "kfpos_host.h"

int drain_slots(kfpos_handle *h) {
    for (auto &sl : h->slot)
        if (sl.busy) {
            HIPCHK(hipEventSynchronize(sl.done));
            sl.busy = false;
        }
    return KFPOS_OK;
}

namespace {

int slots_init(kfpos_handle *h) {
    if (h->s_copy) return KFPOS_OK;
    h->so = kfpos_layout::slot_layout(handle_sizes(h));
    const size_t bytes = h->so.bytes;
    HIPCHK(hipStreamCreateWithFlags(h->s_copy.out(), hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(h->s_copy2.out(), hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(h->s_comp.out(), hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(h->s_back.out(), hipStreamNonBlocking));
    for (auto &sl : h->slot) {
        HIPCHK(hipHostMalloc((void **)sl.host.out(), bytes, hipHostMallocDefault));
        HIPCHK(hipMalloc((void **)sl.dev.out(), bytes));
        std::memset(sl.host, 0, bytes);
        HIPCHK(hipMemset(sl.dev, 0, bytes));
        HIPCHK(hipEventCreateWithFlags(sl.copied.out(), hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(sl.copied2.out(), hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(sl.computed.out(), hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(sl.done.out(), hipEventDisableTiming));
    }
    HIPCHK(hipDeviceSynchronize()); /* whatever the other entry points queued on the default stream comes first */
    return KFPOS_OK;
}

/* both acquires: the slot's last submission has consumed its inputs and delivered its outputs, then the pointers */
int slot_acquire(kfpos_handle *h, int32_t slot, bool listed, kfpos_epoch_slot *out) {
    g_err.clear();
    if (!h || !out || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    const int rc = slots_init(h);
    if (rc) return rc;
    auto &sl = h->slot[slot];
    if (listed && !sl.rows) HIPCHK(hipHostMalloc((void **)sl.rows.out(), sizeof(int32_t) * h->cfg.n_tags, hipHostMallocDefault));
    if (sl.busy) {
        HIPCHK(hipEventSynchronize(sl.done));
        sl.busy = false;
    }
    out->range_mm = (int32_t *)(sl.host + h->so.ranges);
    out->err_est = sl.host + h->so.err;
    out->accel = sl.host + h->so.accel;
    out->cov = sl.host + h->so.cov;
    out->dt = (double *)(sl.host + h->so.dt);
    out->status = (uint32_t *)(sl.host + h->so.status);
    out->pos = (double *)(sl.host + h->so.pos);
    return KFPOS_OK;
}

/* The head of both submits: the slot has been acquired and `flags` names a round a slot can carry (ranging, IMU only,
 * fused; the planar sensors go through kfpos_step_sensor / _rows). The model and anchors answer is the caller's to act
 * on: a row-list round looks at its list first. */
int submit_head(kfpos_handle *h, int32_t slot, int32_t flags, bool listed, Round &r) {
    auto &sl = h->slot[slot];
    if (!h->s_copy || sl.busy || (listed && !sl.rows)) {
        g_err = listed ? "kfpos_slot_submit_rows: acquire the slot first (kfpos_slot_acquire_rows)"
                       : "kfpos_slot_submit: acquire the slot first (kfpos_slot_acquire)";
        return KFPOS_ERR_STATE;
    }
    r = round_check(h, flags & 0xff, 0, true);
    return r.answer == KFPOS_ERR_ARG ? KFPOS_ERR_ARG : KFPOS_OK;
}

/* The third stage of both submits: `computed` on the compute stream, the round's copies (device -> pinned host) behind it on
 * the return stream, `done` behind them */
template <class Copies>
int submit_return(kfpos_handle *h, kfpos_handle::Slot &sl, Copies copies) {
    HIPCHK(hipEventRecord(sl.computed, h->s_comp));
    HIPCHK(hipStreamWaitEvent(h->s_back, sl.computed, 0));
    const int rc = copies();
    if (rc) return rc;
    HIPCHK(hipEventRecord(sl.done, h->s_back));
    sl.busy = true;
    return KFPOS_OK;
}

/* ---- KFPOS_SLOT_RANGES_D16 (kfpos.h, kfpos_d16.h) ---- */
/* the D16 blocks, allocated by the handle's first kfpos_slot_delta: per slot code | esc, pinned and on the device; per
 * handle the mirror and the device base, both zero */
int d16_init(kfpos_handle *h) {
    if (h->d16_base) return KFPOS_OK;
    const size_t n = (size_t)h->cfg.max_anchors * h->cfg.n_tags;
    h->d16 = kfpos_layout::delta_layout(handle_sizes(h));
    for (auto &sl : h->slot) {
        if (!sl.d16_host) {
            HIPCHK(hipHostMalloc((void **)sl.d16_host.out(), h->d16.bytes, hipHostMallocDefault));
            std::memset(sl.d16_host, 0, h->d16.bytes);
        }
        if (!sl.d16_dev) {
            HIPCHK(hipMalloc((void **)sl.d16_dev.out(), h->d16.bytes));
            HIPCHK(hipMemset(sl.d16_dev, 0, h->d16.bytes));
        }
    }
    h->d16_mirror.assign(n, 0);
    DevPtr<int32_t> base;
    HIPCHK(hipMalloc((void **)base.out(), n * sizeof(int32_t)));
    if (hipMemset(base, 0, n * sizeof(int32_t)) != hipSuccess || hipDeviceSynchronize() != hipSuccess) {
        g_err = "kfpos_slot_delta: clearing the device base failed";
        return KFPOS_ERR_HIP;
    }
    h->d16_base = std::move(base);
    return KFPOS_OK;
}

kfpos_delta_slot d16_view(kfpos_handle *h, kfpos_handle::Slot &sl) {
    const int64_t n = (int64_t)h->cfg.max_anchors * h->cfg.n_tags;
    return kfpos_delta_slot{(int16_t *)(sl.d16_host + h->d16.code), (int32_t *)(sl.d16_host + h->d16.esc), &sl.n_esc,
                            (int32_t)n, h->d16_mirror.data(), h->cfg.n_tags, h->cfg.max_anchors};
}

/* the escape list of a D16 round, in O(n_esc), before anything is enqueued: the kernel never sees an unchecked index.
 * dt: the slot's per-tag dt (the entries of a tag whose dt < 0 are not read beyond their index) or null */
int d16_check(const kfpos_handle *h, const kfpos_handle::Slot &sl, int32_t n_esc, const double *dt) {
    const int64_t n = (int64_t)h->cfg.max_anchors * h->cfg.n_tags, T = h->cfg.n_tags;
    if (n_esc < 0 || (int64_t)n_esc > n) {
        g_err = "kfpos_slot_submit: KFPOS_SLOT_RANGES_D16: n_esc = " + std::to_string(n_esc) + " is outside [0, " + std::to_string(n) + "] (the escape list's capacity)";
        return KFPOS_ERR_ARG;
    }
    const int16_t *code = (const int16_t *)(sl.d16_host + h->d16.code);
    const int32_t *esc = (const int32_t *)(sl.d16_host + h->d16.esc);
    int64_t prev = -1;
    for (int32_t k = 0; k < n_esc; ++k) {
        const int64_t i = esc[2 * (size_t)k];
        const int32_t v = esc[2 * (size_t)k + 1];
        const char *what = nullptr;
        if (i < 0 || i >= n) what = " lies outside the matrix";
        else if (i <= prev) what = " does not ascend (the list is strictly ascending by index)";
        else if (dt && dt[i % T] < 0.0) what = nullptr; /* a skipped tag's entry is not read */
        else if (code[i] != KFPOS_D16_ESCAPE) what = " points at a code that is not KFPOS_D16_ESCAPE";
        else if (v <= 0) what = " carries a value <= 0 (an absent range is KFPOS_D16_ABSENT)";
        if (what) {
            g_err = "kfpos_slot_submit: KFPOS_SLOT_RANGES_D16: escape entry " + std::to_string(k) + ": index " + std::to_string(i) + what;
            return KFPOS_ERR_ARG;
        }
        prev = i;
    }
    return KFPOS_OK;
}

/* a slot's submit has ended: an open slot is closed, and the base restarts at the next kfpos_slot_delta unless this
 * was a D16 round that went through (kfpos.h, "RESTART RULE") */
void d16_close(kfpos_handle *h, int32_t slot, bool d16_round, int rc) {
    if (h->d16_open == slot) {
        h->d16_open = -1;
        if (!d16_round || rc != KFPOS_OK) h->d16_restart = true;
    } else if (d16_round && rc != KFPOS_OK) h->d16_restart = true;
}

int submit_whole(kfpos_handle *h, int32_t slot, int32_t flags, double dt_shared);

} // namespace

extern "C" {

int kfpos_slot_count(const kfpos_handle *h) { return h ? KFPOS_N_SLOTS : 0; }

int kfpos_slot_acquire(kfpos_handle *h, int32_t slot, kfpos_epoch_slot *out) { return slot_acquire(h, slot, false, out); }

int kfpos_slot_acquire_rows(kfpos_handle *h, int32_t slot, kfpos_rows_slot *out) {
    kfpos_epoch_slot e;
    const int rc = slot_acquire(h, slot, true, out ? &e : nullptr);
    if (rc) return rc;
    *out = kfpos_rows_slot{h->slot[slot].rows, e.range_mm, e.err_est, e.accel, e.cov, e.dt, e.status, e.pos, h->cfg.n_tags};
    return KFPOS_OK;
}

int kfpos_slot_submit(kfpos_handle *h, int32_t slot, int32_t flags, double dt_shared) {
    g_err.clear();
    if (!h || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    const bool d16 = (flags & KFPOS_SLOT_RANGES_D16) != 0;
    int rc = KFPOS_OK;
    if (d16 && (flags & 0xff) == KFPOS_SLOT_IMU) {
        g_err = "kfpos_slot_submit: KFPOS_SLOT_RANGES_D16 on a round without ranging (KFPOS_SLOT_IMU)";
        rc = KFPOS_ERR_ARG;
    } else if (d16 && h->d16_open != slot) {
        g_err = "kfpos_slot_submit: KFPOS_SLOT_RANGES_D16: open the slot first (kfpos_slot_delta)";
        rc = KFPOS_ERR_STATE;
    }
    if (rc == KFPOS_OK) rc = submit_whole(h, slot, flags, dt_shared);
    d16_close(h, slot, d16, rc);
    return rc;
}

} // extern "C"

namespace {

int submit_whole(kfpos_handle *h, int32_t slot, int32_t flags, double dt_shared) {
    const bool d16 = (flags & KFPOS_SLOT_RANGES_D16) != 0;
    Round r;
    const int rc = submit_head(h, slot, flags, false, r);
    if (rc) return rc;
    int rc_d16 = KFPOS_OK;
    auto &sl = h->slot[slot];
    const auto &so = h->so;
    const size_t T = h->cfg.n_tags, A = h->cfg.max_anchors, m = h->msz;
    if (r.answer == ROUND_EMPTY) {
        std::memset(sl.host + so.status, 0, sizeof(uint32_t) * T);
        return KFPOS_OK;
    }
    if (r.answer) return round_refusal(r.answer);
    const double *slot_dt = (const double *)(sl.host + so.dt);
    const int32_t n_esc = sl.n_esc; /* read once: what is checked is what is copied and decoded */
    if (d16 && (rc_d16 = d16_check(h, sl, n_esc, (flags & KFPOS_SLOT_DT_PER_TAG) ? slot_dt : nullptr))) return rc_d16;
    /* 1. inputs: pinned host -> device on the copy stream. A complete fused epoch is one contiguous block of the slot
     * (ranges | err | accel | cov | dt): one DMA instead of five. Measured on this platform (tools/exp/h2d_probe.hip,
     * profiles/r02g_*): a lone 7.3 MB copy moves at 27-35 GB/s while the GPU is otherwise idle and at 53 GB/s while a
     * kernel is running; two halves on two streams reach 55 GB/s when ALONE but were slower inside this pipeline
     * (KFPOS_SLOT_SPLIT_BYTES=n turns that on for copies of n bytes and more; default off). */
    bool second = false;
    auto h2d = [&](size_t off, size_t bytes) -> hipError_t {
        if (h->policy.slot_split_bytes == 0 || bytes < h->policy.slot_split_bytes) return hipMemcpyAsync(sl.dev + off, sl.host + off, bytes, hipMemcpyHostToDevice, h->s_copy);
        const size_t half = (bytes / 2 + 255) & ~(size_t)255;
        hipError_t e = hipMemcpyAsync(sl.dev + off, sl.host + off, half, hipMemcpyHostToDevice, h->s_copy);
        if (e != hipSuccess) return e;
        second = true;
        return hipMemcpyAsync(sl.dev + off + half, sl.host + off + half, bytes - half, hipMemcpyHostToDevice, h->s_copy2);
    };
    /* a slot's device copy of err / cov may still be read by a later submission of another slot that reused it
     * (KFPOS_SLOT_REUSE_*) -- also after a third slot has uploaded newer ones in between */
    auto guard = [&](hipEvent_t last_use) -> hipError_t {
        hipError_t e = hipStreamWaitEvent(h->s_copy, last_use, 0);
        return e != hipSuccess ? e : hipStreamWaitEvent(h->s_copy2, last_use, 0);
    };
    const bool up_err = r.has_rng && !(flags & KFPOS_SLOT_REUSE_ERR), up_cov = r.has_imu && !(flags & KFPOS_SLOT_REUSE_COV);
    if (r.has_rng && !up_err && h->err_slot < 0) {
        g_err = "KFPOS_SLOT_REUSE_ERR before any errorEstimation was submitted";
        return KFPOS_ERR_STATE;
    }
    if (r.has_imu && !up_cov && h->cov_slot < 0) {
        g_err = "KFPOS_SLOT_REUSE_COV before any covariance was submitted";
        return KFPOS_ERR_STATE;
    }
    if (up_err && sl.err_reader) HIPCHK(guard(sl.err_reader));
    if (up_cov && sl.cov_reader) HIPCHK(guard(sl.cov_reader));
    /* a D16 round: the block's upload starts behind the ranges region, which the decode kernel fills on the device */
    if (up_err && up_cov) { /* the whole block in one go */
        const size_t end = (flags & KFPOS_SLOT_DT_PER_TAG) ? so.dt + T * sizeof(double) : so.cov + 9 * T * m;
        const size_t from = d16 ? so.err : so.ranges;
        HIPCHK(h2d(from, end - from));
    } else {
        if (r.has_rng && !d16) HIPCHK(h2d(so.ranges, up_err ? so.err + A * T * m - so.ranges : A * T * sizeof(int32_t)));
        if (r.has_rng && d16 && up_err) HIPCHK(h2d(so.err, A * T * m));
        if (r.has_imu) HIPCHK(h2d(so.accel, up_cov ? so.cov + 9 * T * m - so.accel : 3 * T * m));
        if (flags & KFPOS_SLOT_DT_PER_TAG) HIPCHK(h2d(so.dt, T * sizeof(double)));
    }
    if (d16) /* code | the pairs in use: neighbours, one copy */
        HIPCHK(hipMemcpyAsync(sl.d16_dev, sl.d16_host, h->d16.esc + (size_t)n_esc * 2 * sizeof(int32_t), hipMemcpyHostToDevice, h->s_copy));
    if (up_err) h->err_slot = slot;
    if (up_cov) h->cov_slot = slot;
    HIPCHK(hipEventRecord(sl.copied, h->s_copy));
    if (second) HIPCHK(hipEventRecord(sl.copied2, h->s_copy2));
    /* 2. the step, on the compute stream (submissions run in order: the filter state is sequential) */
    HIPCHK(hipStreamWaitEvent(h->s_comp, sl.copied, 0));
    if (second) HIPCHK(hipStreamWaitEvent(h->s_comp, sl.copied2, 0));
    if (d16) { /* codes -> the slot's device ranges region and the device base, ahead of the step on the same stream */
        const kfpos_k::D16Args g = {(const int16_t *)(sl.d16_dev + h->d16.code), (const int32_t *)(sl.d16_dev + h->d16.esc),
                                    (uint32_t)n_esc, (uint32_t)(A * T), (uint32_t)T,
                                    (flags & KFPOS_SLOT_DT_PER_TAG) ? (const double *)(sl.dev + so.dt) : nullptr,
                                    h->d16_base, (int32_t *)(sl.dev + so.ranges)};
        kfpos_k::launch_decode_d16(h->s_comp, g);
        HIPCHK(hipGetLastError());
    }
    const RoundIn in = {(const int32_t *)(sl.dev + so.ranges), r.has_rng ? h->slot[h->err_slot].dev + so.err : nullptr,
                        sl.dev + so.accel, r.has_imu ? h->slot[h->cov_slot].dev + so.cov : nullptr, nullptr};
    const bool want_pose = !(flags & KFPOS_SLOT_NO_POSE);
    KArgs a;
    round_args(h, r, in, (flags & KFPOS_SLOT_DT_PER_TAG) ? (const double *)(sl.dev + so.dt) : nullptr, dt_shared,
               (uint32_t *)(sl.dev + so.status), want_pose ? (double *)(sl.dev + so.pos) : nullptr, a);
    const int rcl = launch_step(h, a, h->s_comp);
    if (rcl) return rcl;
    if (r.has_rng) h->slot[h->err_slot].err_reader = sl.computed;
    if (r.has_imu) h->slot[h->cov_slot].cov_reader = sl.computed;
    /* 3. outputs: status words and poses sit side by side in the slot, one copy */
    return submit_return(h, sl, [&]() -> int {
        HIPCHK(hipMemcpyAsync(sl.host + so.status, sl.dev + so.status,
                              want_pose ? so.pos + 3 * T * sizeof(double) - so.status : T * sizeof(uint32_t),
                              hipMemcpyDeviceToHost, h->s_back));
        return KFPOS_OK;
    });
}

} // namespace

extern "C" {

int kfpos_slot_delta(kfpos_handle *h, int32_t slot, kfpos_delta_slot *out) {
    g_err.clear();
    if (!h || !out || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    const int64_t n = (int64_t)h->cfg.max_anchors * h->cfg.n_tags;
    if (n > INT32_MAX) {
        g_err = "kfpos_slot_delta: max_anchors * n_tags exceeds INT32_MAX (flat indices are int32)";
        return KFPOS_ERR_ARG;
    }
    auto &sl = h->slot[slot];
    if (!h->s_copy || sl.busy) {
        g_err = "kfpos_slot_delta: acquire the slot first (kfpos_slot_acquire)";
        return KFPOS_ERR_STATE;
    }
    if (h->d16_open >= 0 && h->d16_open != slot) {
        g_err = "kfpos_slot_delta: slot " + std::to_string(h->d16_open) + " is open (one D16 round is encoded at a time: submit it first)";
        return KFPOS_ERR_STATE;
    }
    if (h->d16_open == slot) h->d16_restart = true; /* opened again: the mirror may have moved for a round never sent */
    const int rc = d16_init(h);
    if (rc) return rc;
    if (h->d16_restart) { /* behind every decode already queued, ahead of the next one */
        HIPCHK(hipMemsetAsync(h->d16_base, 0, (size_t)n * sizeof(int32_t), h->s_comp));
        std::memset(h->d16_mirror.data(), 0, (size_t)n * sizeof(int32_t));
        h->d16_restart = false;
    }
    sl.n_esc = 0;
    h->d16_open = slot;
    *out = d16_view(h, sl);
    return KFPOS_OK;
}

int kfpos_slot_encode_ranges(kfpos_handle *h, int32_t slot, int32_t flags) {
    g_err.clear();
    if (!h || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    if (h->d16_open != slot) {
        g_err = "kfpos_slot_encode_ranges: open the slot first (kfpos_slot_delta)";
        return KFPOS_ERR_STATE;
    }
    auto &sl = h->slot[slot];
    const kfpos_delta_slot d = d16_view(h, sl);
    const int32_t *r = (const int32_t *)(sl.host + h->so.ranges);
    const double *dt = (flags & KFPOS_SLOT_DT_PER_TAG) ? (const double *)(sl.host + h->so.dt) : nullptr;
    const int64_t T = h->cfg.n_tags, A = h->cfg.max_anchors;
    for (int64_t a = 0; a < A; ++a) /* ascending flat index: the escape list comes out sorted */
        for (int64_t t = 0; t < T; ++t) {
            if (dt && dt[t] < 0.0) continue;
            if (kfpos_d16_put(&d, a * T + t, r[a * T + t])) {
                g_err = "kfpos_slot_encode_ranges: the escape list is full (elements were put before the call)";
                return KFPOS_ERR_STATE;
            }
        }
    return KFPOS_OK;
}

int kfpos_slot_wait(kfpos_handle *h, int32_t slot) {
    g_err.clear();
    if (!h || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    auto &sl = h->slot[slot];
    if (sl.busy) {
        HIPCHK(hipEventSynchronize(sl.done));
        sl.busy = false;
    }
    return KFPOS_OK;
}

int kfpos_slot_submit_rows(kfpos_handle *h, int32_t slot, int32_t flags, int32_t n, double dt_shared) {
    g_err.clear();
    if (!h || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    if (h->n_cells > 0) return cells_refusal("kfpos_slot_submit_rows", CELLS_NO_ROWS); /* (nothing of the slot has changed) */
    DevScope dev_(h->cfg.device);
    d16_close(h, slot, false, KFPOS_OK); /* an open slot sent as a row list: its D16 round is abandoned */
    if (flags & KFPOS_SLOT_RANGES_D16) {
        h->d16_restart = true;
        g_err = "kfpos_slot_submit_rows: KFPOS_SLOT_RANGES_D16 belongs to whole-bank rounds (row lists stay int32)";
        return KFPOS_ERR_ARG;
    }
    Round r;
    int rc = submit_head(h, slot, flags, true, r);
    if (rc) return rc;
    auto &sl = h->slot[slot];
    const auto &so = h->so;
    if (flags & (KFPOS_SLOT_REUSE_ERR | KFPOS_SLOT_REUSE_COV)) {
        g_err = "kfpos_slot_submit_rows: KFPOS_SLOT_REUSE_* belongs to whole-bank rounds (a row-list round brings the listed tags' own values)";
        return KFPOS_ERR_ARG;
    }
    const bool pose_cov = (flags & KFPOS_SLOT_POSE_COV) != 0;
    if (pose_cov && (flags & KFPOS_SLOT_NO_POSE)) {
        g_err = "kfpos_slot_submit_rows: KFPOS_SLOT_POSE_COV with KFPOS_SLOT_NO_POSE (a round that returns what is published returns pos)";
        return KFPOS_ERR_ARG;
    }
    if (n > h->cfg.n_tags) {
        g_err = "kfpos_slot_submit_rows: n exceeds the slot's capacity (n_tags)";
        return KFPOS_ERR_ARG;
    }
    if ((rc = rows_check(h, "kfpos_slot_submit_rows", sl.rows, n))) return rc;
    sl.pose_round = false; /* until this round has enqueued its own (a round that enqueues nothing publishes nothing) */
    if (n == 0) return KFPOS_OK;
    if (r.answer == ROUND_EMPTY) {
        std::memset(sl.host + so.status, 0, sizeof(uint32_t) * n);
        return KFPOS_OK;
    }
    if (r.answer) return round_refusal(r.answer);
    const size_t cap = h->cfg.n_tags;
    if (pose_cov && !sl.pose_host) { /* first use of the flag in this slot */
        HIPCHK(hipHostMalloc((void **)sl.pose_host.out(), cap * 12 * sizeof(double), hipHostMallocDefault));
        HIPCHK(hipMalloc((void **)sl.pose_dev.out(), cap * 12 * sizeof(double)));
    }
    if ((rc = rows_reserve(h, (size_t)n))) return rc;
    const kfpos_layout::Rows L = rows_layout(h, (size_t)n);
    unsigned char *in = h->d_work + (size_t)slot * L.in_bytes; /* this slot's input area: its last round has completed */
    const size_t N = (size_t)n, A = h->cfg.max_anchors, m = h->msz;
    /* 1. the listed tags' records, pinned host -> device on the copy stream: bytes proportional to n. The slot's device
     * block is not touched: it may hold the errorEstimations / covariance a later whole-bank round reuses */
    auto up = [&](size_t i_off, const void *src, size_t bytes) {
        return hipMemcpyAsync(in + i_off, src, bytes, hipMemcpyHostToDevice, h->s_copy);
    };
    HIPCHK(up(L.i_rows, sl.rows, N * sizeof(int32_t)));
    if (r.has_rng) {
        HIPCHK(up(L.i_ranges, sl.host + so.ranges, N * A * sizeof(int32_t)));
        HIPCHK(up(L.i_err, sl.host + so.err, N * A * m));
    }
    if (r.has_imu) {
        HIPCHK(up(L.i_accel, sl.host + so.accel, N * 3 * m));
        HIPCHK(up(L.i_cov, sl.host + so.cov, N * 9 * m));
    }
    if (flags & KFPOS_SLOT_DT_PER_TAG) HIPCHK(up(L.i_dt, sl.host + so.dt, N * sizeof(double)));
    HIPCHK(hipEventRecord(sl.copied, h->s_copy));
    /* 2. turn, gather, step, scatter on the compute stream, in submission order with the whole-bank rounds */
    HIPCHK(hipStreamWaitEvent(h->s_comp, sl.copied, 0));
    auto turn = [&](size_t i_off, size_t w_off, int Cc, size_t esz) -> const void * {
        kfpos_k::launch_rows_to_cols(esz, h->s_comp, in + i_off, h->d_work + w_off, n, Cc);
        return h->d_work + w_off;
    };
    RoundIn d = {};
    if (r.has_rng) {
        d.ranges = (const int32_t *)turn(L.i_ranges, L.w_ranges, (int)A, sizeof(int32_t));
        d.err = turn(L.i_err, L.w_err, (int)A, m);
    }
    if (r.has_imu) {
        d.accel = turn(L.i_accel, L.w_accel, 3, m);
        d.cov = turn(L.i_cov, L.w_cov, 9, m);
    }
    HIPCHK(hipGetLastError());
    const bool want_pose = !(flags & KFPOS_SLOT_NO_POSE);
    KArgs a;
    round_args(h, r, d, (flags & KFPOS_SLOT_DT_PER_TAG) ? (const double *)(in + L.i_dt) : nullptr, dt_shared,
               (uint32_t *)(in + L.i_status), want_pose ? (double *)(in + L.i_pos) : nullptr, a);
    if ((rc = rows_step(h, h->s_comp, L, (const int32_t *)(in + L.i_rows), n, a))) return rc;
    if (pose_cov) { /* what is published for the round's tags: getPose at timeLag 0 of the bank the scatter just wrote */
        kfpos_k::PoseRowsArgs g = {};
        pose_bank_args(h, g.p);
        g.p.cov = sl.pose_dev;
        g.p.vel = sl.pose_dev + cap * 9;
        g.rows = (const int32_t *)(in + L.i_rows);
        g.n = n;
        kfpos_k::launch_get_pose_rows(h->cfg.model, h->full != 0, h->cfg.storage, h->s_comp, g);
        HIPCHK(hipGetLastError());
    }
    /* 3. status [n] and pos [3][n] back; cov3x3 [n][9], vel [n][3] behind them */
    rc = submit_return(h, sl, [&]() -> int {
        HIPCHK(hipMemcpyAsync(sl.host + so.status, in + L.i_status, N * sizeof(uint32_t), hipMemcpyDeviceToHost, h->s_back));
        if (want_pose) HIPCHK(hipMemcpyAsync(sl.host + so.pos, in + L.i_pos, N * 3 * sizeof(double), hipMemcpyDeviceToHost, h->s_back));
        if (pose_cov) {
            HIPCHK(hipMemcpyAsync(sl.pose_host, sl.pose_dev, N * 9 * sizeof(double), hipMemcpyDeviceToHost, h->s_back));
            HIPCHK(hipMemcpyAsync(sl.pose_host + cap * 9, sl.pose_dev + cap * 9, N * 3 * sizeof(double), hipMemcpyDeviceToHost, h->s_back));
        }
        return KFPOS_OK;
    });
    if (rc == KFPOS_OK) sl.pose_round = pose_cov;
    return rc;
}

int kfpos_slot_pose_rows(kfpos_handle *h, int32_t slot, double **cov3x3, double **vel) {
    g_err.clear();
    if (!h || slot < 0 || slot >= KFPOS_N_SLOTS) return KFPOS_ERR_ARG;
    const auto &sl = h->slot[slot];
    if (!sl.pose_round) {
        g_err = "kfpos_slot_pose_rows: the slot's last row-list round did not carry KFPOS_SLOT_POSE_COV";
        return KFPOS_ERR_STATE;
    }
    if (cov3x3) *cov3x3 = sl.pose_host;
    if (vel) *vel = sl.pose_host + (size_t)h->cfg.n_tags * 9;
    return KFPOS_OK;
}

} // extern "C"
