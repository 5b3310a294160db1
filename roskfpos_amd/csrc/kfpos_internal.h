/*
 * kfpos_internal.h -- what the host translation units of libkfpos_hip.so (kfpos_hip*.hip through kfpos_host.h, and
 * kfpos_comm.hip) share and the ABI does not show: the handle. No kernel unit sees it. The list of units: kfpos_kargs.h.
 */
#ifndef KFPOS_INTERNAL_H
#define KFPOS_INTERNAL_H

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/kfpos.h"
#include "kfpos_host_layout.h"
#include "kfpos_owned.h"
#include "kfpos_policy.h"

#define KFPOS_N_SLOTS 3      /* streaming host API: one slot being filled, one on the bus, one computing / returning */

/* thread-local text behind kfpos_last_error() */
__attribute__((visibility("hidden"))) std::string &kfpos_error_text();

/* Every entry point runs on its handle's device whatever the calling thread's current device is (a process that
 * drives one handle per GPU from one thread: kfpos_comm_create_all), and leaves the caller's device as it found it. */
struct KfposDevScope {
    int prev = -1;
    bool switched = false;
    explicit KfposDevScope(int dev) {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~KfposDevScope() {
        if (switched) (void)hipSetDevice(prev);
    }
    KfposDevScope(const KfposDevScope &) = delete;
    KfposDevScope &operator=(const KfposDevScope &) = delete;
};

/* What the handle and the communicator own gives itself back when they are deleted: nothing else frees anything. A raw
 * pointer, event or stream beside these points into a block or names somebody else's, and says so. */
template <class T> using DevPtr = kfpos_owned::Owned<T *, hipFree>;
template <class T> using PinnedPtr = kfpos_owned::Owned<T *, hipHostFree>;
using Event = kfpos_owned::Owned<hipEvent_t, hipEventDestroy>;
using Stream = kfpos_owned::Owned<hipStream_t, hipStreamDestroy>;

struct kfpos_handle {
    kfpos_config cfg;
    int n;        /* state dimension */
    int full;     /* COV_FULL layout: 6-state with ML initialisation (non-symmetric P) */
    int psz;      /* stored covariance entries per tag */
    int rsz;      /* bytes per stored covariance entry */
    int msz;      /* sizeof(kfpos_real): bytes per measurement element */
    int A;        /* anchors set */
    bool have_anchors, stepped;
    kfpos_policy::Policy policy; /* kfpos_create's choices (kfpos_policy.h), fixed from then on but for policy.coop */
    double anchors[KFPOS_MAX_ANCHORS * 3];
    /* anchor cells (kfpos_set_anchor_cells): n_cells > 0 = every block of KFPOS_CELL_TAGS rows ranges against the table
     * of its cell, and ranging rounds run the cells kernels (kfpos_k_cells*.hip). d_cell_xyz: [n_cells][max_anchors][3],
     * zeros behind the A rows set (room for cell_cap cells); d_cell_of_block: [(n_tags + 63) / 64], validated by the host.
     * Both stay allocated when kfpos_set_anchors returns the handle to one table (n_cells = 0). */
    int n_cells = 0;
    size_t cell_cap = 0;
    DevPtr<double> d_cell_xyz;
    DevPtr<int32_t> d_cell_of_block;
    /* device state */
    DevPtr<double> d_pos, d_vel;
    DevPtr<void> d_P, d_imu_acc, d_imu_cov;
    DevPtr<uint32_t> d_flags;
    /* staging for the host-buffer API */
    DevPtr<int32_t> d_ranges;
    DevPtr<void> d_err, d_accel, d_cov;
    DevPtr<double> d_dt, d_out; /* d_out: [15][T] doubles for pose results */
    DevPtr<uint32_t> d_status;
    Event ev0, ev1;
    /* planar filter */
    kfpos_planar_config planar = {};
    bool planar_sensors = false; /* a PX4Flow / IMU / magnetometer / compass sample has been fed: latches are live */
    DevPtr<double> d_latch;      /* [15][T] */
    DevPtr<double> d_sensor;     /* [24][T] staging of one sensor sample */
    /* row-major staging area of the host-buffer API: one region per array of a call (bump-allocated) */
    DevPtr<unsigned char> d_stage;
    size_t stage_cap = 0, stage_used = 0;
    /* small banks (the single-tag adaptor objects, test banks): ONE host-pinned, device-mapped block holds every
     * input and output of a host-API call in component-major form; the kernels read and write it in place over the
     * bus, so a call is "turn the layout on the CPU, launch, synchronise" -- no hipMemcpy, no layout kernels */
    PinnedPtr<unsigned char> sm_h;
    unsigned char *sm_d = nullptr; /* sm_h as the device sees it: not owning */
    kfpos_layout::Mapped sm = {}; /* sm.bytes, the whole block: nothing in it outlives a call, so the per-tag accessors stage through all of it */
    /* streaming host API: KFPOS_N_SLOTS slots of pinned host + device buffers, three streams (kfpos_slot_*) */
    struct Slot {
        PinnedPtr<unsigned char> host; /* pinned block: ranges | err | accel | cov | dt | status | pos */
        DevPtr<unsigned char> dev;     /* device block, same layout */
        Event copied, copied2, computed, done;
        /* `computed` of the last submission (of ANY slot) whose kernel read this slot's device errorEstimations /
         * sensor covariance: an upload into those regions waits for it, whichever slot holds the current ones by then
         * (some slot's `computed`: not owning) */
        hipEvent_t err_reader = nullptr, cov_reader = nullptr;
        bool busy = false;
        PinnedPtr<int32_t> rows; /* pinned [n_tags]: the row list of a row-list round (kfpos_slot_acquire_rows) */
        /* KFPOS_SLOT_POSE_COV, allocated by the first round that carries it: cov3x3 [n][9] at 0 and vel [n][3] at
         * 9 * n_tags doubles, pinned and on the device; pose_round: the slot's last row-list round filled them */
        PinnedPtr<double> pose_host;
        DevPtr<double> pose_dev;
        bool pose_round = false;
        /* KFPOS_SLOT_RANGES_D16, allocated by the handle's first kfpos_slot_delta: code | esc (kfpos_layout::Delta),
         * pinned and on the device; n_esc: what kfpos_delta_slot::n_esc points at */
        PinnedPtr<unsigned char> d16_host;
        DevPtr<unsigned char> d16_dev;
        int32_t n_esc = 0;
    } slot[KFPOS_N_SLOTS];
    /* the base of the D16 rounds: host mirror and device copy [max_anchors][n_tags]; d16_open: the slot kfpos_slot_delta
     * opened, or -1; d16_restart: the next kfpos_slot_delta zeroes both sides first */
    std::vector<int32_t> d16_mirror;
    DevPtr<int32_t> d16_base;
    kfpos_layout::Delta d16 = {};
    int d16_open = -1;
    bool d16_restart = false;
    kfpos_layout::Slot so = {};
    Stream s_copy, s_copy2, s_comp, s_back;
    int err_slot = -1, cov_slot = -1;                  /* which slot's device block holds the current err / cov */
    /* row-list steps (kfpos_step_*_rows, kfpos_slot_submit_rows): one device block, allocated on first use, grown to the
     * largest n seen (never beyond n_tags): KFPOS_N_SLOTS input areas -- what a round uploads (rows, row-major inputs,
     * dt) and returns (status, pos); fixed places, since the copy stream runs ahead of the compute stream -- followed by
     * the work bank: the listed tags' state and the turned inputs at stride n, used on one stream in submission order */
    DevPtr<unsigned char> d_work;
    size_t work_cap = 0;                               /* listed tags it holds */
    std::vector<uint32_t> row_stamp;                   /* [n_tags] host: the call that last listed a row (duplicate check in O(n)) */
    uint32_t stamp = 0;
};

#endif /* KFPOS_INTERNAL_H */
