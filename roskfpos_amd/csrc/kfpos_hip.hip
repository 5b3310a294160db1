/*
 * kfpos_hip.hip -- host side of libkfpos_hip.so: the handle, the step launch (a Plan of kfpos_launch_plan.h as a kernel,
 * its grid and its LDS bytes: launch selection itself lives there), two of the three ways in
 * (synchronous host-buffer API, device-buffer API) and the C ABI of include/kfpos.h. The kernels live in
 * kfpos_k_*.hip (kfpos_kargs.h says which is where); the state side of the ABI (whole-bank accessors, per-tag lifecycle,
 * pose for a row list) in kfpos_hip_state.hip; the streaming slots in kfpos_hip_slots.hip; the replay entry points
 * (kfpos_run_*_dev: whole schedules in few launches) in kfpos_hip_replay.hip; the RCCL pose gather in kfpos_comm.hip.
 */
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "kfpos_host.h"
#include "kfpos_core.h" /* the per-tag arithmetic's own constants: iekf9_next_meet, ST_* */
using namespace kfpos;

std::string &kfpos_error_text() {
    thread_local std::string text;
    return text;
}

/* ------------------------------------------------------------------ host side */
void fill_args(const kfpos_handle *h, KArgs &a) {
    std::memcpy(a.anchors, h->anchors, sizeof(a.anchors));
    a.T = h->cfg.n_tags;
    a.A = h->have_anchors ? h->A : 0; /* anchors set (<= max_anchors): columns beyond them do not exist */
    a.accel_noise = h->cfg.accel_noise;
    a.jolt = h->cfg.jolt;
    a.cost_threshold = h->cfg.cost_threshold;
    a.ignore_worst = h->cfg.ignore_worst;
    a.top_n = h->cfg.top_n;
    a.ml_variant = h->cfg.model == KFPOS_MODEL_ML ? h->cfg.ml_variant : 0;
    a.pair9 = h->policy.pair9 ? 1 : 0;
    a.pair9_first = (short)h->policy.pair9_first;
    a.pair9_dense_until = (short)h->policy.pair9_dense_until;
    a.imu9_diag = h->policy.imu9_diag ? 1 : 0;
    a.use_init_pos = h->cfg.use_init_pos;
    a.use_fixed_height = h->planar.use_fixed_height;
    a.imu_fixed_cov_acc = h->planar.imu_use_fixed_cov_acc;
    a.imu_fixed_cov_w = h->planar.imu_use_fixed_cov_ang_vel_z;
    a.px4_height = h->planar.px4_height;
    a.px4_arm_p1 = h->planar.px4_arm_p1;
    a.px4_arm_p2 = h->planar.px4_arm_p2;
    a.px4_cov_vel = h->planar.px4_cov_velocity;
    a.px4_cov_gyro_z = h->planar.px4_cov_gyro_z;
    a.imu_cov_acc = h->planar.imu_cov_acc;
    a.imu_cov_w = h->planar.imu_cov_ang_vel_z;
    a.mag_offset = h->planar.mag_angle_offset;
    a.mag_cov = h->planar.mag_cov;
    a.platch = h->d_latch;
    a.sensor = nullptr;
    a.pos = h->d_pos;
    a.vel = h->d_vel;
    a.P = h->d_P;
    a.flags = h->d_flags;
    a.imu_acc = h->d_imu_acc;
    a.imu_cov = h->d_imu_cov;
    a.ranges = nullptr;
    a.err = nullptr;
    a.dt = nullptr;
    a.dt_shared = 0.0;
    a.accel = nullptr;
    a.cov = nullptr;
    a.mode = MODE_TOA;
    a.latch = 1;
    a.status = nullptr;
    a.n_steps = 1;
    a.stride_ranges = a.stride_err = a.stride_accel = a.stride_cov = 0;
    a.traj = nullptr;
}

namespace {

/* a step plan (kfpos_launch_plan.h) as the kernel it names: the covariance layout says which unit's selector is asked */
step_kernel_t step_kernel(const kfpos_handle *h, const kfpos_plan::Plan &p) {
    const int st = h->cfg.storage;
    if (h->cfg.model == KFPOS_MODEL_PLANAR) return kfpos_k::planar_kernel(st, p.sensors, p.as);
    if (h->cfg.model == KFPOS_MODEL_ML) return kfpos_k::ml_kernel(st, p.as);
    if (h->cfg.model == KFPOS_MODEL_TOA_IMU) return kfpos_k::imu9_kernel(st, p.as, p.ranging);
    if (h->policy.coop) return kfpos_k::toa6_coop_kernel(st);
    return h->full ? kfpos_k::toa6_full_kernel(st, p.as, p.heur) : kfpos_k::toa6_sym_kernel(st, p.as, p.heur, p.two_waves);
}


/* ---- anchor cells: the ranging round of a handle with cells (kfpos_set_anchor_cells) ----
 * The plan of the same handle without the 8-lanes-per-tag kernel and without the two-wavefront build: the cells kernels
 * are the one-tag-per-lane, one-wavefront forms (kfpos_launch_plan.h is not told about cells) */
kfpos_plan::Plan cells_plan(const kfpos_handle *h) {
    kfpos_plan::Inputs in = plan_inputs(h);
    in.coop = false;
    in.two_waves = false;
    return kfpos_plan::plan(in, kfpos_plan::STEP_RANGING);
}
kfpos_k::cells_kernel_t cells_kernel(const kfpos_handle *h, const kfpos_plan::Plan &p) {
    const int st = h->cfg.storage;
    if (h->cfg.model == KFPOS_MODEL_TOA_IMU) return kfpos_k::cells_imu9_kernel(st, p.as);
    return h->full ? kfpos_k::cells_toa6_full_kernel(st, p.as, p.heur) : kfpos_k::cells_toa6_sym_kernel(st, p.as, p.heur);
}
int launch_cells(kfpos_handle *h, const KArgs &a, hipStream_t s) {
    if (a.T != h->cfg.n_tags) { /* (every row-list call refuses a handle with cells before it gets here) */
        g_err = "a handle with anchor cells steps the whole bank only";
        return KFPOS_ERR_STATE;
    }
    const kfpos_plan::Plan p = cells_plan(h);
    kfpos_k::CellArgs c;
    static_cast<KArgs &>(c) = a;
    c.cell_xyz = h->d_cell_xyz;
    c.cell_of_block = h->d_cell_of_block;
    c.cell_stride = 3 * h->cfg.max_anchors;
    hipLaunchKernelGGL(cells_kernel(h, p), dim3(p.groups(a.T)), dim3(WAVE), p.bytes(), s, c);
    HIPCHK(hipGetLastError());
    h->stepped = true;
    return KFPOS_OK;
}

} // namespace

int cells_refusal(const char *who, const char *why) {
    g_err = std::string(who) + " is not defined for a handle with anchor cells (kfpos_set_anchor_cells): " + why;
    return KFPOS_ERR_MODEL;
}

/* a.T tags: the whole bank, or the n tags of a work bank (row-list steps). WHICH kernel runs is a property of the handle
 * and of what the call feeds (a planar bank's a.mode is 0 or the sensor kind), never of a.T -- the plan is not told it: a
 * row-list step computes bit for bit what the whole-bank call does */
int launch_step(kfpos_handle *h, const KArgs &a, hipStream_t s) {
    if (h->n_cells > 0 && a.mode != MODE_IMU_ONLY) return launch_cells(h, a, s);
    const bool planar = h->cfg.model == KFPOS_MODEL_PLANAR;
    const kfpos_plan::Plan p = kfpos_plan::plan(plan_inputs(h), planar ? (a.mode != 0 ? kfpos_plan::STEP_SENSOR : kfpos_plan::STEP_RANGING)
                                                                       : (a.mode == MODE_IMU_ONLY ? kfpos_plan::STEP_IMU_ONLY : kfpos_plan::STEP_RANGING));
    hipLaunchKernelGGL(step_kernel(h, p), dim3(p.groups(a.T)), dim3(WAVE), p.bytes(), s, a);
    HIPCHK(hipGetLastError());
    h->stepped = true;
    return KFPOS_OK;
}

/* ---- staging and the route of a host-buffer call: Route, kfpos_kernels.h says what each does ---- */
int stage_region(kfpos_handle *h, size_t bytes, void **out) {
    bytes = (bytes + 255) & ~(size_t)255;
    if (h->stage_used + bytes > h->stage_cap) {
        /* grow: everything queued so far still reads the old buffer, so drain first */
        HIPCHK(hipDeviceSynchronize());
        const size_t cap = (h->stage_used + bytes) * 2;
        DevPtr<unsigned char> nb;
        HIPCHK(hipMalloc((void **)nb.out(), cap));
        h->d_stage = std::move(nb);
        h->stage_cap = cap;
        h->stage_used = 0; /* regions handed out before the growth have been consumed (synchronised above) */
    }
    *out = h->d_stage + h->stage_used;
    h->stage_used += bytes;
    return KFPOS_OK;
}
int stage_in(kfpos_handle *h, void *dst, const void *src, size_t n, int C, size_t esz, void *landing) {
    if (C == 1) {
        HIPCHK(hipMemcpy(dst, src, n * esz, hipMemcpyHostToDevice));
        return KFPOS_OK;
    }
    const int rc = landing ? KFPOS_OK : stage_region(h, n * C * esz, &landing);
    if (rc) return rc;
    HIPCHK(hipMemcpy(landing, src, n * C * esz, hipMemcpyHostToDevice));
    kfpos_k::launch_rows_to_cols(esz, nullptr, landing, dst, (int)n, C);
    HIPCHK(hipGetLastError());
    return KFPOS_OK;
}
int stage_out(kfpos_handle *h, double *dst, const double *dsrc, size_t n, int C) {
    if (C == 1) {
        HIPCHK(hipMemcpy(dst, dsrc, n * sizeof(double), hipMemcpyDeviceToHost));
        return KFPOS_OK;
    }
    void *rows = nullptr;
    const int rc = stage_region(h, n * C * sizeof(double), &rows);
    if (rc) return rc;
    kfpos_k::launch_cols_to_rows(nullptr, dsrc, (double *)rows, (int)n, C);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpy(dst, rows, n * C * sizeof(double), hipMemcpyDeviceToHost));
    return KFPOS_OK;
}
Route route_of(kfpos_handle *h) {
    if (!h->sm_h) stage_reset(h);
    return Route{h, h->sm_h, h->sm_h ? h->sm_d : nullptr, 0};
}

namespace {

static_assert(kfpos_policy::TRACE_CHUNK_MAX == KFPOS_TRACE_CHUNK, "Policy::trace_chunk: what the argument blocks hold");

/* kfpos_create, third part: everything the bank owns from its first call on (the rest comes with its first use), zeroed */
int bank_allocate(kfpos_handle *h) {
    const size_t T = h->cfg.n_tags, A = h->cfg.max_anchors, r = h->rsz, m = h->msz;
#define ALLOC(ptr, bytes)                                                     \
    do {                                                                      \
        hipError_t e_ = hipMalloc((void **)(ptr).out(), (bytes));             \
        if (e_ != hipSuccess) {                                               \
            g_err = std::string("hipMalloc: ") + hipGetErrorString(e_);       \
            return KFPOS_ERR_HIP;                                             \
        }                                                                     \
        (void)hipMemset((ptr), 0, (bytes));                                   \
    } while (0)
    ALLOC(h->d_pos, 3 * T * sizeof(double));
    ALLOC(h->d_P, h->psz * T * r);
    ALLOC(h->d_flags, T * sizeof(uint32_t));
    if (h->n == 3) ALLOC(h->d_vel, 3 * T * sizeof(double)); /* ALGORITHM_ML: the solver's per-tag seed */
    if (h->n == 8) {
        ALLOC(h->d_vel, 4 * T * sizeof(double)); /* vx, vy, theta, omega */
        ALLOC(h->d_latch, LATCH_ROWS * T * sizeof(double));
        ALLOC(h->d_sensor, 24 * T * sizeof(double));
    }
    if (h->n == 9) {
        ALLOC(h->d_vel, 3 * T * sizeof(double));
        ALLOC(h->d_imu_acc, 3 * T * m);
        ALLOC(h->d_imu_cov, 6 * T * m);
        ALLOC(h->d_accel, 3 * T * m);
        ALLOC(h->d_cov, 9 * T * m);
    }
    ALLOC(h->d_ranges, A * T * sizeof(int32_t));
    ALLOC(h->d_err, A * T * m);
    ALLOC(h->d_dt, T * sizeof(double));
    ALLOC(h->d_out, 15 * T * sizeof(double));
    ALLOC(h->d_status, T * sizeof(uint32_t));
#undef ALLOC
    if (hipEventCreate(h->ev0.out()) != hipSuccess || hipEventCreate(h->ev1.out()) != hipSuccess) {
        g_err = "hipEventCreate failed";
        return KFPOS_ERR_HIP;
    }
    if (T * A <= h->policy.small_bank_elems) { /* small bank: one mapped block instead of staging copies (kfpos_handle::sm_*) */
        h->sm = kfpos_layout::mapped_layout(handle_sizes(h));
        void *dp = nullptr;
        if (hipHostMalloc((void **)h->sm_h.out(), h->sm.bytes, hipHostMallocMapped) != hipSuccess ||
            hipHostGetDevicePointer(&dp, h->sm_h, 0) != hipSuccess) {
            g_err = "hipHostMalloc(mapped block of a small bank) failed";
            return KFPOS_ERR_HIP;
        }
        std::memset(h->sm_h, 0, h->sm.bytes);
        h->sm_d = (unsigned char *)dp;
    }
    return KFPOS_OK;
}

/* ... and fourth: the kernels' LDS allowance and the bank's initial position */
int bank_seed(kfpos_handle *h) {
    /* every step launch this handle can ever make -- ranging, IMU-only, sensor call, ranging after a sensor sample --:
     * a kernel whose plan takes more than 64 KB of LDS is allowed them here, once */
    const kfpos_plan::Launch may[4] = {kfpos_plan::STEP_RANGING, kfpos_plan::STEP_IMU_ONLY, kfpos_plan::STEP_SENSOR, kfpos_plan::STEP_RANGING};
    for (int k = 0; k < 4; ++k) {
        kfpos_plan::Inputs in = plan_inputs(h);
        in.planar_sensors = k == 3;
        const kfpos_plan::Plan p = kfpos_plan::plan(in, may[k]);
        if (p.bytes() <= 64 * 1024) continue;
        hipError_t e_ = hipFuncSetAttribute((const void *)step_kernel(h, p), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bytes());
        if (e_ != hipSuccess) {
            g_err = std::string("hipFuncSetAttribute: ") + hipGetErrorString(e_);
            return KFPOS_ERR_HIP;
        }
    }
    /* initial position: fixed start (P0 = 0) or NaN until the ML initialisation */
    const size_t T = h->cfg.n_tags;
    std::vector<double> p0(3 * T);
    for (size_t t = 0; t < T; ++t)
        for (int k = 0; k < 3; ++k) {
            p0[(size_t)k * T + t] = h->cfg.use_init_pos ? h->cfg.init_pos[k] : NAN;
            if (h->n == 8 && k == 2) p0[(size_t)k * T + t] = 0.0; /* mUWBtagZ: kfpos_set_planar, not initialPosition.z */
        }
    if (h->n == 3 && hipMemcpy(h->d_vel, p0.data(), p0.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        g_err = "hipMemcpy(ml seed) failed";
        return KFPOS_ERR_HIP;
    }
    if (hipMemcpy(h->d_pos, p0.data(), p0.size() * sizeof(double), hipMemcpyHostToDevice) != hipSuccess) {
        g_err = "hipMemcpy(init pos) failed";
        return KFPOS_ERR_HIP;
    }
    return KFPOS_OK;
}
} // namespace

extern "C" {

const char *kfpos_last_error(void) { return g_err.c_str(); }
const char *kfpos_strerror(int code) {
    switch (code) {
    case KFPOS_OK: return "ok";
    case KFPOS_ERR_ARG: return "invalid argument";
    case KFPOS_ERR_HIP: return "HIP runtime error";
    case KFPOS_ERR_NO_DEVICE: return "no usable GPU";
    case KFPOS_ERR_MODEL: return "call not defined for this model";
    case KFPOS_ERR_STATE: return "call out of sequence";
    case KFPOS_ERR_COMM: return "RCCL error";
    default: return "unknown error";
    }
}
int kfpos_version(void) { return KFPOS_VERSION; }
int kfpos_pair9_meet_points(int32_t first, int32_t dense_until, int32_t *out) {
    using kfpos_policy::PAIR9_MEET_MAX;
    if (!out || !kfpos_policy::pair9_meet_ok(first, dense_until)) return -1;
    int n = 0;
    int stop = first;
    for (;;) { /* as iekf9_info walks it with max_steps = 20 */
        out[n++] = stop;
        if (stop >= PAIR9_MEET_MAX) return n;
        stop = iekf9_next_meet(stop, dense_until, PAIR9_MEET_MAX);
    }
}

/* validate, decide (both kfpos_policy.h), allocate, seed. Answers in this order: a null argument, a configuration refusal,
 * a KFPOS_PAIR9_MEET refusal, KFPOS_ERR_NO_DEVICE, allocation */
int kfpos_create(const kfpos_config *cfg, kfpos_handle **out) {
    if (!cfg || !out) return KFPOS_ERR_ARG;
    *out = nullptr;
    g_err.clear();
    auto bad = [](const char *why) {
        g_err = why;
        return KFPOS_ERR_ARG;
    };
    if (const char *why = kfpos_policy::config_refusal(*cfg)) return bad(why);
    int ndev = 0;
    const bool have_dev = hipGetDeviceCount(&ndev) == hipSuccess && ndev > 0 && cfg->device >= 0 && cfg->device < ndev;
    hipDeviceProp_t prop;
    const size_t wave_slots = have_dev && hipGetDeviceProperties(&prop, cfg->device) == hipSuccess ? (size_t)prop.multiProcessorCount * 4 : 0;
    kfpos_policy::Policy policy; /* every KFPOS_* variable of the handle is read here, once */
    if (!kfpos_policy::policy(*cfg, wave_slots, [](const char *name) -> const char * { return getenv(name); }, &policy))
        return bad(kfpos_policy::PAIR9_MEET_REFUSAL);
    if (!have_dev) {
        g_err = "no HIP device";
        return KFPOS_ERR_NO_DEVICE;
    }
    DevScope dev_(cfg->device); /* the caller's current device is left as it was */
    kfpos_handle *h = new (std::nothrow) kfpos_handle();
    if (!h) return KFPOS_ERR_ARG;
    h->cfg = *cfg;
    h->policy = policy;
    h->n = cfg->model == KFPOS_MODEL_TOA_IMU ? 9 : (cfg->model == KFPOS_MODEL_ML ? 3 : (cfg->model == KFPOS_MODEL_PLANAR ? 8 : 6));
    h->full = kfpos_policy::full_layout(*cfg) ? 1 : 0;
    h->psz = h->full ? h->n * h->n : h->n * (h->n + 1) / 2;
    h->rsz = cfg->storage == KFPOS_STORE_F32 ? 4 : (cfg->storage == KFPOS_STORE_P48 ? 6 : 8);
    h->msz = cfg->storage == KFPOS_STORE_F64 ? 8 : 4;
    h->A = 0;
    h->have_anchors = false;
    h->stepped = false;
    std::memset(h->anchors, 0, sizeof(h->anchors));
    int rc = bank_allocate(h);
    if (rc == KFPOS_OK) rc = bank_seed(h);
    if (rc) { /* what it owns so far goes with it */
        kfpos_destroy(h);
        return rc;
    }
    *out = h;
    return KFPOS_OK;
}

int kfpos_destroy(kfpos_handle *h) {
    if (!h) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    (void)hipDeviceSynchronize(); /* nothing of this handle may still be in flight (streaming slots) */
    delete h; /* every member that owns something gives it back (kfpos_internal.h) */
    return KFPOS_OK;
}

int kfpos_init(kfpos_handle *h) { return h ? KFPOS_OK : KFPOS_ERR_ARG; }

int kfpos_set_anchors(kfpos_handle *h, const double *xyz, const int32_t *ids, int32_t n_anchors) {
    g_err.clear();
    (void)ids;
    if (!h || !xyz || n_anchors < 1 || n_anchors > h->cfg.max_anchors) return KFPOS_ERR_ARG;
    if (h->cfg.model == KFPOS_MODEL_ML && h->cfg.ml_variant == KFPOS_ML_BEST && n_anchors > 5) {
        g_err = "estimatePositionBestGroup has no defined result for more than 5 ranges: its erase loop removes by an index "
                "into the vector it is shrinking and runs past the end from the first group on (MLLocation.cpp:377-381)";
        return KFPOS_ERR_MODEL;
    }
    std::memset(h->anchors, 0, sizeof(h->anchors));
    std::memcpy(h->anchors, xyz, sizeof(double) * 3 * n_anchors);
    h->A = n_anchors;
    h->have_anchors = true;
    h->n_cells = 0; /* back to one table (a handle that left the 8-lanes-per-tag kernel for cells does not return to it) */
    return KFPOS_OK;
}

int kfpos_set_anchor_cells(kfpos_handle *h, int32_t n_cells, int32_t n_anchors, const double *xyz, const int32_t *cell_of_block) {
    g_err.clear();
    if (!h || !xyz || !cell_of_block || n_cells < 1 || n_anchors < 1 || n_anchors > h->cfg.max_anchors) return KFPOS_ERR_ARG;
    if (h->cfg.model != KFPOS_MODEL_TOA && h->cfg.model != KFPOS_MODEL_TOA_IMU) {
        g_err = "kfpos_set_anchor_cells: no cells kernel is built for KFPOS_MODEL_ML and KFPOS_MODEL_PLANAR";
        return KFPOS_ERR_MODEL;
    }
    const size_t n_blocks = ((size_t)h->cfg.n_tags + KFPOS_CELL_TAGS - 1) / KFPOS_CELL_TAGS;
    for (size_t b = 0; b < n_blocks; ++b)
        if (cell_of_block[b] < 0 || cell_of_block[b] >= n_cells) {
            g_err = "kfpos_set_anchor_cells: cell_of_block[" + std::to_string(b) + "] = " + std::to_string(cell_of_block[b]) +
                    " is outside [0, " + std::to_string(n_cells) + ")";
            return KFPOS_ERR_ARG;
        }
    if (h->policy.coop && h->stepped) {
        g_err = "kfpos_set_anchor_cells: this handle runs the 8-lanes-per-tag kernel, which sums in another order than the "
                "cells kernels, and has already stepped (call it before the first step, or create the handle under KFPOS_NO_COOP=1)";
        return KFPOS_ERR_STATE;
    }
    DevScope dev_(h->cfg.device);
    /* a configuration call: nothing that still reads the table in force may be in flight */
    const int rc = drain_slots(h);
    if (rc) return rc;
    HIPCHK(hipDeviceSynchronize());
    /* a cells kernel whose plan takes more than 64 KB of LDS is allowed it here, as kfpos_create allows the others theirs */
    const kfpos_plan::Plan p = cells_plan(h);
    if (p.bytes() > 64 * 1024)
        HIPCHK(hipFuncSetAttribute((const void *)cells_kernel(h, p), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bytes()));
    const size_t stride = 3 * (size_t)h->cfg.max_anchors;
    DevPtr<double> tab; /* both or neither: a table that grew replaces the old one once the map has its room too */
    if ((size_t)n_cells > h->cell_cap) HIPCHK(hipMalloc((void **)tab.out(), (size_t)n_cells * stride * sizeof(double)));
    if (!h->d_cell_of_block && hipMalloc((void **)h->d_cell_of_block.out(), n_blocks * sizeof(int32_t)) != hipSuccess) {
        g_err = "hipMalloc(cell_of_block) failed";
        return KFPOS_ERR_HIP;
    }
    if (tab) {
        h->d_cell_xyz = std::move(tab);
        h->cell_cap = (size_t)n_cells;
    }
    /* the table as the kernels read it: n_anchors rows per cell, zeros up to max_anchors */
    std::vector<double> padded((size_t)n_cells * stride, 0.0);
    for (size_t c = 0; c < (size_t)n_cells; ++c)
        std::memcpy(&padded[c * stride], xyz + c * 3 * (size_t)n_anchors, sizeof(double) * 3 * (size_t)n_anchors);
    HIPCHK(hipMemcpy(h->d_cell_xyz, padded.data(), padded.size() * sizeof(double), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->d_cell_of_block, cell_of_block, n_blocks * sizeof(int32_t), hipMemcpyHostToDevice));
    std::memset(h->anchors, 0, sizeof(h->anchors)); /* (KArgs::anchors: no kernel of a handle with cells reads it) */
    h->A = n_anchors;
    h->have_anchors = true;
    h->n_cells = n_cells;
    h->policy.coop = false; /* the one change of the policy after kfpos_create (not stepped, or never was: see above) */
    return KFPOS_OK;
}
int kfpos_anchor_cells(const kfpos_handle *h) { return h ? h->n_cells : 0; }

int kfpos_set_init_positions(kfpos_handle *h, const double *xyz) {
    g_err.clear();
    if (!h || !xyz) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    if (!h->cfg.use_init_pos || h->stepped) return KFPOS_ERR_STATE;
    stage_reset(h);
    if (h->n == 3) { /* ALGORITHM_ML: the seed of every solve */
        const int rc = stage_in(h, h->d_vel, xyz, h->cfg.n_tags, 3, sizeof(double));
        if (rc) return rc;
    }
    const int rc = stage_in(h, h->d_pos, xyz, h->cfg.n_tags, 3, sizeof(double));
    if (rc == KFPOS_OK && h->n == 8) { /* the filter works at mUWBtagZ, whatever initialPosition.z says */
        std::vector<double> z(h->cfg.n_tags, h->planar.fixed_height);
        HIPCHK(hipMemcpy(h->d_pos + 2 * (size_t)h->cfg.n_tags, z.data(), z.size() * sizeof(double), hipMemcpyHostToDevice));
    }
    return rc;
}

int kfpos_set_planar(kfpos_handle *h, const kfpos_planar_config *cfg) {
    g_err.clear();
    if (!h || !cfg) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    if (h->cfg.model != KFPOS_MODEL_PLANAR) return KFPOS_ERR_MODEL;
    if (h->stepped) return KFPOS_ERR_STATE;
    h->planar = *cfg;
    /* mUWBtagZ and mAngle of every tag: pos row 2, vel row 2 (angular speed, row 3, stays 0) */
    const size_t T = h->cfg.n_tags;
    std::vector<double> v(T, cfg->fixed_height);
    HIPCHK(hipMemcpy(h->d_pos + 2 * T, v.data(), T * sizeof(double), hipMemcpyHostToDevice));
    v.assign(T, cfg->init_angle);
    HIPCHK(hipMemcpy(h->d_vel + 2 * T, v.data(), T * sizeof(double), hipMemcpyHostToDevice));
    return KFPOS_OK;
}

int kfpos_real_size(const kfpos_handle *h) { return h ? h->msz : 0; }
int kfpos_state_dim(const kfpos_handle *h) { return h ? h->n : 0; }

/* ---- rounds: what a call feeds, and whether this handle takes it (kfpos_kernels.h: Round) ---- */
static_assert(ROUND_TOA == MODE_TOA && ROUND_IMU == MODE_IMU_ONLY && ROUND_FUSED == MODE_FUSED, "Round::mode = the kind");
static_assert(ROUND_TOA == KFPOS_SLOT_TOA && ROUND_IMU == KFPOS_SLOT_IMU && ROUND_FUSED == KFPOS_SLOT_TOA_IMU, "a slot's kind is a round kind");
extern "C++" Round round_check(const kfpos_handle *h, int kind, int32_t sensor_kind, bool slot) {
    static const int width[5] = {0, 5, 24, 3, 1}; /* KFPOS_SENSOR_PX4FLOW, _IMU, _MAG, _COMPASS */
    const bool sensor = kind == ROUND_SENSOR && !slot && sensor_kind >= 1 && sensor_kind <= 4;
    const bool imu9 = h->cfg.model == KFPOS_MODEL_TOA_IMU, planar = h->cfg.model == KFPOS_MODEL_PLANAR;
    Round r = {KFPOS_OK, kind == ROUND_TOA || kind == ROUND_FUSED, kind == ROUND_IMU || kind == ROUND_FUSED,
               sensor ? width[sensor_kind] : 0, sensor ? sensor_kind : kind};
    if (!sensor && kind != ROUND_TOA && kind != ROUND_IMU && kind != ROUND_FUSED) r.answer = KFPOS_ERR_ARG;
    else if (slot && planar && kind != ROUND_TOA) r.answer = KFPOS_ERR_MODEL; /* its sensors: kfpos_step_sensor / _rows */
    else if (kind == ROUND_FUSED && !imu9) r.answer = KFPOS_ERR_MODEL;
    /* the empty virtuals: KalmanFilterTOA::newIMUMeasurement, PositionEstimationAlgorithm.h:26-35 */
    else if ((kind == ROUND_IMU && !imu9) || (sensor && !planar)) r.answer = ROUND_EMPTY;
    else if (r.has_rng && !h->have_anchors) r.answer = KFPOS_ERR_STATE;
    return r;
}
extern "C++" int round_refusal(int answer) {
    if (answer == KFPOS_ERR_STATE)
        g_err = "kfpos_set_anchors has not been called (the node drops ranges until the anchors are known, Posgenerator.cpp:92-96)";
    return answer;
}
extern "C++" void round_args(const kfpos_handle *h, const Round &r, const RoundIn &in, const double *dt, double dt_shared,
                             uint32_t *status, double *traj, KArgs &a) {
    fill_args(h, a);
    if (r.has_rng) {
        a.ranges = in.ranges;
        a.err = in.err;
    }
    if (r.has_imu) {
        a.accel = in.accel;
        a.cov = in.cov;
    }
    if (r.width) a.sensor = in.sensor;
    a.mode = r.mode;
    a.dt = dt;
    a.dt_shared = dt_shared;
    a.status = status;
    a.traj = traj;
}

/* ---- device-buffer API: the caller has checked h and the pointers its kind carries ---- */
static int round_dev(kfpos_handle *h, int kind, int32_t sensor_kind, const RoundIn &in, int32_t latch, const double *dt,
                     double dt_shared, uint32_t *status, void *stream) {
    DevScope dev_(h->cfg.device);
    const Round r = round_check(h, kind, sensor_kind, false);
    if (r.answer == ROUND_EMPTY) { /* (an IMU sample leaves the caller's status words as they are) */
        if (status && r.width) HIPCHK(hipMemsetAsync(status, 0, sizeof(uint32_t) * h->cfg.n_tags, (hipStream_t)stream));
        return KFPOS_OK;
    }
    if (r.answer) return round_refusal(r.answer);
    KArgs a;
    round_args(h, r, in, dt, dt_shared, status, nullptr, a);
    a.latch = latch ? 1 : 0;
    const int rc = launch_step(h, a, (hipStream_t)stream);
    if (r.width) h->planar_sensors = true; /* ranging epochs now carry the latched samples */
    return rc;
}

int kfpos_step_toa_dev(kfpos_handle *h, const int32_t *range_mm, const void *err_est, const double *dt,
                       double dt_shared, uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || !range_mm || !err_est) return KFPOS_ERR_ARG;
    return round_dev(h, ROUND_TOA, 0, {range_mm, err_est, nullptr, nullptr, nullptr}, 1, dt, dt_shared, status, stream);
}

int kfpos_step_imu_dev(kfpos_handle *h, const void *accel, const void *cov, const double *dt,
                       double dt_shared, uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || !accel || !cov) return KFPOS_ERR_ARG;
    return round_dev(h, ROUND_IMU, 0, {nullptr, nullptr, accel, cov, nullptr}, 1, dt, dt_shared, status, stream);
}

int kfpos_step_sensor_dev(kfpos_handle *h, int32_t kind, const double *data, const double *dt, double dt_shared,
                          uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || !data) return KFPOS_ERR_ARG;
    return round_dev(h, ROUND_SENSOR, kind, {nullptr, nullptr, nullptr, nullptr, data}, 1, dt, dt_shared, status, stream);
}

int kfpos_step_toa_imu_dev(kfpos_handle *h, const int32_t *range_mm, const void *err_est, const void *accel,
                           const void *cov, int32_t latch, const double *dt, double dt_shared,
                           uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || !range_mm || !err_est || !accel || !cov) return KFPOS_ERR_ARG;
    return round_dev(h, ROUND_FUSED, 0, {range_mm, err_est, accel, cov, nullptr}, latch, dt, dt_shared, status, stream);
}

/* the bank as the pose kernels read it; outputs and extrapolation times: null / 0 until the caller sets them */
extern "C++" void pose_bank_args(const kfpos_handle *h, PoseArgs &a) {
    std::memset(&a, 0, sizeof(a));
    a.T = h->cfg.n_tags;
    a.model = h->cfg.model;
    a.full = h->full;
    a.accel_noise = h->cfg.accel_noise;
    a.jolt = h->cfg.jolt;
    a.pos_in = h->d_pos;
    a.vel_in = h->d_vel;
    a.P = h->d_P;
    a.flags = h->d_flags;
}

static int launch_pose(kfpos_handle *h, double dt_ahead, const double *dt_each, double *pos, double *cov3x3,
                       double *vel, uint32_t *status, void *stream, double *full_x = nullptr,
                       double *full_P = nullptr) {
    if (!h) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    PoseArgs a;
    pose_bank_args(h, a);
    a.dt_each = dt_each;
    a.full_x = full_x;
    a.full_P = full_P;
    a.dt_ahead = dt_ahead;
    a.pos = pos;
    a.cov = cov3x3;
    a.vel = vel;
    a.status = status;
    kfpos_k::launch_get_pose(h->cfg.model, h->full != 0, h->cfg.storage, (a.T + WAVE - 1) / WAVE, (hipStream_t)stream, a);
    HIPCHK(hipGetLastError());
    return KFPOS_OK;
}

int kfpos_get_pose_dev(kfpos_handle *h, double dt_ahead, double *pos, double *cov3x3, double *vel,
                       uint32_t *status, void *stream) {
    g_err.clear();
    return launch_pose(h, dt_ahead, nullptr, pos, cov3x3, vel, status, stream);
}

/* ---- host-buffer API ---- */
/* Every synchronous step call, whole-bank (listed = false: n_tags tags) or for a row list: what the round may feed, the
 * inputs through the call's route to where the step reads them -- the bank's staging arrays, or the work block's input
 * area 0 and work bank (the slots have been drained) --, the step, the status words back. */
static int round_host(kfpos_handle *h, const char *who, int kind, int32_t sensor_kind, bool listed, const int32_t *rows,
                      int32_t n, const RoundIn &src, const double *dt, int32_t dt_len, uint32_t *status) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    if (listed && h->n_cells > 0) return cells_refusal(who, CELLS_NO_ROWS);
    const Round r = round_check(h, kind, sensor_kind, false);
    if (r.answer == KFPOS_ERR_ARG) return KFPOS_ERR_ARG;
    int rc = listed ? rows_check(h, who, rows, n) : KFPOS_OK;
    if (rc) return rc;
    if (!listed) n = h->cfg.n_tags;
    if (n == 0) return KFPOS_OK;
    if ((r.has_rng && (!src.ranges || !src.err)) || (r.has_imu && (!src.accel || !src.cov)) || (r.width && !src.sensor)) return KFPOS_ERR_ARG;
    if (r.answer == ROUND_EMPTY) {
        if (status) std::memset(status, 0, sizeof(uint32_t) * n);
        return KFPOS_OK;
    }
    if (r.answer) return round_refusal(r.answer);
    DevScope dev_(h->cfg.device);
    if ((rc = drain_slots(h))) return rc;
    if (!dt || (dt_len != 1 && dt_len != n)) return KFPOS_ERR_ARG;
    if (listed && (rc = rows_reserve(h, (size_t)n))) return rc;
    const kfpos_layout::Rows L = listed ? rows_layout(h, (size_t)n) : kfpos_layout::Rows{};
    auto place = [&](size_t mapped, void *bank, size_t w_off, size_t i_off) {
        return listed ? Place{mapped, h->d_work + w_off, h->d_work + i_off} : Place{mapped, bank, nullptr};
    };
    const size_t N = (size_t)n, m = h->msz;
    const int A = h->cfg.max_anchors;
    const Place p_rows = {h->sm.out, h->d_work + L.i_rows, nullptr}; /* mapped: the pose-output region, free during a step */
    const Place p_dt = place(h->sm.dt, h->d_dt, L.i_dt, 0), p_status = place(h->sm.status, h->d_status, L.i_status, 0);
    const Place p_ranges = place(h->sm.ranges, h->d_ranges, L.w_ranges, L.i_ranges), p_err = place(h->sm.err, h->d_err, L.w_err, L.i_err);
    const Place p_accel = place(h->sm.accel, h->d_accel, L.w_accel, L.i_accel), p_cov = place(h->sm.cov, h->d_cov, L.w_cov, L.i_cov);
    const Place p_sensor = place(h->sm.sensor, h->d_sensor, L.w_sensor, L.i_sensor);
    Route rt = route_of(h);
    const double *d_dt;
    if (listed && (rc = rt.in(rows, N, 1, sizeof(int32_t), p_rows))) return rc;
    if ((rc = rt.dt_in(dt, dt_len, N, p_dt, &d_dt))) return rc;
    if (r.has_rng && ((rc = rt.in(src.ranges, N, A, sizeof(int32_t), p_ranges)) || (rc = rt.in(src.err, N, A, m, p_err)))) return rc;
    if (r.has_imu && ((rc = rt.in(src.accel, N, 3, m, p_accel)) || (rc = rt.in(src.cov, N, 9, m, p_cov)))) return rc;
    if (r.width && (rc = rt.in(src.sensor, N, r.width, sizeof(double), p_sensor))) return rc;
    const RoundIn in = {(const int32_t *)rt.at(p_ranges), rt.at(p_err), rt.at(p_accel), rt.at(p_cov), (const double *)rt.at(p_sensor)};
    KArgs a;
    round_args(h, r, in, d_dt, dt[0], (uint32_t *)rt.at(p_status), nullptr, a);
    rc = listed ? rows_step(h, nullptr, L, (const int32_t *)rt.at(p_rows), n, a) : launch_step(h, a, nullptr);
    if (r.width) h->planar_sensors = true; /* ranging epochs now carry the latched samples */
    if (rc) return rc;
    return rt.finish(status, p_status, N);
}

int kfpos_step_toa(kfpos_handle *h, const int32_t *range_mm, const void *err_est, const double *dt,
                   int32_t dt_len, uint32_t *status) {
    return round_host(h, "kfpos_step_toa", ROUND_TOA, 0, false, nullptr, 0, {range_mm, err_est, nullptr, nullptr, nullptr}, dt, dt_len, status);
}
int kfpos_step_imu(kfpos_handle *h, const void *accel, const void *cov, const double *dt, int32_t dt_len,
                   uint32_t *status) {
    return round_host(h, "kfpos_step_imu", ROUND_IMU, 0, false, nullptr, 0, {nullptr, nullptr, accel, cov, nullptr}, dt, dt_len, status);
}
int kfpos_step_sensor(kfpos_handle *h, int32_t kind, const double *data, const double *dt, int32_t dt_len,
                      uint32_t *status) {
    return round_host(h, "kfpos_step_sensor", ROUND_SENSOR, kind, false, nullptr, 0, {nullptr, nullptr, nullptr, nullptr, data}, dt, dt_len, status);
}
int kfpos_step_toa_imu(kfpos_handle *h, const int32_t *range_mm, const void *err_est, const void *accel,
                       const void *cov, const double *dt, int32_t dt_len, uint32_t *status) {
    return round_host(h, "kfpos_step_toa_imu", ROUND_FUSED, 0, false, nullptr, 0, {range_mm, err_est, accel, cov, nullptr}, dt, dt_len, status);
}

/* getPose (pos, cov3x3, vel) or the predicted state (x, P) of the whole bank: out[k] = the caller's k-th array (null = not
 * wanted), dt validated by the caller. The results sit behind one another in the mapped block's output region, getPose's
 * 15 rows first; staged, getPose's in d_out and the predicted state in the staging area -- reserved together with their
 * row-major turns, so that no region moves while another is in use. */
static int pose_host(kfpos_handle *h, const double *dt, int32_t dt_len, bool predicted, double *const out[3],
                     uint32_t *status) {
    DevScope dev_(h->cfg.device);
    const size_t T = h->cfg.n_tags, n = h->n;
    const size_t w[3] = {predicted ? n : 3, predicted ? n * n : 9, predicted ? 0 : (size_t)3};
    int rc = drain_slots(h);
    if (rc) return rc;
    Route rt = route_of(h);
    const Place p_dt = {h->sm.dt, h->d_dt, nullptr}, p_status = {h->sm.status, h->d_status, nullptr};
    if (predicted && (rc = rt.reserve(2 * (n + n * n) * T * sizeof(double) + 1024))) return rc;
    double *d[3];
    for (size_t k = 0, off = predicted ? 15 * T : 0; k < 3; off += w[k++] * T) {
        Place p = {h->sm.out + off * sizeof(double), h->d_out + off, nullptr};
        if (predicted && (rc = rt.region(w[k] * T * sizeof(double), p))) return rc;
        d[k] = (double *)rt.at(p);
    }
    const double *d_each;
    if ((rc = rt.dt_in(dt, dt_len, T, p_dt, &d_each))) return rc;
    uint32_t *d_status = (uint32_t *)rt.at(p_status);
    rc = predicted ? launch_pose(h, dt[0], d_each, nullptr, nullptr, nullptr, d_status, nullptr, d[0], d[1])
                   : launch_pose(h, dt[0], d_each, d[0], d[1], d[2], d_status, nullptr);
    if (rc || (rc = rt.sync())) return rc;
    for (int k = 0; k < 3; ++k)
        if (out[k] && (rc = rt.out(out[k], d[k], T, (int)w[k]))) return rc;
    return rt.words(status, p_status, T);
}

int kfpos_get_pose(kfpos_handle *h, double dt_ahead, double *pos, double *cov3x3, double *vel,
                   uint32_t *status) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    double *const out[3] = {pos, cov3x3, vel};
    return pose_host(h, &dt_ahead, 1, false, out, status);
}

int kfpos_get_pose_each(kfpos_handle *h, const double *dt_ahead, double *pos, double *cov3x3, double *vel,
                        uint32_t *status) {
    g_err.clear();
    if (!dt_ahead || !h) return KFPOS_ERR_ARG;
    double *const out[3] = {pos, cov3x3, vel};
    return pose_host(h, dt_ahead, h->cfg.n_tags, false, out, status);
}

int kfpos_get_predicted(kfpos_handle *h, const double *dt_ahead, int32_t dt_len, double *x, double *P,
                        uint32_t *status) {
    g_err.clear();
    if (!h || !dt_ahead || !x || !P || (dt_len != 1 && dt_len != h->cfg.n_tags)) return KFPOS_ERR_ARG;
    double *const out[3] = {x, P, nullptr};
    return pose_host(h, dt_ahead, dt_len, true, out, status);
}

/* ---- row-list steps: kfpos_step_*_rows, kfpos_slot_acquire_rows / kfpos_slot_submit_rows ----
 * The step kernels are not touched and see no row index: the listed tags' stored bits are gathered into a compact work
 * bank (kfpos_k_tags.hip: k_rows_work), the kernel this handle runs anyway steps that bank with KArgs::T = n, and the
 * result is scattered back. Launches per round: gather + one layout turn per input array (2 for a ranging round, 4 for a
 * fused one, 1 for a sensor sample; none on a small bank's mapped block) + step + scatter. */
/* room for n listed tags; growing frees the old block, so everything in flight completes first */
extern "C++" int rows_reserve(kfpos_handle *h, size_t n) {
    if (n <= h->work_cap) return KFPOS_OK;
    size_t cap = n > 2 * h->work_cap ? n : 2 * h->work_cap;
    if (cap > (size_t)h->cfg.n_tags) cap = h->cfg.n_tags;
    HIPCHK(hipDeviceSynchronize());
    h->work_cap = 0;
    HIPCHK(hipMalloc((void **)h->d_work.out(), kfpos_layout::rows_layout(handle_sizes(h), KFPOS_N_SLOTS, cap, cap).total));
    h->work_cap = cap;
    return KFPOS_OK;
}
/* tags_check(unique) in O(n) -- a round of the streaming path validates its list on every submission: each row carries
 * the number of the call that last listed it. Same answers, same texts: the first offending entry of the list. */
extern "C++" int rows_check(kfpos_handle *h, const char *who, const int32_t *rows, int32_t n) {
    if (n < 0 || (n > 0 && !rows)) return tags_check(h, who, rows, n, true);
    if (h->row_stamp.empty()) h->row_stamp.assign((size_t)h->cfg.n_tags, 0u);
    if (++h->stamp == 0) { /* wrapped: forget every earlier call */
        std::fill(h->row_stamp.begin(), h->row_stamp.end(), 0u);
        h->stamp = 1;
    }
    for (int32_t i = 0; i < n; ++i) {
        const int32_t r = rows[i];
        if (r < 0 || r >= h->cfg.n_tags || h->row_stamp[r] == h->stamp) return tags_check(h, who, rows, i + 1, true);
        h->row_stamp[r] = h->stamp;
    }
    return KFPOS_OK;
}
/* gather -> step -> scatter on stream s. a: fill_args + the inputs of the call at [.][n], status [n], traj [3][n] */
extern "C++" int rows_step(kfpos_handle *h, hipStream_t s, const kfpos_layout::Rows &L, const int32_t *d_rows, int n, KArgs &a) {
    using namespace kfpos_k;
    TagArgs g;
    tag_args(h, g);
    g.n_comp = fresh_table(h->n, h->psz, g.comp); /* the stored rows of a tag: the list a reset writes */
    g.n = n;
    g.rows = d_rows;
    for (int b = 0; b < TB_N; ++b) g.wbuf[b] = g.buf[b] ? h->d_work + L.w[b] : nullptr;
    g.wflags = (uint32_t *)(h->d_work + L.w_flags);
    launch_tags(TAGS_WORK_IN, h->cfg.storage, s, g);
    HIPCHK(hipGetLastError());
    a.T = n;
    a.pos = (double *)g.wbuf[TB_POS];
    a.vel = (double *)g.wbuf[TB_VEL];
    a.P = g.wbuf[TB_P];
    a.flags = g.wflags;
    a.imu_acc = g.wbuf[TB_IMU_ACC];
    a.imu_cov = g.wbuf[TB_IMU_COV];
    a.platch = (double *)g.wbuf[TB_LATCH];
    const int rc = launch_step(h, a, s);
    if (rc) return rc;
    launch_tags(TAGS_WORK_OUT, h->cfg.storage, s, g);
    HIPCHK(hipGetLastError());
    return KFPOS_OK;
}

int kfpos_step_toa_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const int32_t *range_mm, const void *err_est,
                        const double *dt, int32_t dt_len, uint32_t *status) {
    return round_host(h, "kfpos_step_toa_rows", ROUND_TOA, 0, true, rows, n, {range_mm, err_est, nullptr, nullptr, nullptr}, dt, dt_len, status);
}
int kfpos_step_imu_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const void *accel, const void *cov,
                        const double *dt, int32_t dt_len, uint32_t *status) {
    return round_host(h, "kfpos_step_imu_rows", ROUND_IMU, 0, true, rows, n, {nullptr, nullptr, accel, cov, nullptr}, dt, dt_len, status);
}
int kfpos_step_toa_imu_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const int32_t *range_mm, const void *err_est,
                            const void *accel, const void *cov, const double *dt, int32_t dt_len, uint32_t *status) {
    return round_host(h, "kfpos_step_toa_imu_rows", ROUND_FUSED, 0, true, rows, n, {range_mm, err_est, accel, cov, nullptr}, dt, dt_len, status);
}
int kfpos_step_sensor_rows(kfpos_handle *h, const int32_t *rows, int32_t n, int32_t kind, const double *data,
                           const double *dt, int32_t dt_len, uint32_t *status) {
    return round_host(h, "kfpos_step_sensor_rows", ROUND_SENSOR, kind, true, rows, n, {nullptr, nullptr, nullptr, nullptr, data}, dt, dt_len, status);
}

int kfpos_timing_begin(kfpos_handle *h, void *stream) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    HIPCHK(hipEventRecord(h->ev0, (hipStream_t)stream));
    return KFPOS_OK;
}
int kfpos_timing_end(kfpos_handle *h, void *stream, float *elapsed_ms) {
    g_err.clear();
    if (!h || !elapsed_ms) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    HIPCHK(hipEventRecord(h->ev1, (hipStream_t)stream));
    HIPCHK(hipEventSynchronize(h->ev1));
    HIPCHK(hipEventElapsedTime(elapsed_ms, h->ev0, h->ev1));
    return KFPOS_OK;
}

} // extern "C"
