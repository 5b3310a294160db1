/*
 * kfpos_kernels.h -- what the kernel translation units of libkfpos_hip.so share: the kernel-argument blocks, the
 * device-side helpers that stage an epoch (component-major HBM -> registers / LDS), and the selector functions through
 * which the host side (kfpos_hip.hip, kfpos_hip_state.hip, kfpos_hip_slots.hip, kfpos_hip_replay.hip) obtains a kernel without seeing its template, and what those
 * host units share among themselves (at the end of namespace kfpos_k's declarations). WHICH kernel a launch takes, over
 * how many workgroups and with how many bytes of LDS: kfpos_launch_plan.h.
 *
 * Execution model: ONE FILTER PER LANE, 64 filters per wavefront, one wavefront per workgroup.
 *  - The whole per-tag state (position, velocity, packed covariance: 21 / 36 / 45 doubles) lives in
 *    VGPRs/AGPRs for the duration of a step -- and across the epochs of a multi-epoch launch; every array
 *    index in kfpos_core.h is a compile-time constant after unrolling. At 65 536 tags there is exactly one
 *    wavefront per SIMD (1024 waves on 256 CUs x 4 SIMDs), so the 512-register file per lane is free to use.
 *    No kernel may spill to scratch inside a loop (checked at build time, tools/check_scratch.py).
 *  - HBM layout is component-major ([component][tag]): lane l of a wave reads element
 *    base + tag0 + l, so every state / measurement access is one fully coalesced
 *    512-byte (f64) or 256-byte (f32 / int32) wave transaction, each byte touched once.
 *  - The epoch's measurements -- range in metres (the integer-mm wire value converted once, with the
 *    reference's exact `(double) mm / 1000`, Posgenerator.cpp:484), errorEstimation, working weight (1/e for
 *    the ML sweeps, 1/R for the IEKF sweeps) -- live in registers for 8 anchors (RegScratch) and per lane in
 *    LDS otherwise, [anchor][lane] (lane-consecutive 8-byte words: conflict-free ds_read_b64), with
 *    compile-time anchor loops for 16 anchors (StaticScratch) and a run-time loop for every other count. The
 *    inner sweeps (2-4 ML + 3-20 IEKF per step) then touch only registers / LDS + SGPRs, never HBM.
 *  - Anchor coordinates are wave-uniform: they travel in the kernel-argument segment and are read
 *    with scalar loads into SGPRs.
 *  - No MFMA: the largest dense object is 9x9 per filter; lanes are independent filters, so there is nothing to
 *    shuffle and no barrier (the exception: the 8-lanes-per-tag kernel of small banks, kfpos_k_coop.hip).
 *
 * Translation units (one code object each, built in parallel): kfpos_k_toa6s / kfpos_k_toa6f (6-state filter, symmetric /
 * full covariance layout), kfpos_k_toa6eachs / kfpos_k_toa6eachf (6-state, ranging slots with a timeline per tag, the same two layouts), kfpos_k_coop (6-state, 8 lanes per tag), kfpos_k_cells6s / kfpos_k_cells6f / kfpos_k_cells9 (ranging rounds of a bank with anchor cells, an anchor table per block of 64 rows: the step kernels of kfpos_k_toa6.inc / kfpos_k_imu9.inc once more, around CellArgs), kfpos_k_imu9 (9-state; its text is kfpos_k_imu9.inc), kfpos_k_imu9ev (9-state, event schedules), kfpos_k_imu9each (9-state, event schedules with a timeline per tag), kfpos_k_planarev (8-state planar filter, event schedules), kfpos_k_planareach (8-state planar filter, event schedules with a timeline per tag), kfpos_k_misc (8-state planar
 * filter, standalone ML estimator, getPose for the bank and for a list of tags, layout turns), kfpos_k_tags (per-tag gather / scatter / reset, the work bank of row-list steps), kfpos_k_d16 (the decoder of KFPOS_SLOT_RANGES_D16 rounds), kfpos_hip (host side + C ABI; it and kfpos_hip_replay turn a Plan of kfpos_launch_plan.h into a kernel and launch it, and hold no LDS size or kernel form of their own), kfpos_hip_state (the state side of the C ABI: whole-bank accessors, per-tag lifecycle, pose for a row list), kfpos_hip_slots (the streaming slots of the C ABI, kfpos_slot_*), kfpos_hip_replay (the replay entry points of the C ABI: whole schedules in few launches), kfpos_comm (RCCL gather).
 */
#ifndef KFPOS_KERNELS_H
#define KFPOS_KERNELS_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <type_traits>

#define KFPOS_HD __host__ __device__
#include "kfpos_core.h"
#include "kfpos_internal.h"
#include "kfpos_launch_plan.h"
#include "kfpos_p48.h"
#include "kfpos_replay_plan.h"
#include "kfpos_state_record.h"

namespace kfpos_k {

/* kernel arguments: everything wave-uniform, read through scalar loads */
struct KArgs {
    double anchors[KFPOS_MAX_ANCHORS * 3];
    int T, A;
    double accel_noise, jolt, cost_threshold;
    int ignore_worst, top_n, use_init_pos, ml_variant;
    int pair9;        /* 9-state kernel: two lanes per tag for the tail of the gain iteration (default: on in the mixed and p48 storage modes; KFPOS_PAIR9=0 / =1 overrides: profiles/HISTORY.md "The pairs' tail") */
    int imu9_diag;    /* 9-state kernel: a wavefront whose accelerometer covariances are all diagonal runs the diagonal form of the gain iteration's pass (same bits; KFPOS_IMU9_DIAG=0: never) */
    /* planar filter configuration (kfpos_planar_config) */
    int use_fixed_height, imu_fixed_cov_acc, imu_fixed_cov_w;
    /* pair9's meeting points (Params::pair9_first / pair9_dense_until; KFPOS_PAIR9_MEET=first,dense_until at kfpos_create,
     * both 1 .. 20). Two 16-bit fields HERE, in the four bytes that were padding in front of the doubles: no other field
     * moves, so no other kernel's argument loads do */
    short pair9_first, pair9_dense_until;
    double px4_height, px4_arm_p1, px4_arm_p2, px4_cov_vel, px4_cov_gyro_z;
    double imu_cov_acc, imu_cov_w, mag_offset, mag_cov;
    double *platch;   /* [15][T] planar filter: latched PX4Flow (5), IMU (8), magnetometer (2) samples */
    const double *sensor; /* planar sensor call: [C][T] sample of this call (C = 5 / 24 / 3 / 1) */
    /* persistent state, component-major */
    double *pos;      /* [3][T] */
    double *vel;      /* [3][T] (9-state; always f64: the 9-state filter amplifies velocity rounding);
                         planar filter: [4][T] = vx, vy, theta, omega */
    void *P;          /* [SZ][T] real */
    uint32_t *flags;  /* [T] */
    void *imu_acc;    /* [3][T] real, latched sample (9-state) */
    void *imu_cov;    /* [6][T] real, lower triangle {00,10,11,20,21,22} of the latched covariance */
    /* epoch inputs */
    const int32_t *ranges; /* [A][T] */
    const void *err;       /* [A][T] real */
    const double *dt;      /* [T] or null */
    double dt_shared;
    const void *accel;     /* [3][T] real */
    const void *cov;       /* [9][T] real */
    int mode, latch;
    uint32_t *status;      /* [T] or null */
    /* multi-epoch launches (kfpos_run_trace_dev): epoch s reads its inputs at base + s * stride (elements),
     * dt_steps[s] is its shared dt. n_steps = 1 is the single-epoch case and uses dt / dt_shared. */
    int n_steps;
    long long stride_ranges, stride_err, stride_accel, stride_cov;
    double *traj;          /* [n_steps][3][T] positions after each epoch, or null */
    double dt_steps[KFPOS_TRACE_CHUNK];
};


struct PoseArgs {
    int T, model, full;
    double accel_noise, jolt, dt_ahead;
    const double *dt_each; /* [T] per-tag extrapolation time, or null to use dt_ahead */
    const double *pos_in;
    const double *vel_in;
    const void *P;
    const uint32_t *flags;
    double *pos, *cov, *vel; /* [3][T], [9][T], [3][T]; any may be null */
    double *full_x, *full_P; /* [n][T], [n*n][T] predicted state / covariance (row-major index first), or null */
    uint32_t *status;
};

/* k_get_pose_rows (kfpos_k_misc.hip): getPose for a list of tags, a block of its own around an unchanged PoseArgs. p.T,
 * p.pos_in / vel_in / P / flags describe the bank as ever; entry i of the list is row rows[i] of it, p.dt_each (or null:
 * p.dt_ahead) is indexed by ENTRY, and the outputs are row-major per entry: pos [n][3], cov [n][9], vel [n][3],
 * full_x [n][dim], full_P [n][dim * dim], status [n]; any may be null (full_x and full_P together). */
struct PoseRowsArgs {
    PoseArgs p;
    const int32_t *rows; /* DEVICE (or mapped), [n], validated by the host */
    int n;
};

typedef void (*step_kernel_t)(const KArgs);

/* kfpos_run_events_dev (kfpos_k_imu9ev.hip): an argument block of its own around KArgs, whose layout every other kernel
 * sees unchanged. k.n_steps events; k.dt_steps[e] is the timeLag of event e; bit e of `kinds` says what it is (0 =
 * KFPOS_EVENT_IMU, 1 = KFPOS_EVENT_TOA); the j-th ranging event of the launch reads k.ranges / k.err + j * stride,
 * the i-th IMU event k.accel + i * stride; k.cov is the one covariance of the call; k.traj / status_events start at
 * the launch's first event; k.status: the last event's words, or null. */
struct EvArgs {
    KArgs k;
    unsigned long long kinds[KFPOS_TRACE_CHUNK / 64];
    uint32_t *status_events; /* [n_steps][T] or null */
};
static_assert(KFPOS_TRACE_CHUNK == 128, "EvArgs::kinds is indexed as two 64-bit words");
static_assert(KFPOS_TRACE_CHUNK == KFPOS_PLAN_MAX_EVENTS, "kfpos_replay_plan.h packs and decodes `kinds` for this many events");
static_assert(sizeof(EvArgs) <= 4096, "kernel arguments are limited to 4 KB");
typedef void (*events_kernel_t)(const EvArgs);

/* kfpos_run_events_each_dev (kfpos_k_imu9each.hip): the same schedule with a timeline per tag, again a block of its own
 * around an unchanged KArgs. `kinds` as in EvArgs -- a slot's kind is shared by the bank --, but the timeLag is per tag:
 * dt_each[e * T + t] is tag t's in slot e of the launch, < 0 = the tag sits the slot out (k.dt_steps is unused). The
 * ordinals of ranges and samples count SLOTS, not a tag's own events. k.cov is the one covariance of the call, null in
 * a launch without an IMU slot. */
struct EvEachArgs {
    KArgs k;
    unsigned long long kinds[KFPOS_TRACE_CHUNK / 64];
    uint32_t *status_events; /* [n_steps][T] or null */
    const double *dt_each;   /* DEVICE, [n_steps][T], at the launch's first slot */
};
static_assert(sizeof(EvEachArgs) <= 4096, "kernel arguments are limited to 4 KB");
typedef void (*events_each_kernel_t)(const EvEachArgs);

/* kfpos_run_trace_each_dev (kfpos_k_toa6eachs.hip / kfpos_k_toa6eachf.hip): ranging slots of the 6-state filter with a
 * timeline per tag, a block of its own around an unchanged KArgs as well. Every slot is a ranging epoch, so there are no
 * kinds: slot e of the launch reads k.ranges / k.err + e * stride, dt_each[e * T + t] is tag t's timeLag in it, < 0 =
 * the tag sits the slot out (k.dt_steps is unused). k.traj / status_events start at the launch's first slot; k.status:
 * the last slot's words, or null. */
struct TraceEachArgs {
    KArgs k;
    uint32_t *status_events; /* [n_steps][T] or null */
    const double *dt_each;   /* DEVICE, [n_steps][T], at the launch's first slot */
};
static_assert(sizeof(TraceEachArgs) <= 4096, "kernel arguments are limited to 4 KB");
typedef void (*trace_each_kernel_t)(const TraceEachArgs);

/* kfpos_run_planar_events_dev (kfpos_k_planarev.hip): the planar filter's argument block around KArgs, unchanged as
 * well. k.n_steps events; k.dt_steps[e] is the timeLag of event e; its kind (0 = ranging, KFPOS_SENSOR_* otherwise)
 * is nibble e of `kinds`; the j-th ranging event of the launch reads k.ranges / k.err + j * stride, the i-th event of
 * sensor kind c sens[c - 1] + i * stride_sens[c - 1]; k.traj / status_events start at the launch's first event;
 * k.status: the last event's words, or null. */
struct PevArgs {
    KArgs k;
    uint32_t kinds[KFPOS_TRACE_CHUNK / 8];
    const double *sens[4];     /* PX4Flow [5][T], IMU [24][T], magnetometer [3][T], compass [1][T] */
    long long stride_sens[4];
    uint32_t *status_events;   /* [n_steps][T] or null */
};
static_assert(sizeof(PevArgs) <= 4096, "kernel arguments are limited to 4 KB");
typedef void (*planar_events_kernel_t)(const PevArgs);

/* kfpos_run_planar_events_each_dev (kfpos_k_planareach.hip): the planar schedule with a timeline per tag, once more a
 * block of its own around an unchanged KArgs. kinds, sens, stride_sens and status_events as in PevArgs -- a slot's kind
 * is shared by the bank --, but the timeLag is per tag: dt_each[e * T + t] is tag t's in slot e of the launch, < 0 = the
 * tag sits the slot out (k.dt_steps is unused). The ordinals of ranges and samples count SLOTS, not a tag's own events. */
struct PevEachArgs {
    KArgs k;
    uint32_t kinds[KFPOS_TRACE_CHUNK / 8];
    const double *sens[4];     /* PX4Flow [5][T], IMU [24][T], magnetometer [3][T], compass [1][T] */
    long long stride_sens[4];
    uint32_t *status_events;   /* [n_steps][T] or null */
    const double *dt_each;     /* DEVICE, [n_steps][T], at the launch's first slot */
};
static_assert(sizeof(PevEachArgs) <= 4096, "kernel arguments are limited to 4 KB");
typedef void (*planar_events_each_kernel_t)(const PevEachArgs);

/* Ranging rounds of a bank with anchor cells (kfpos_set_anchor_cells; kfpos_k_cells6s.hip / kfpos_k_cells6f.hip,
 * kfpos_k_cells9.hip): KArgs, unchanged, and behind it where the tables are. A step kernel takes its argument block as a
 * template parameter (KArgs by default) and names the by-value parameter itself wherever it reads a field: CellArgs
 * derives from KArgs, so the one text reads a.T, a.flags, ... of either block, and `if constexpr (cells_block<ARGS>)`
 * guards the lines that differ (kfpos_k_toa6.inc, kfpos_k_imu9.inc). Rows [64 b, 64 b + 64) are workgroup b of the launch
 * and range against cell cell_of_block[b], whose table starts at cell_xyz + cell_of_block[b] * cell_stride: A rows of
 * xyz, zeros up to max_anchors rows (cell_stride = 3 * max_anchors doubles: a kernel with a compile-time anchor count
 * reads that many rows whatever A is, and finds the zeros kfpos_set_anchors pads with). `anchors` is not read. The host
 * has checked every entry of cell_of_block against the number of cells: the kernels index with it as it is. */
struct CellArgs : KArgs {
    const double *cell_xyz;       /* DEVICE, [n_cells][max_anchors][3] */
    const int32_t *cell_of_block; /* DEVICE, [(T + 63) / 64] */
    int32_t cell_stride;          /* doubles from one cell's table to the next */
};
static_assert(sizeof(CellArgs) <= 4096, "kernel arguments are limited to 4 KB");
static_assert(KFPOS_CELL_TAGS == kfpos_plan::LANES, "a cell is assigned per workgroup: one wavefront, one tag per lane");
template <class ARGS>
constexpr bool cells_block = std::is_same<ARGS, CellArgs>::value;
/* One workgroup is one wavefront is one block of KFPOS_CELL_TAGS rows, so a cell's table is wave-uniform as the
 * kernel-argument table is: map and table are read through pointers in the constant address space (scalar loads) */
typedef const __attribute__((address_space(4))) double *cell_table_t;
typedef const __attribute__((address_space(4))) int32_t *cell_map_t;
typedef void (*cells_kernel_t)(const CellArgs);

/* ---- selectors: each is defined in the translation unit that instantiates the kernels it hands out ----
 * st = KFPOS_STORE_*; as = anchor-count specialisation (8: epoch in registers; -8 / -16: compile-time loops over an
 * LDS-resident epoch; 0: run-time loop); heur: 0 = no outlier heuristic, 1 = top-N only, 2 = leave-one-out */
step_kernel_t toa6_sym_kernel(int st, int as, int heur, bool two_waves);   /* kfpos_k_toa6s.hip */
step_kernel_t toa6_full_kernel(int st, int as, int heur);                  /* kfpos_k_toa6f.hip */
step_kernel_t toa6_coop_kernel(int st);                                    /* kfpos_k_coop.hip */
trace_each_kernel_t toa6_each_sym_kernel(int st, int as, int heur);        /* kfpos_k_toa6eachs.hip */
trace_each_kernel_t toa6_each_full_kernel(int st, int as, int heur);       /* kfpos_k_toa6eachf.hip */
step_kernel_t imu9_kernel(int st, int as, bool ranging);                   /* kfpos_k_imu9.hip */
cells_kernel_t cells_toa6_sym_kernel(int st, int as, int heur);            /* kfpos_k_cells6s.hip */
cells_kernel_t cells_toa6_full_kernel(int st, int as, int heur);           /* kfpos_k_cells6f.hip */
cells_kernel_t cells_imu9_kernel(int st, int as);                          /* kfpos_k_cells9.hip: as = 8 or 0 */
events_kernel_t imu9_events_kernel(int st, int as);                        /* kfpos_k_imu9ev.hip: as = 8 or 0 */
events_each_kernel_t imu9_events_each_kernel(int st, int as);              /* kfpos_k_imu9each.hip: as = 8 or 0 */
planar_events_kernel_t planar_events_kernel(int st, int as);               /* kfpos_k_planarev.hip: as = -8 or 0 */
planar_events_each_kernel_t planar_events_each_kernel(int st, int as);     /* kfpos_k_planareach.hip: as = -8 or 0 */
step_kernel_t ml_kernel(int st, int as);                                   /* kfpos_k_misc.hip */
step_kernel_t planar_kernel(int st, bool sensors, int as);                 /* kfpos_k_misc.hip */
void launch_get_pose(int model, bool full, int st, int blocks, hipStream_t s, const PoseArgs &a); /* kfpos_k_misc.hip */
void launch_get_pose_rows(int model, bool full, int st, hipStream_t s, const PoseRowsArgs &a);    /* kfpos_k_misc.hip */
void launch_rows_to_cols(size_t esz, hipStream_t s, const void *src, void *dst, int T, int C);    /* kfpos_k_misc.hip */
void launch_cols_to_rows(hipStream_t s, const double *src, double *dst, int T, int C);            /* kfpos_k_misc.hip */

/* ---- per-tag lifecycle (kfpos_k_tags.hip): gather / scatter / reset of a list of tags ----
 * TagComp, TC_*, TAG_SECTIONS, TAG_COMPS and the two tables of comp[] (the record of a tag / its stored rows):
 * kfpos_state_record.h. TB_* (TB_POS ... TB_LATCH, TB_N), the indices into TagArgs::buf: kfpos_host_layout.h */
enum : int { TAGS_GATHER = 0, TAGS_SCATTER = 1, TAGS_RESET = 2, TAGS_WORK_IN = 3, TAGS_WORK_OUT = 4 };
struct TagArgs {
    int T, n, psz;            /* tags in the bank, tags listed in this launch, stored covariance entries per tag */
    int w[TAG_SECTIONS];      /* gather / scatter: components per tag of each section present in `val`, 0 = section absent */
    int cbase[TAG_SECTIONS];  /* where each section starts in comp[] */
    int n_comp;               /* reset: stored rows listed in comp[] */
    void *buf[TB_N];          /* the bank's component-major arrays */
    uint32_t *flags;          /* [T] */
    const int32_t *rows;      /* [n] rows of the bank, validated by the host */
    double *val;              /* staging: x [n][w0] | P [n][w1] | latch [n][w2] | height [n][w3] */
    uint32_t *fl;             /* staging: [n] flags words, or null */
    const double *init;       /* reset: [n][3] start positions, or null = cst[0..2] */
    double cst[5];            /* reset: start position x y z (NaN: ML initialisation), planar height, planar angle */
    void *wbuf[TB_N];         /* TAGS_WORK_IN / _OUT: the work bank, the same arrays as buf[] at stride n (row-list steps) */
    uint32_t *wflags;         /* [n] */
    TagComp comp[TAG_COMPS];
};
void launch_tags(int op, int st, hipStream_t s, const TagArgs &a);          /* kfpos_k_tags.hip */
/* TAGS_WORK_IN: work[c][i] = bank[c][rows[i]] for every stored row c listed in comp[] (n_comp of them, the list reset
 * uses) and the flags word, raw stored bits; TAGS_WORK_OUT: the inverse. The step kernels then run on the work bank
 * with KArgs::T = n: they never see a row index. */

/* ---- k_decode_d16 (kfpos_k_d16.hip): the int16 codes and the escape list of a KFPOS_SLOT_RANGES_D16 round -> the int32
 * range matrix and the moved base (kfpos_d16.h). n = max_anchors * n_tags elements, flat; the escape indices have been
 * validated by the host */
struct D16Args {
    const int16_t *code; /* [n], 16-byte aligned */
    const int32_t *esc;  /* [n_esc][2]: flat index, value; 8-byte aligned */
    uint32_t n_esc, n, T;
    const double *dt;    /* [T] per-tag dt of the round (< 0: the tag's codes and entries are not read), or null */
    int32_t *base, *out; /* [n] each, 16-byte aligned */
};
void launch_decode_d16(hipStream_t s, const D16Args &a);                    /* kfpos_k_d16.hip */

constexpr int PLANAR_HAS_SHIFT = 4;              /* planar flags word: bits 5..7 = latched PX4Flow / IMU / magnetometer */
/* LATCH_ROWS: kfpos_host_layout.h; COOP_LANES, COOP_TAGS_PER_WAVE: kfpos_launch_plan.h */

} // namespace kfpos_k

/* ---- what the host units share: defined in kfpos_hip.hip unless noted, used by kfpos_hip_state.hip,
 * kfpos_hip_replay.hip and kfpos_hip_slots.hip as well ---- */
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
/* what launch selection depends on (kfpos_launch_plan.h): the handle's configuration and kfpos_create's policy flags */
inline kfpos_plan::Inputs plan_inputs(const kfpos_handle *h) {
    return {h->cfg.model, h->cfg.storage, h->cfg.max_anchors, h->full != 0, h->cfg.ignore_worst != 0, h->cfg.top_n != 0,
            h->force_generic, h->coop, h->two_waves, h->planar_sensors};
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

namespace {

using namespace kfpos;
using kfpos_k::KArgs;
using kfpos_k::CellArgs;
using kfpos_k::cells_block;
using kfpos_k::PoseArgs;
using kfpos_k::PoseRowsArgs;
using kfpos_k::step_kernel_t;
using kfpos_k::COOP_LANES;
using kfpos_k::COOP_TAGS_PER_WAVE;
using kfpos_k::PLANAR_HAS_SHIFT;
using kfpos_k::LATCH_ROWS;

constexpr int WAVE = kfpos_plan::LANES; /* lanes per workgroup = one wavefront */

enum StepMode : int { MODE_TOA = 0, MODE_IMU_ONLY = 1, MODE_FUSED = 2 };

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

template <class P>
__device__ inline P make_params_of(const KArgs &a) {
    P pr;
    pr.anchors = a.anchors;
    pr.n_anchors = a.A;
    pr.accel_noise = a.accel_noise;
    pr.jolt = a.jolt;
    pr.cost_threshold = a.cost_threshold;
    pr.ignore_worst = a.ignore_worst;
    pr.top_n = a.top_n;
    pr.ml_variant = a.ml_variant;
    pr.use_init_pos = a.use_init_pos;
    pr.use_fixed_height = a.use_fixed_height;
    pr.imu_fixed_cov_acc = a.imu_fixed_cov_acc;
    pr.imu_fixed_cov_w = a.imu_fixed_cov_w;
    pr.px4_height = a.px4_height;
    pr.px4_arm_p1 = a.px4_arm_p1;
    pr.px4_arm_p2 = a.px4_arm_p2;
    pr.px4_cov_vel = a.px4_cov_vel;
    pr.px4_cov_gyro_z = a.px4_cov_gyro_z;
    pr.imu_cov_acc = a.imu_cov_acc;
    pr.imu_cov_w = a.imu_cov_w;
    pr.mag_offset = a.mag_offset;
    pr.mag_cov = a.mag_cov;
    return pr;
}
__device__ inline Params make_params(const KArgs &a) { return make_params_of<Params>(a); }
/* the anchor table of this workgroup's cell: what Params::anchors points at in a kernel built around CellArgs */
__device__ inline const double *cell_anchors(const CellArgs &c) {
    const int cell = ((kfpos_k::cell_map_t)c.cell_of_block)[blockIdx.x];
    return (const double *)((kfpos_k::cell_table_t)c.cell_xyz + (size_t)cell * c.cell_stride);
}

/* The 6-state selector table, once for every kernel family that has these forms (k_step_toa6 around either argument
 * block: kfpos_k_toa6.inc; k_trace_toa6_each: kfpos_k_toa6each.inc): FAM::kernel<SYMM, REAL, MREAL, AS, HEUR>() is the
 * family's instantiation. heur: 0 = the bank has no outlier heuristic (BASELINE configs 2 and 4), 1 = top-N only
 * (config 5), 2 = leave-one-out (with or without top-N). 0 and 1 get instantiations with no leave-one-out loop compiled
 * in: 13 % faster at 8 anchors. Combinations that run the AS = 0 form because their own would touch scratch memory
 * inside the epoch loop (make check): DESIGN.md section 6 lists them. */
template <class FAM, bool SYMM, typename REAL, typename MREAL>
auto toa6_table(int as, int heur) -> decltype(FAM::template kernel<SYMM, REAL, MREAL, 0, 0>()) {
    if constexpr (SYMM) {
        if (as == 8) return heur ? FAM::template kernel<true, REAL, MREAL, 8, 2>() : FAM::template kernel<true, REAL, MREAL, 8, 0>();
    } else {
        /* non-symmetric layout (ML initialisation): its SVD path needs the registers a resident epoch would take
         * (148-180 bytes/lane of scratch otherwise), so the 8-anchor epoch goes to LDS, loops still compile-time */
        if (as == 8) {
            if (!heur) return FAM::template kernel<false, REAL, MREAL, -8, 0>();
            /* (leave-one-out with the 48-bit covariance: the host never asks -- kfpos_create -- and the instantiation
             * is not built: it would access scratch memory inside its epoch loop) */
            if constexpr (!std::is_same<REAL, p48>::value) return FAM::template kernel<false, REAL, MREAL, -8, 2>();
        }
    }
    if (as == -16) return heur == 1 ? FAM::template kernel<SYMM, REAL, MREAL, -16, 1>() : FAM::template kernel<SYMM, REAL, MREAL, -16, 2>();
    return heur ? FAM::template kernel<SYMM, REAL, MREAL, 0, 2>() : FAM::template kernel<SYMM, REAL, MREAL, 0, 0>();
}

/* Raw epoch of one tag as it sits in HBM: fetched one epoch ahead in multi-epoch launches, so its
 * latency hides behind the previous epoch's arithmetic. */
template <typename MREAL, int AS>
struct RawEpoch {
    int32_t mm[AS];
    MREAL e[AS];
};
template <typename MREAL, int AS>
__device__ inline void fetch_epoch(const KArgs &a, size_t t, int s, RawEpoch<MREAL, AS> &raw) {
    const int32_t *rp = a.ranges + (size_t)s * a.stride_ranges;
    const MREAL *ep = (const MREAL *)a.err + (size_t)s * a.stride_err;
#pragma unroll
    for (int k = 0; k < AS; ++k) { /* all loads first: one latency, not AS of them */
        raw.mm[k] = (rp + (size_t)k * a.T)[(uint32_t)t];
        raw.e[k] = (ep + (size_t)k * a.T)[(uint32_t)t];
    }
}
template <typename MREAL, int AS>
__device__ inline void unpack_epoch(const RawEpoch<MREAL, AS> &raw, RegScratch<AS> &sc) {
#pragma unroll
    for (int k = 0; k < AS; ++k) {
        sc.r[k] = raw.mm[k] > 0 ? kf_mm_to_m(raw.mm[k]) : 0.0; /* Posgenerator.cpp:483-484 */
        sc.e[k] = (double)raw.e[k];
        sc.w[k] = 0.0;
    }
}
/* generic anchor count: epoch s -> per-lane LDS scratch */
template <typename MREAL>
__device__ inline Scratch stage_epoch_lds(const KArgs &a, double *lds, int lane, size_t t, int s) {
    Scratch sc;
    sc.r = lds + lane;
    sc.e = lds + (size_t)a.A * WAVE + lane;
    sc.w = lds + 2 * (size_t)a.A * WAVE + lane;
    sc.stride = WAVE;
    const int32_t *rp = a.ranges + (size_t)s * a.stride_ranges;
    const MREAL *ep = (const MREAL *)a.err + (size_t)s * a.stride_err;
    for (int k = 0; k < a.A; ++k) {
        const int32_t mm = (rp + (size_t)k * a.T)[(uint32_t)t];
        sc.r[k * WAVE] = mm > 0 ? kf_mm_to_m(mm) : 0.0;
        sc.e[k * WAVE] = (double)(ep + (size_t)k * a.T)[(uint32_t)t];
    }
    return sc;
}
/* anchor count known at compile time: all 2 N loads first, then the conversions and the LDS stores */
template <typename MREAL, int N>
__device__ inline StaticScratch<N> stage_epoch_lds_n(const KArgs &a, double *lds, int lane, size_t t, int s) {
    StaticScratch<N> sc;
    sc.r = lds + lane;
    sc.e = lds + (size_t)N * WAVE + lane;
    sc.w = lds + 2 * (size_t)N * WAVE + lane;
    sc.stride = WAVE;
    RawEpoch<MREAL, N> raw;
    fetch_epoch<MREAL, N>(a, t, s, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sc.r[k * WAVE] = raw.mm[k] > 0 ? kf_mm_to_m(raw.mm[k]) : 0.0;
        sc.e[k * WAVE] = (double)raw.e[k];
    }
    return sc;
}
/* ---- 9-state kernels (kfpos_k_imu9.inc, kfpos_k_imu9ev.hip): the accelerometer sample and its covariance ---- */
/* The acceleration sample is fetched one epoch ahead like the ranges. Its covariance is loaded and whitened ONCE per
 * launch: a multi-epoch launch always has one covariance array for all its epochs (stride_cov = 0: a sensor with a
 * fixed covariance); a trace with a covariance per epoch is replayed one epoch per launch (kfpos_run_trace_dev). */
template <typename MREAL>
struct RawImu {
    MREAL acc[3];
};
template <typename MREAL>
__device__ inline void fetch_imu(const KArgs &a, size_t t, int s, RawImu<MREAL> &raw) {
    const MREAL *ap = (const MREAL *)a.accel + (size_t)s * a.stride_accel;
#pragma unroll
    for (int k = 0; k < 3; ++k) raw.acc[k] = (ap + (size_t)k * a.T)[(uint32_t)t];
}
template <typename MREAL>
__device__ inline void fetch_imu_cov(const KArgs &a, size_t t, int s, MREAL raw[9]) {
    const MREAL *cp = (const MREAL *)a.cov + (size_t)s * a.stride_cov;
#pragma unroll
    for (int k = 0; k < 9; ++k) raw[k] = (cp + (size_t)k * a.T)[(uint32_t)t];
}
template <typename MREAL>
__device__ inline void latch_imu_cov(const KArgs &a, size_t T, uint32_t t32, const double cv[9]) {
    strow<MREAL>(a.imu_cov, 0, T, t32, cv[0]);
    strow<MREAL>(a.imu_cov, 1, T, t32, cv[3]);
    strow<MREAL>(a.imu_cov, 2, T, t32, cv[4]);
    strow<MREAL>(a.imu_cov, 3, T, t32, cv[6]);
    strow<MREAL>(a.imu_cov, 4, T, t32, cv[7]);
    strow<MREAL>(a.imu_cov, 5, T, t32, cv[8]);
}

/* step_imu9_state's `fast`: the wavefront's accelerometer covariances are diagonal (diag: decided per launch) and every
 * lane that is about to run the step has a sample -- one ballot over the lanes that are here */
__device__ inline bool imu9_fast(bool diag, bool has) {
    return diag && __builtin_amdgcn_ballot_w64(!has) == 0;
}
/* A wave-uniform epoch index the optimiser cannot see through: addresses derived from it are formed anew in every
 * epoch (a few scalar instructions) instead of living as two dozen running row pointers across the whole epoch loop,
 * where they exhaust the scalar registers and end up as spilled 64-bit per-lane addresses. */
__device__ inline int opaque_uniform(int v) {
    asm volatile("" : "+s"(v));
    return v;
}
/* the same for the lane's tag index: its per-array 64-bit addresses are then formed where they are used instead of
 * being carried (spilled) across the epoch loop */
__device__ inline size_t opaque_lane(size_t t) {
    uint32_t v = (uint32_t)t;
    asm volatile("" : "+v"(v));
    return v;
}
/* the same with 4-byte errorEstimations kept as they are: LDS = r [N][lane] f64 | w [N][lane] f64 | e [N][lane] f32 */
template <int N>
__device__ inline StaticScratchF<N> stage_epoch_lds_nf(const KArgs &a, double *lds, int lane, size_t t, int s) {
    StaticScratchF<N> sc;
    sc.r = lds + lane;
    sc.w = lds + (size_t)N * WAVE + lane;
    sc.e = (float *)(lds + 2 * (size_t)N * WAVE) + lane;
    sc.stride = WAVE;
    RawEpoch<float, N> raw;
    fetch_epoch<float, N>(a, t, s, raw);
#pragma unroll
    for (int k = 0; k < N; ++k) {
        sc.r[k * WAVE] = raw.mm[k] > 0 ? kf_mm_to_m(raw.mm[k]) : 0.0;
        sc.e[k * WAVE] = raw.e[k];
    }
    return sc;
}
/* doubles of LDS the epoch of a compile-time-count kernel takes per workgroup */
template <typename MREAL, int N>
constexpr size_t static_epoch_doubles() { return kfpos_plan::static_epoch_doubles(sizeof(MREAL), N); }
__device__ inline double epoch_dt(const KArgs &a, size_t t, int s) {
    return a.n_steps > 1 ? a.dt_steps[s] : (a.dt ? a.dt[(uint32_t)t] : a.dt_shared);
}

/* a lane that sits a call out (dt < 0, or a dropped PX4Flow sample) still reports where its tag is: the trajectory /
 * pose output of the call carries the untouched position (what getPose at timeLag 0 would return) */
__device__ inline void skipped_lane(const KArgs &a, size_t t, bool write) {
    if (!write) return;
    if (a.status) a.status[t] = ST_SKIPPED;
    if (a.traj) {
#pragma unroll
        for (int k = 0; k < 3; ++k) (a.traj + (size_t)k * a.T)[(uint32_t)t] = (a.pos + (size_t)k * a.T)[(uint32_t)t];
    }
}

} // namespace
#endif /* KFPOS_KERNELS_H */
