/*
 * kfpos_kargs.h -- the contract between the host units and the kernel units of libkfpos_hip.so: the kernel-argument
 * blocks, and the selectors through which the host side obtains a kernel without seeing its template. No __device__
 * function, no handle: the kernels share kfpos_kernels.h beyond this, the host units kfpos_host.h, and neither side sees
 * the other's. WHICH kernel a launch takes, over how many workgroups, with how much LDS: kfpos_launch_plan.h.
 *
 * Translation units (one code object each, built in parallel, each with the headers the compiler saw it read):
 * kfpos_k_toa6s / kfpos_k_toa6f (6-state filter, symmetric / full covariance layout; text: kfpos_k_toa6.inc),
 * kfpos_k_toa6eachs / kfpos_k_toa6eachf (6-state, ranging slots with a timeline per tag; kfpos_k_toa6each.inc),
 * kfpos_k_coop (6-state, 8 lanes per tag), kfpos_k_cells6s / kfpos_k_cells6f / kfpos_k_cells9 (ranging rounds of a bank
 * with anchor cells, an anchor table per block of 64 rows: the step kernels of kfpos_k_toa6.inc / kfpos_k_imu9.inc once
 * more, around CellArgs), kfpos_k_imu9 (9-state; kfpos_k_imu9.inc), kfpos_k_imu9ev (9-state, event schedules),
 * kfpos_k_imu9each (the same with a timeline per tag), kfpos_k_planarev (8-state planar filter, event schedules),
 * kfpos_k_planareach (the same with a timeline per tag), kfpos_k_misc (planar filter, standalone ML estimator, getPose
 * for the bank and for a list of tags, layout turns), kfpos_k_tags (per-tag gather / scatter / reset, the work bank of
 * row-list steps), kfpos_k_d16 (the decoder of KFPOS_SLOT_RANGES_D16 rounds);
 * kfpos_hip (host side + C ABI; it and kfpos_hip_replay turn a Plan of kfpos_launch_plan.h into a kernel and launch it,
 * and hold no LDS size or kernel form of their own), kfpos_hip_state (whole-bank accessors, per-tag lifecycle, pose for
 * a row list), kfpos_hip_slots (the streaming slots, kfpos_slot_*), kfpos_hip_replay (the replay entry points: whole
 * schedules in few launches), kfpos_comm (RCCL gather).
 */
#ifndef KFPOS_KARGS_H
#define KFPOS_KARGS_H

#include <hip/hip_runtime.h>

#include <cstdint>
#include <type_traits>

#define KFPOS_HD __host__ __device__
#include "../../include/kfpos.h"
#include "kfpos_host_layout.h"
#include "kfpos_launch_plan.h"
#include "kfpos_replay_plan.h"
#include "kfpos_state_record.h"

#define KFPOS_TRACE_CHUNK 128 /* epochs per multi-epoch launch (their dt values travel in the kernel arguments) */

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

namespace {

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

} // namespace
#endif /* KFPOS_KARGS_H */
