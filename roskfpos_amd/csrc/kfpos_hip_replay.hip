/*
 * kfpos_hip_replay.hip -- the replay entry points of the C ABI (include/kfpos.h): a whole schedule of events in few
 * launches. kfpos_run_trace_dev (ranging epochs, shared dt), kfpos_run_trace_each_dev (6-state, a timeline per tag),
 * kfpos_run_events_dev / _each_dev (9-state), kfpos_run_planar_events_dev / _each_dev (planar). Each of them is argument
 * checks plus what is its own; what they share is written once, above them: the validation of `kinds`, the two ranging
 * paths ahead of a replay kernel's first event, a family's replay plan (kfpos_launch_plan.h: form, grid, LDS bytes) as
 * its kernel, and the one loop that launches. How a schedule is cut into launches and how `kinds` travels: kfpos_replay_plan.h. No kernel lives
 * here: like kfpos_hip.hip this unit obtains them through the selectors of kfpos_kargs.h.
 */
#include <cstring>
#include <string>

#include "kfpos_host.h"

namespace {

static_assert(KFPOS_EVENT_IMU == 0 && KFPOS_EVENT_TOA == 1, "kfpos_kinds1_pack, kfpos_replay_cut: ranging is bit / kind 1");
static_assert(KFPOS_PLANAR_EVENT_TOA == 0 && KFPOS_SENSOR_COMPASS == 4, "kfpos_kinds4_pack, kfpos_replay_cut: ranging is kind 0 of 5");

int no_anchors() {
    g_err = "kfpos_set_anchors has not been called (the node drops ranges until the anchors are known, Posgenerator.cpp:92-96)";
    return KFPOS_ERR_STATE;
}

/* ---- validation of `kinds`, one per family; `fn` is the entry point the user called ---- */
int bad_kind(const char *fn, int e, int kind, const std::string &why) {
    g_err = std::string(fn) + ": kinds[" + std::to_string(e) + "] = " + std::to_string(kind) + why;
    return KFPOS_ERR_ARG;
}
/* 9-state: every kind is one, the arrays of the kinds that occur are there, the handle can run them. *first_imu: the
 * call's first sample (n_events: none) */
int check_events9(const char *fn, const kfpos_handle *h, int n_events, const uint8_t *kinds, const void *range_mm,
                  const void *err_est, const void *accel, const void *cov, int *first_imu) {
    int n_toa = 0;
    *first_imu = n_events;
    for (int e = 0; e < n_events; ++e) {
        if (kinds[e] == KFPOS_EVENT_TOA) ++n_toa;
        else if (kinds[e] != KFPOS_EVENT_IMU) return bad_kind(fn, e, kinds[e], " is no event kind");
        else if (*first_imu == n_events) *first_imu = e;
    }
    if ((n_toa && (!range_mm || !err_est)) || (n_toa < n_events && (!accel || !cov))) return KFPOS_ERR_ARG;
    if (h->cfg.model != KFPOS_MODEL_TOA_IMU) return KFPOS_ERR_MODEL;
    return n_toa && !h->have_anchors ? no_anchors() : KFPOS_OK;
}
/* planar: the same. *first_sensor: the call's first event that is no ranging (n_events: none) */
int check_planar_events(const char *fn, const kfpos_handle *h, int n_events, const uint8_t *kinds,
                        const kfpos_planar_inputs *in, int *first_sensor) {
    static const char *const names[5] = {"range_mm / err_est", "px4flow", "imu", "mag", "compass"};
    const bool have[5] = {in->range_mm && in->err_est, in->px4flow != nullptr, in->imu != nullptr, in->mag != nullptr,
                          in->compass != nullptr};
    int n_toa = 0;
    *first_sensor = -1;
    for (int e = 0; e < n_events; ++e) {
        const int kind = kinds[e];
        if (kind > KFPOS_SENSOR_COMPASS) return bad_kind(fn, e, kind, " is no event kind");
        if (!have[kind]) return bad_kind(fn, e, kind, std::string(" but kfpos_planar_inputs.") + names[kind] + " is NULL");
        if (kind == KFPOS_PLANAR_EVENT_TOA) ++n_toa;
        else if (*first_sensor < 0) *first_sensor = e;
    }
    if (*first_sensor < 0) *first_sensor = n_events;
    if (h->cfg.model != KFPOS_MODEL_PLANAR) return KFPOS_ERR_MODEL;
    return n_toa && !h->have_anchors ? no_anchors() : KFPOS_OK;
}

/* ---- ranging events ahead of the replay kernel's first event: they go down launch_step ---- */
/* the last of the per-event status words is the call's, where the ranging path ran the call to its end */
int copy_last_status(const kfpos_handle *h, int n_events, const uint32_t *status_events, uint32_t *status, hipStream_t s) {
    const size_t T = h->cfg.n_tags;
    if (status_events && status)
        HIPCHK(hipMemcpyAsync(status, status_events + (size_t)(n_events - 1) * T, sizeof(uint32_t) * T, hipMemcpyDeviceToDevice, s));
    return KFPOS_OK;
}
/* Shared timeline: events [0, lead) through the multi-epoch ranging path of kfpos_run_trace_dev, up to trace_chunk of
 * them per launch. It reports the last status word of a launch only, so with status_events every one of these events
 * is a launch of its own. */
int ranging_lead(kfpos_handle *h, int lead, int n_events, const double *dt_events, const int32_t *range_mm,
                 int64_t stride_ranges, const void *err_est, int64_t stride_err, double *trajectory,
                 uint32_t *status_events, uint32_t *status, hipStream_t s) {
    const size_t T = h->cfg.n_tags, r = h->msz;
    KArgs a;
    fill_args(h, a);
    a.mode = MODE_TOA;
    a.stride_ranges = stride_ranges;
    a.stride_err = stride_err;
    const int chunk = status_events ? 1 : h->policy.trace_chunk;
    for (int s0 = 0; s0 < lead; s0 += chunk) {
        const int n = lead - s0 < chunk ? lead - s0 : chunk;
        a.n_steps = n;
        a.ranges = range_mm + (size_t)s0 * stride_ranges;
        a.err = (const char *)err_est + (size_t)s0 * stride_err * r;
        for (int k = 0; k < n; ++k) a.dt_steps[k] = dt_events[s0 + k];
        a.dt_shared = dt_events[s0];
        a.traj = trajectory ? trajectory + (size_t)s0 * 3 * T : nullptr;
        a.status = status_events ? status_events + (size_t)s0 * T : (s0 + n == n_events ? status : nullptr);
        const int rc = launch_step(h, a, s);
        if (rc != KFPOS_OK) return rc;
    }
    return lead > 0 && lead == n_events ? copy_last_status(h, n_events, status_events, status, s) : KFPOS_OK;
}
/* A timeline per tag: slots [0, lead) as the single calls they stand for, one launch each -- KArgs carries a per-tag dt
 * with n_steps == 1 only. */
int ranging_lead_each(kfpos_handle *h, int lead, int n_events, const double *dt_each, const int32_t *range_mm,
                      int64_t stride_ranges, const void *err_est, int64_t stride_err, double *trajectory,
                      uint32_t *status_events, uint32_t *status, hipStream_t s) {
    const size_t T = h->cfg.n_tags, r = h->msz;
    KArgs a;
    fill_args(h, a);
    a.mode = MODE_TOA;
    for (int e = 0; e < lead; ++e) {
        a.ranges = range_mm + (size_t)e * stride_ranges;
        a.err = (const char *)err_est + (size_t)e * stride_err * r;
        a.dt = dt_each + (size_t)e * T;
        a.traj = trajectory ? trajectory + (size_t)e * 3 * T : nullptr;
        a.status = status_events ? status_events + (size_t)e * T : (e + 1 == n_events ? status : nullptr);
        const int rc = launch_step(h, a, s);
        if (rc != KFPOS_OK) return rc;
    }
    return lead > 0 && lead == n_events ? copy_last_status(h, n_events, status_events, status, s) : KFPOS_OK;
}

/* ---- a family's replay plan (kfpos_launch_plan.h: the shared-timeline and the per-tag form alike) as its kernel ---- */
using kfpos_plan::Plan;
Plan replay_plan(const kfpos_handle *h, kfpos_plan::Launch what) { return kfpos_plan::plan(plan_inputs(h), what); }
template <class K>
int replay_kernel(K kern, const Plan &p, K *out) {
    if (p.bytes() > 64 * 1024) HIPCHK(hipFuncSetAttribute((const void *)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.bytes()));
    *out = kern;
    return KFPOS_OK;
}

/* ---- the launch loop of every replay kernel: events [first, n_events), up to trace_chunk per launch ----
 * Sets what every argument block has -- the launch's event count, where its trajectory rows and per-event status words
 * start, the call's status on the last launch only --, then own(cut) fills in what is the caller's for this launch. */
template <class K, class Args, class Own>
int replay_launches(kfpos_handle *h, K kern, const Plan &p, Args &ev, const uint8_t *kinds, int n_kinds, int first,
                    int n_events, double *trajectory, uint32_t *status_events, uint32_t *status, hipStream_t s, Own own) {
    const size_t T = h->cfg.n_tags;
    for (kfpos_replay_cut c(kinds, n_events, first, h->policy.trace_chunk, n_kinds); c.next();) {
        ev.k.n_steps = c.n;
        ev.k.traj = trajectory ? trajectory + (size_t)c.e0 * 3 * T : nullptr;
        ev.status_events = status_events ? status_events + (size_t)c.e0 * T : nullptr;
        ev.k.status = c.last() ? status : nullptr;
        own(c);
        hipLaunchKernelGGL(kern, dim3(p.groups(h->cfg.n_tags)), dim3(WAVE), p.bytes(), s, ev);
        HIPCHK(hipGetLastError());
        h->stepped = true;
    }
    return KFPOS_OK;
}

/* the shared dt of a launch's events (the forms with a timeline per tag leave dt_steps zeroed: their kernels do not read it) */
void shared_dt(KArgs &k, const double *dt_events, const kfpos_replay_cut &c) {
    for (int i = 0; i < c.n; ++i) k.dt_steps[i] = dt_events[c.e0 + i];
    k.dt_shared = dt_events[c.e0];
}
void no_shared_dt(KArgs &k) {
    for (double &d : k.dt_steps) d = 0.0;
}

/* the 9-state inputs of a launch: either kind at its ordinal (arrays of a kind that does not occur may be missing) */
template <class Args>
void imu9_inputs(const kfpos_handle *h, Args &ev, const uint8_t *kinds, const int32_t *range_mm, const void *err_est,
                 const void *accel, const kfpos_replay_cut &c) {
    const size_t j = c.ord[KFPOS_EVENT_TOA], i = c.ord[KFPOS_EVENT_IMU], r = h->msz;
    ev.k.ranges = range_mm ? range_mm + j * ev.k.stride_ranges : nullptr;
    ev.k.err = err_est ? (const char *)err_est + j * ev.k.stride_err * r : nullptr;
    ev.k.accel = accel ? (const char *)accel + i * ev.k.stride_accel * r : nullptr;
    kfpos_kinds1_pack(ev.kinds, kinds + c.e0, c.n);
}
/* the planar inputs of a launch: every kind at its ordinal; the launch latches samples, so from here on ranging epochs
 * carry them (kfpos_step_sensor_dev) */
template <class Args>
void planar_strides(Args &ev, const kfpos_planar_inputs *in) {
    ev.k.stride_ranges = in->stride_ranges;
    ev.k.stride_err = in->stride_err;
    const int64_t stride[4] = {in->stride_px4flow, in->stride_imu, in->stride_mag, in->stride_compass};
    for (int c = 0; c < 4; ++c) ev.stride_sens[c] = stride[c];
}
template <class Args>
void planar_inputs(kfpos_handle *h, Args &ev, const kfpos_planar_inputs *in, const uint8_t *kinds, const kfpos_replay_cut &c) {
    const double *const base[4] = {in->px4flow, in->imu, in->mag, in->compass};
    ev.k.ranges = in->range_mm ? in->range_mm + c.ord[0] * in->stride_ranges : nullptr;
    ev.k.err = in->err_est ? (const char *)in->err_est + c.ord[0] * in->stride_err * h->msz : nullptr;
    for (int k = 0; k < 4; ++k) ev.sens[k] = base[k] ? base[k] + c.ord[k + 1] * ev.stride_sens[k] : nullptr;
    kfpos_kinds4_pack(ev.kinds, kinds + c.e0, c.n);
    h->planar_sensors = true;
}

} // namespace

extern "C" {

int kfpos_run_trace_dev(kfpos_handle *h, int32_t n_steps, const int32_t *range_mm, int64_t stride_ranges,
                        const void *err_est, int64_t stride_err, const void *accel, int64_t stride_accel,
                        const void *cov, int64_t stride_cov, const double *dt_steps, double *trajectory,
                        uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || n_steps < 0 || !range_mm || !err_est || !dt_steps) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    if (accel && (!cov || h->cfg.model != KFPOS_MODEL_TOA_IMU)) return KFPOS_ERR_MODEL;
    if (!h->have_anchors) return KFPOS_ERR_STATE;
    KArgs a;
    fill_args(h, a);
    a.status = status;
    a.mode = accel ? MODE_FUSED : MODE_TOA;
    a.stride_ranges = stride_ranges;
    a.stride_err = stride_err;
    a.stride_accel = stride_accel;
    a.stride_cov = stride_cov;
    const size_t r = h->msz;
    /* the kernels whiten the accelerometer covariance once per launch: a covariance per epoch means one epoch per launch */
    const int chunk = (accel && stride_cov != 0) ? 1 : h->policy.trace_chunk;
    /* Up to `chunk` epochs per launch: the kernel keeps every tag's state in registers across them, so
     * state traffic and launch boundaries are paid once per chunk instead of once per epoch. (A loop of its own, not
     * ranging_lead: the sample, its covariance and the latch, a status every launch writes.) */
    for (int s0 = 0; s0 < n_steps; s0 += chunk) {
        const int n = n_steps - s0 < chunk ? n_steps - s0 : chunk;
        a.n_steps = n;
        a.ranges = range_mm + (size_t)s0 * stride_ranges;
        a.err = (const char *)err_est + (size_t)s0 * stride_err * r;
        if (accel) {
            a.accel = (const char *)accel + (size_t)s0 * stride_accel * r;
            a.cov = (const char *)cov + (size_t)s0 * stride_cov * r;
            a.latch = (s0 + n == n_steps) ? 1 : 0; /* leave the last sample latched, as n separate calls would */
        }
        for (int k = 0; k < n; ++k) a.dt_steps[k] = dt_steps[s0 + k];
        a.dt_shared = dt_steps[s0];
        a.traj = trajectory ? trajectory + (size_t)s0 * 3 * h->cfg.n_tags : nullptr;
        const int rc = launch_step(h, a, (hipStream_t)stream);
        if (rc != KFPOS_OK) return rc;
    }
    return KFPOS_OK;
}

int kfpos_run_events_dev(kfpos_handle *h, int32_t n_events, const uint8_t *kinds, const double *dt_events,
                         const int32_t *range_mm, int64_t stride_ranges, const void *err_est, int64_t stride_err,
                         const void *accel, int64_t stride_accel, const void *cov, double *trajectory,
                         uint32_t *status_events, uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || n_events < 0) return KFPOS_ERR_ARG;
    if (n_events == 0) return KFPOS_OK;
    if (!kinds || !dt_events) return KFPOS_ERR_ARG;
    int lead; /* ranging events ahead of the call's first sample */
    int rc = check_events9("kfpos_run_events_dev", h, n_events, kinds, range_mm, err_est, accel, cov, &lead);
    if (rc != KFPOS_OK) return rc;
    if (h->n_cells > 0) return cells_refusal("kfpos_run_events_dev", CELLS_NO_REPLAY);
    DevScope dev_(h->cfg.device);
    const hipStream_t s = (hipStream_t)stream;
    /* They re-fuse what the handle held latched, with THAT sample's covariance: the ranging path, which reads the latch. */
    rc = ranging_lead(h, lead, n_events, dt_events, range_mm, stride_ranges, err_est, stride_err, trajectory, status_events, status, s);
    if (rc != KFPOS_OK || lead == n_events) return rc;
    /* From the first sample on: k_events_imu9. Every launch leaves its last sample and `cov` latched, so the next one
     * (and whoever calls next) finds them where single calls leave them. */
    kfpos_k::events_kernel_t kern;
    const Plan p = replay_plan(h, kfpos_plan::EVENTS9);
    rc = replay_kernel(kfpos_k::imu9_events_kernel(h->cfg.storage, p.as), p, &kern);
    if (rc != KFPOS_OK) return rc;
    kfpos_k::EvArgs ev;
    fill_args(h, ev.k);
    ev.k.stride_ranges = stride_ranges;
    ev.k.stride_err = stride_err;
    ev.k.stride_accel = stride_accel;
    ev.k.cov = cov;
    return replay_launches(h, kern, p, ev, kinds, 2, lead, n_events, trajectory, status_events, status, s,
                           [&](const kfpos_replay_cut &c) {
        imu9_inputs(h, ev, kinds, range_mm, err_est, accel, c);
        shared_dt(ev.k, dt_events, c);
    });
}

int kfpos_run_events_each_dev(kfpos_handle *h, int32_t n_events, const uint8_t *kinds, const double *dt_events_dev,
                              const int32_t *range_mm, int64_t stride_ranges, const void *err_est, int64_t stride_err,
                              const void *accel, int64_t stride_accel, const void *cov, double *trajectory,
                              uint32_t *status_events, uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || n_events < 0) return KFPOS_ERR_ARG;
    if (n_events == 0) return KFPOS_OK;
    if (!kinds || !dt_events_dev) return KFPOS_ERR_ARG;
    int first_imu;
    int rc = check_events9("kfpos_run_events_each_dev", h, n_events, kinds, range_mm, err_est, accel, cov, &first_imu);
    if (rc != KFPOS_OK) return rc;
    if (h->n_cells > 0) return cells_refusal("kfpos_run_events_each_dev", CELLS_NO_REPLAY);
    DevScope dev_(h->cfg.device);
    /* No "lead" split as in kfpos_run_events_dev: which tags have ranging events ahead of their first sample is in
     * dt_events_dev, which the host never reads. The kernel switches whiteners per lane instead -- the latched
     * covariance's until the lane's own first sample, the call's from then on -- and every launch leaves the samples it
     * took latched with `cov`, so the next launch (and whoever calls next) finds them where single calls leave them. */
    kfpos_k::events_each_kernel_t kern;
    const Plan p = replay_plan(h, kfpos_plan::EVENTS9);
    rc = replay_kernel(kfpos_k::imu9_events_each_kernel(h->cfg.storage, p.as), p, &kern);
    if (rc != KFPOS_OK) return rc;
    kfpos_k::EvEachArgs ev;
    fill_args(h, ev.k);
    ev.k.stride_ranges = stride_ranges;
    ev.k.stride_err = stride_err;
    ev.k.stride_accel = stride_accel;
    no_shared_dt(ev.k);
    const size_t T = h->cfg.n_tags;
    return replay_launches(h, kern, p, ev, kinds, 2, 0, n_events, trajectory, status_events, status, (hipStream_t)stream,
                           [&](const kfpos_replay_cut &c) {
        imu9_inputs(h, ev, kinds, range_mm, err_est, accel, c);
        /* the kernel whitens `cov` only where a lane can come to use it: in a launch with an IMU slot */
        ev.k.cov = std::memchr(kinds + c.e0, KFPOS_EVENT_IMU, c.n) ? cov : nullptr;
        ev.dt_each = dt_events_dev + (size_t)c.e0 * T;
    });
}

int kfpos_run_trace_each_dev(kfpos_handle *h, int32_t n_steps, const double *dt_steps_dev, const int32_t *range_mm,
                             int64_t stride_ranges, const void *err_est, int64_t stride_err, double *trajectory,
                             uint32_t *status_steps, uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || n_steps < 0) return KFPOS_ERR_ARG;
    if (n_steps == 0) return KFPOS_OK;
    if (!dt_steps_dev || !range_mm || !err_est) return KFPOS_ERR_ARG;
    if (h->cfg.model != KFPOS_MODEL_TOA) return KFPOS_ERR_MODEL;
    if (!h->have_anchors) return no_anchors();
    if (h->n_cells > 0) return cells_refusal("kfpos_run_trace_each_dev", CELLS_NO_REPLAY);
    DevScope dev_(h->cfg.device);
    const size_t T = h->cfg.n_tags, r = h->msz;
    const hipStream_t s = (hipStream_t)stream;
    /* The 8-lanes-per-tag kernel sums in another order and has a contraction mode of its own (kfpos_k_coop.hip): a
     * one-tag-per-lane replay would not match what this handle's single calls compute. Such a handle runs its slots
     * as those single calls, one launch each: the same bits, not fused. */
    if (h->policy.coop)
        return ranging_lead_each(h, n_steps, n_steps, dt_steps_dev, range_mm, stride_ranges, err_est, stride_err, trajectory,
                                 status_steps, status, s);
    /* k_trace_toa6_each; a bank with more wavefronts than SIMDs runs it too (the two-wavefront build of the single
     * calls computes the same bits): the plan of the 6-state step without that build. */
    const Plan p = replay_plan(h, kfpos_plan::TRACE6_EACH);
    kfpos_k::trace_each_kernel_t kern;
    const int rc = replay_kernel(h->full ? kfpos_k::toa6_each_full_kernel(h->cfg.storage, p.as, p.heur)
                                         : kfpos_k::toa6_each_sym_kernel(h->cfg.storage, p.as, p.heur), p, &kern);
    if (rc != KFPOS_OK) return rc;
    kfpos_k::TraceEachArgs ev;
    fill_args(h, ev.k);
    ev.k.mode = MODE_TOA;
    ev.k.stride_ranges = stride_ranges;
    ev.k.stride_err = stride_err;
    no_shared_dt(ev.k);
    return replay_launches(h, kern, p, ev, nullptr, 0, 0, n_steps, trajectory, status_steps, status, s,
                           [&](const kfpos_replay_cut &c) {
        ev.k.ranges = range_mm + (size_t)c.e0 * stride_ranges;
        ev.k.err = (const char *)err_est + (size_t)c.e0 * stride_err * r;
        ev.dt_each = dt_steps_dev + (size_t)c.e0 * T;
    });
}

int kfpos_run_planar_events_dev(kfpos_handle *h, int32_t n_events, const uint8_t *kinds, const double *dt_events,
                                const kfpos_planar_inputs *in, double *trajectory, uint32_t *status_events,
                                uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || n_events < 0) return KFPOS_ERR_ARG;
    if (n_events == 0) return KFPOS_OK;
    if (!kinds || !dt_events || !in) return KFPOS_ERR_ARG;
    int lead; /* ranging events ahead of the call's first sensor event */
    int rc = check_planar_events("kfpos_run_planar_events_dev", h, n_events, kinds, in, &lead);
    if (rc != KFPOS_OK) return rc;
    DevScope dev_(h->cfg.device);
    const hipStream_t s = (hipStream_t)stream;
    /* On a handle that never had a sensor sample the ranging path is the closed-form ranging-only kernel, which single
     * calls would run as well. */
    rc = ranging_lead(h, lead, n_events, dt_events, in->range_mm, in->stride_ranges, in->err_est, in->stride_err, trajectory,
                      status_events, status, s);
    if (rc != KFPOS_OK || lead == n_events) return rc;
    /* From the first sensor event on: k_events_planar. Every launch leaves the samples it latched in HBM, so the next
     * one (and whoever calls next) finds them where single calls leave them. */
    kfpos_k::planar_events_kernel_t kern;
    const Plan p = replay_plan(h, kfpos_plan::EVENTS_PLANAR);
    rc = replay_kernel(kfpos_k::planar_events_kernel(h->cfg.storage, p.as), p, &kern);
    if (rc != KFPOS_OK) return rc;
    kfpos_k::PevArgs ev;
    fill_args(h, ev.k);
    planar_strides(ev, in);
    return replay_launches(h, kern, p, ev, kinds, 5, lead, n_events, trajectory, status_events, status, s,
                           [&](const kfpos_replay_cut &c) {
        planar_inputs(h, ev, in, kinds, c);
        shared_dt(ev.k, dt_events, c);
    });
}

int kfpos_run_planar_events_each_dev(kfpos_handle *h, int32_t n_events, const uint8_t *kinds,
                                     const double *dt_events_dev, const kfpos_planar_inputs *in, double *trajectory,
                                     uint32_t *status_events, uint32_t *status, void *stream) {
    g_err.clear();
    if (!h || n_events < 0) return KFPOS_ERR_ARG;
    if (n_events == 0) return KFPOS_OK;
    if (!kinds || !dt_events_dev || !in) return KFPOS_ERR_ARG;
    int first_sensor;
    int rc = check_planar_events("kfpos_run_planar_events_each_dev", h, n_events, kinds, in, &first_sensor);
    if (rc != KFPOS_OK) return rc;
    DevScope dev_(h->cfg.device);
    const hipStream_t s = (hipStream_t)stream;
    /* WHICH ranging kernel runs is a property of the handle: on one that never had a sensor sample a single
     * kfpos_step_toa_dev runs the closed-form ranging-only kernel for every tag, so the ranging slots ahead of the call's
     * first sensor slot go down launch_step there, one slot per launch. On a handle that has planar_sensors set the
     * single call is k_step_planar<true>, whose text k_events_planar_each runs: there the new kernel takes the call from
     * its first slot (lead = 0), one launch instead of one per leading slot. */
    const int lead = h->planar_sensors ? 0 : first_sensor;
    rc = ranging_lead_each(h, lead, n_events, dt_events_dev, in->range_mm, in->stride_ranges, in->err_est, in->stride_err,
                           trajectory, status_events, status, s);
    if (rc != KFPOS_OK || lead == n_events) return rc;
    /* From there on: k_events_planar_each. Every launch leaves the samples its lanes latched in HBM, so the next one
     * (and whoever calls next) finds them where single calls leave them. */
    kfpos_k::planar_events_each_kernel_t kern;
    const Plan p = replay_plan(h, kfpos_plan::EVENTS_PLANAR);
    rc = replay_kernel(kfpos_k::planar_events_each_kernel(h->cfg.storage, p.as), p, &kern);
    if (rc != KFPOS_OK) return rc;
    kfpos_k::PevEachArgs ev;
    fill_args(h, ev.k);
    planar_strides(ev, in);
    no_shared_dt(ev.k);
    const size_t T = h->cfg.n_tags;
    return replay_launches(h, kern, p, ev, kinds, 5, lead, n_events, trajectory, status_events, status, s,
                           [&](const kfpos_replay_cut &c) {
        planar_inputs(h, ev, in, kinds, c);
        ev.dt_each = dt_events_dev + (size_t)c.e0 * T;
    });
}

} // extern "C"
