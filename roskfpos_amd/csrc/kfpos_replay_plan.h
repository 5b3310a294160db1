/*
 * kfpos_replay_plan.h -- the two decisions every replay entry point (kfpos_hip_replay.hip) shares with the kernels it
 * launches, and nobody else knows:
 *   - the wire format of `kinds` in a kernel-argument block: a packer (host) and its decoder (kernel) side by side;
 *   - how a schedule of events is cut into launches, and which per-kind ordinals carry from launch to launch.
 * No HIP header: g++ compiles this file alone (tests/replay/plan_driver.cpp); KFPOS_HD as in kfpos_p48.h.
 */
#ifndef KFPOS_REPLAY_PLAN_H
#define KFPOS_REPLAY_PLAN_H

#include <stddef.h>
#include <stdint.h>

#ifndef KFPOS_HD
#define KFPOS_HD
#endif

#define KFPOS_PLAN_MAX_EVENTS 128 /* events per launch at the most: KFPOS_TRACE_CHUNK (kfpos_kargs.h asserts it) */
#define KFPOS_PLAN_MAX_KINDS 5    /* the planar filter's: ranging, PX4Flow, IMU, magnetometer, compass */

/* ---- 9-state schedules (EvArgs, EvEachArgs): one bit per event, 0 = KFPOS_EVENT_IMU, 1 = KFPOS_EVENT_TOA ---- */
#define KFPOS_KINDS1_WORDS (KFPOS_PLAN_MAX_EVENTS / 64)
inline void kfpos_kinds1_pack(unsigned long long words[KFPOS_KINDS1_WORDS], const uint8_t *kinds, int n) {
    for (int w = 0; w < KFPOS_KINDS1_WORDS; ++w) words[w] = 0;
    for (int e = 0; e < n; ++e) words[e >> 6] |= (unsigned long long)(kinds[e] & 1u) << (e & 63);
}
KFPOS_HD inline int kfpos_kinds1_at(const unsigned long long *words, int e) {
    return (int)((words[(e >> 6) & 1] >> (e & 63)) & 1ull);
}

/* ---- planar schedules (PevArgs, PevEachArgs): four bits per event, 0 = ranging, 1..4 = KFPOS_SENSOR_* ---- */
#define KFPOS_KINDS4_WORDS (KFPOS_PLAN_MAX_EVENTS / 8)
inline void kfpos_kinds4_pack(uint32_t words[KFPOS_KINDS4_WORDS], const uint8_t *kinds, int n) {
    for (int w = 0; w < KFPOS_KINDS4_WORDS; ++w) words[w] = 0;
    for (int e = 0; e < n; ++e) words[e >> 3] |= (uint32_t)(kinds[e] & 7u) << ((e & 7) * 4);
}
KFPOS_HD inline int kfpos_kinds4_at(const uint32_t *words, int e) {
    return (int)((words[e >> 3] >> ((e & 7) * 4)) & 7u);
}

/* ---- the cut: events [first, n_events) in launches of up to `chunk` events ----
 * The events ahead of `first` went down the ranging path, one ranging input each, so the ranging ordinal starts at
 * `first`; every other ordinal at 0. ord[kind] of a launch = events of that kind ahead of its e0: where the launch's
 * first event of that kind finds its input. n_kinds = 2: the 9-state kinds (ranging is 1); 5: the planar ones (ranging
 * is 0); 0, kinds = NULL: every event is a ranging slot (the 6-state per-tag form), there is nothing to count.
 *     for (kfpos_replay_cut c(kinds, n_events, first, chunk, n_kinds); c.next();) launch(c.e0, c.n, c.ord); */
struct kfpos_replay_cut {
    int e0, n;                         /* this launch: events [e0, e0 + n) */
    size_t ord[KFPOS_PLAN_MAX_KINDS];
    const uint8_t *kinds;
    int n_events, chunk;

    kfpos_replay_cut(const uint8_t *kinds_, int n_events_, int first, int chunk_, int n_kinds)
        : e0(first), n(0), ord{}, kinds(kinds_), n_events(n_events_), chunk(chunk_) {
        if (n_kinds) ord[n_kinds == 2 ? 1 : 0] = (size_t)first;
    }
    bool next() {
        if (kinds)
            for (int k = 0; k < n; ++k) ++ord[kinds[e0 + k]];
        e0 += n;
        n = n_events - e0 < chunk ? n_events - e0 : chunk;
        return n > 0;
    }
    bool last() const { return e0 + n == n_events; }
};

#endif /* KFPOS_REPLAY_PLAN_H */
