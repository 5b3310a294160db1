/*
 * kfpos_hip_state.hip -- the state side of the C ABI (include/kfpos.h): the whole-bank accessors (kfpos_get_state /
 * kfpos_set_state, kfpos_get_latch / kfpos_set_latch, kfpos_get_height / kfpos_set_height), the per-tag lifecycle
 * (kfpos_get_tags / kfpos_set_tags / kfpos_reset_tags; kernels: kfpos_k_tags.hip) and the pose for a row list
 * (kfpos_get_pose_rows / kfpos_get_predicted_rows; kernel: k_get_pose_rows, kfpos_k_misc.hip). How a tag's record is laid
 * out in the bank is not written down here: kfpos_state_record.h holds the table, the whole-bank accessors walk it on the
 * CPU, the per-tag calls hand it to their kernels. Staging goes over the routes of kfpos_hip.hip (Route, kfpos_host.h).
 */
#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <type_traits>
#include <vector>

#include "kfpos_host.h"

using namespace kfpos_k;

void tag_args(const kfpos_handle *h, TagArgs &a) {
    std::memset(&a, 0, sizeof(a));
    a.T = h->cfg.n_tags;
    a.psz = h->psz;
    a.buf[TB_POS] = h->d_pos;
    a.buf[TB_VEL] = h->d_vel;
    a.buf[TB_P] = h->d_P;
    a.buf[TB_IMU_ACC] = h->d_imu_acc;
    a.buf[TB_IMU_COV] = h->d_imu_cov;
    a.buf[TB_LATCH] = h->d_latch;
    a.flags = h->d_flags;
}

/* The bounds check of the per-tag kernels. Nothing has been written when this fails; the text names the first offending
 * entry of the list, whichever rule it breaks. */
int tags_check(const kfpos_handle *h, const char *who, const int32_t *rows, int32_t n, bool unique) {
    if (n < 0 || (n > 0 && !rows)) {
        g_err = std::string(who) + (n < 0 ? ": n < 0" : ": rows == NULL");
        return KFPOS_ERR_ARG;
    }
    int32_t bad = 0; /* the first entry out of range, n if none */
    while (bad < n && rows[bad] >= 0 && rows[bad] < h->cfg.n_tags) ++bad;
    int32_t twice = bad; /* the first entry in front of it that repeats an earlier one */
    if (unique && bad > 1) {
        /* one sort of (row, position) keys: inside a run of equal rows positions ascend, so the second key of a run is
         * that row's first repeat */
        std::vector<uint64_t> key((size_t)bad);
        for (int32_t i = 0; i < bad; ++i) key[i] = ((uint64_t)(uint32_t)rows[i] << 32) | (uint32_t)i;
        std::sort(key.begin(), key.end());
        for (int32_t k = 1; k < bad; ++k) {
            const bool repeats = (key[k] >> 32) == (key[k - 1] >> 32);
            const bool second_of_run = repeats && (k == 1 || (key[k - 2] >> 32) != (key[k] >> 32));
            const int32_t at = (int32_t)(uint32_t)key[k];
            if (second_of_run && at < twice) twice = at;
        }
    }
    if (twice < bad) {
        g_err = std::string(who) + ": rows[" + std::to_string(twice) + "] = row " + std::to_string(rows[twice]) +
                " is listed twice";
        return KFPOS_ERR_ARG;
    }
    if (bad < n) {
        g_err = std::string(who) + ": rows[" + std::to_string(bad) + "] = row " + std::to_string(rows[bad]) +
                " is outside [0, " + std::to_string(h->cfg.n_tags) + ")";
        return KFPOS_ERR_ARG;
    }
    return KFPOS_OK;
}

namespace {

/* a get (STORE = false) writes the caller's arrays, a set only ever reads them; null = that part is absent */
template <bool STORE, typename E>
using io = std::conditional_t<STORE, const E, E>;

/* restored planar latch bits: ranging epochs must run the instantiation that honours them */
void planar_latch_bits(kfpos_handle *h, const uint32_t *flags, size_t n) {
    for (size_t i = 0; h->n == 8 && i < n; ++i) h->planar_sensors = h->planar_sensors || ((flags[i] >> PLANAR_HAS_SHIFT) != 0);
}

/* ---- the whole bank: every section asked for is turned on the CPU, between the caller's [T][w] array and host images
 * of the bank arrays its table entries name. A get copies down the rows it reads; a set copies up the rows it stores
 * through and no others (a planar x leaves the height row of d_pos alone, the height x and y): each a contiguous run. */
template <bool STORE>
int bank_transfer(kfpos_handle *h, io<STORE, double> *x, io<STORE, double> *P, io<STORE, uint32_t> *flags,
                  io<STORE, double> *latch, io<STORE, double> *height) {
    const kfpos_layout::Sizes sz = handle_sizes(h);
    TagArgs a; /* (for the bank's arrays by TB_*) */
    tag_args(h, a);
    int cbase[TAG_SECTIONS + 1];
    record_table(h->n, h->full, a.comp, cbase);
    io<STORE, double> *part[TAG_SECTIONS] = {x, P, latch, height};
    for (int s = 0; s < TAG_SECTIONS; ++s) {
        const TagComp *sec = a.comp + cbase[s];
        const int w = cbase[s + 1] - cbase[s];
        if (!part[s] || w == 0) continue;
        int kind[TB_N] = {}, lo[TB_N], hi[TB_N];
        for (int k = 0; k < w; ++k) {
            const TagComp d = sec[k];
            if (d.kind == TC_NONE || (STORE && !d.aux)) continue;
            lo[d.buf] = kind[d.buf] ? std::min<int>(lo[d.buf], d.row) : d.row;
            hi[d.buf] = kind[d.buf] ? std::max<int>(hi[d.buf], d.row) : d.row;
            kind[d.buf] = d.kind;
        }
        std::unique_ptr<unsigned char[]> image[TB_N]; /* not zeroed: every byte that is read or sent up is written first */
        unsigned char *img[TB_N] = {};
        for (int b = 0; b < TB_N; ++b)
            if (kind[b]) image[b].reset(img[b] = new unsigned char[image_bytes(kind[b], sz, hi[b])]);
        auto copy = [&]() -> int {
            for (int b = 0; b < TB_N; ++b) {
                ByteRun run[2];
                const int runs = kind[b] ? image_runs(kind[b], sz, lo[b], hi[b], run) : 0;
                for (int r = 0; r < runs; ++r) {
                    unsigned char *dev = (unsigned char *)a.buf[b] + run[r].off, *host = img[b] + run[r].off;
                    HIPCHK(STORE ? hipMemcpy(dev, host, run[r].bytes, hipMemcpyHostToDevice)
                                 : hipMemcpy(host, dev, run[r].bytes, hipMemcpyDeviceToHost));
                }
            }
            return KFPOS_OK;
        };
        if constexpr (STORE) record_in(sec, w, sz, img, part[s]);
        const int rc = copy();
        if (rc) return rc;
        if constexpr (!STORE) record_out(sec, w, sz, img, part[s]);
    }
    if (flags) {
        const size_t bytes = sizeof(uint32_t) * sz.T;
        if constexpr (STORE) HIPCHK(hipMemcpy(h->d_flags, flags, bytes, hipMemcpyHostToDevice));
        else HIPCHK(hipMemcpy(flags, h->d_flags, bytes, hipMemcpyDeviceToHost));
    }
    return KFPOS_OK;
}
/* kfpos_get_latch / kfpos_set_latch: a model without latched samples answers KFPOS_OK, to a null pointer as well */
template <bool STORE>
int latch_call(kfpos_handle *h, io<STORE, double> *latch) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    if (latch_width(h->n) == 0) return KFPOS_OK;
    if (!latch) return KFPOS_ERR_ARG;
    HIPCHK(hipDeviceSynchronize());
    return bank_transfer<STORE>(h, nullptr, nullptr, nullptr, latch, nullptr);
}
/* kfpos_get_height / kfpos_set_height: the planar filter's own */
template <bool STORE>
int height_call(kfpos_handle *h, io<STORE, double> *z) {
    g_err.clear();
    if (!h || !z) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    if (h->cfg.model != KFPOS_MODEL_PLANAR) return KFPOS_ERR_MODEL;
    HIPCHK(hipDeviceSynchronize());
    return bank_transfer<STORE>(h, nullptr, nullptr, nullptr, nullptr, z);
}

/* ---- the calls that take a row list ----
 * The way in, in this order: the handle, the list (tags_check; `who` names the call in the texts), what the call itself
 * refuses (refusal(): KFPOS_OK, or its code with the text set), the empty list, the handle's device, whatever the
 * streaming slots have in flight, a quiet device -- then the work. */
template <class Refusal, class Work>
int tags_call(kfpos_handle *h, const char *who, const int32_t *rows, int32_t n, bool unique, Refusal refusal, Work work) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    int rc = tags_check(h, who, rows, n, unique);
    if (rc || (rc = refusal())) return rc;
    if (n == 0) return KFPOS_OK;
    DevScope dev_(h->cfg.device);
    if ((rc = drain_slots(h))) return rc;
    HIPCHK(hipDeviceSynchronize());
    return work();
}
int height_refusal(const kfpos_handle *h, const char *who, const double *height) {
    if (!height || h->cfg.model == KFPOS_MODEL_PLANAR) return KFPOS_OK;
    g_err = std::string(who) + ": height belongs to KFPOS_MODEL_PLANAR";
    return KFPOS_ERR_MODEL;
}

/* n records of `rec` bytes through the route's block (Route::block), chunk by chunk: chunk(c0, m) stages entries c0 ..
 * c0 + m - 1 at st.dev, launches on the null stream, waits (launched()) and brings down what the call returns */
template <class Chunk>
int by_chunks(Route &st, size_t rec, size_t n, Chunk chunk) {
    int rc = st.block(rec, n);
    for (size_t c0 = 0; !rc && c0 < n; c0 += st.chunk) rc = chunk(c0, std::min(n - c0, st.chunk));
    return rc;
}
/* the chunk's launch has completed: the staging is free again, a mapped block's results are visible */
int launched() {
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(nullptr));
    return KFPOS_OK;
}

/* get / set of the listed tags; the host pointers of absent parts are null */
template <bool STORE>
int tags_transfer(kfpos_handle *h, const int32_t *rows, int32_t n, io<STORE, double> *x, io<STORE, double> *P,
                  io<STORE, uint32_t> *flags, io<STORE, double> *latch, io<STORE, double> *height) {
    TagArgs a;
    tag_args(h, a);
    int cbase[TAG_SECTIONS + 1];
    record_table(h->n, h->full, a.comp, cbase);
    io<STORE, double> *part[TAG_SECTIONS] = {x, P, latch, height};
    size_t wsum = 0;
    for (int s = 0; s < TAG_SECTIONS; ++s) {
        a.cbase[s] = cbase[s];
        a.w[s] = part[s] ? cbase[s + 1] - cbase[s] : 0;
        wsum += (size_t)a.w[s];
    }
    if (wsum == 0 && !flags) return KFPOS_OK;
    /* per listed tag: its values (doubles), its flags word, its row index */
    const size_t rec = wsum * sizeof(double) + sizeof(uint32_t) + sizeof(int32_t);
    Route st = route_of(h);
    /* the sections present behind one another, then the flags words: up for a set, down for a get */
    auto move = [&](size_t c0, size_t m) -> int {
        auto one = [&](auto *p, size_t off, size_t bytes) {
            if constexpr (STORE) return st.up(off, p, bytes);
            else return st.down(p, off, bytes);
        };
        size_t off = 0;
        for (int s = 0; s < TAG_SECTIONS; ++s) {
            if (!a.w[s]) continue;
            HIPCHK(one(part[s] + c0 * a.w[s], off, m * a.w[s] * sizeof(double)));
            off += m * a.w[s] * sizeof(double);
        }
        if (flags) HIPCHK(one(flags + c0, off, m * sizeof(uint32_t)));
        return KFPOS_OK;
    };
    return by_chunks(st, rec, (size_t)n, [&](size_t c0, size_t m) -> int {
        const size_t off_fl = m * wsum * sizeof(double), off_rows = off_fl + m * sizeof(uint32_t);
        HIPCHK(st.up(off_rows, rows + c0, m * sizeof(int32_t)));
        if constexpr (STORE) {
            const int rc = move(c0, m);
            if (rc) return rc;
        }
        a.n = (int)m;
        a.val = (double *)st.dev;
        a.fl = flags ? (uint32_t *)(st.dev + off_fl) : nullptr;
        a.rows = (const int32_t *)(st.dev + off_rows);
        launch_tags(STORE ? TAGS_SCATTER : TAGS_GATHER, h->cfg.storage, nullptr, a);
        const int rc = launched();
        if (rc) return rc;
        if constexpr (STORE) return KFPOS_OK;
        else return move(c0, m);
    });
}

/* kfpos_get_pose_rows / kfpos_get_predicted_rows: out[k] = the caller's k-th array of w[k] doubles per entry (null = not
 * wanted). Staged like the lifecycle calls: per chunk of m entries the list and dt go up, one launch writes the entries'
 * results row-major, and they come down as they are -- nothing here is sized by n_tags. */
int pose_rows_host(kfpos_handle *h, const char *who, const int32_t *rows, int32_t n, const double *dt_ahead, int32_t dt_len,
                   bool predicted, double *const out[3], const int w[3], uint32_t *status) {
    auto refusal = [&]() -> int {
        if (!dt_ahead || (dt_len != 1 && dt_len != n))
            g_err = std::string(who) + (!dt_ahead ? ": dt_ahead == NULL" : ": dt_len = " + std::to_string(dt_len) + " is neither 1 nor n = " + std::to_string(n));
        else if (predicted && (!out[0] || !out[1])) g_err = std::string(who) + (!out[0] ? ": x == NULL" : ": P == NULL");
        else return KFPOS_OK;
        return KFPOS_ERR_ARG;
    };
    return tags_call(h, who, rows, n, false, refusal, [&]() -> int {
        const bool each = dt_len != 1; /* (dt_len == n == 1: the shared value is that entry's) */
        size_t wsum = 0;
        for (int k = 0; k < 3; ++k) wsum += out[k] ? (size_t)w[k] : 0;
        if (wsum == 0 && !status) return KFPOS_OK;
        /* per entry: its results and its dt (doubles), its status word, its row index */
        const size_t rec = (wsum + (each ? 1 : 0)) * sizeof(double) + sizeof(uint32_t) + sizeof(int32_t);
        Route st = route_of(h);
        PoseRowsArgs a = {};
        pose_bank_args(h, a.p);
        a.p.dt_ahead = dt_ahead[0];
        return by_chunks(st, rec, (size_t)n, [&](size_t c0, size_t m) -> int {
            size_t off[3], o = 0;
            double *d[3];
            for (int k = 0; k < 3; ++k) {
                off[k] = o;
                d[k] = out[k] ? (double *)(st.dev + o) : nullptr;
                o += out[k] ? m * w[k] * sizeof(double) : 0;
            }
            const size_t off_dt = o, off_st = off_dt + (each ? m * sizeof(double) : 0), off_rows = off_st + m * sizeof(uint32_t);
            HIPCHK(st.up(off_rows, rows + c0, m * sizeof(int32_t)));
            if (each) HIPCHK(st.up(off_dt, dt_ahead + c0, m * sizeof(double)));
            (predicted ? a.p.full_x : a.p.pos) = d[0];
            (predicted ? a.p.full_P : a.p.cov) = d[1];
            a.p.vel = d[2]; /* (the predicted state has no third array) */
            a.p.dt_each = each ? (const double *)(st.dev + off_dt) : nullptr;
            a.p.status = status ? (uint32_t *)(st.dev + off_st) : nullptr;
            a.rows = (const int32_t *)(st.dev + off_rows);
            a.n = (int)m;
            launch_get_pose_rows(h->cfg.model, h->full != 0, h->cfg.storage, nullptr, a);
            const int rc = launched();
            if (rc) return rc;
            for (int k = 0; k < 3; ++k)
                if (out[k]) HIPCHK(st.down(out[k] + c0 * w[k], off[k], m * w[k] * sizeof(double)));
            if (status) HIPCHK(st.down(status + c0, off_st, m * sizeof(uint32_t)));
            return KFPOS_OK;
        });
    });
}

} // namespace

extern "C" {

/* ---- whole-bank accessors: each its own argument check and refusals, then bank_transfer on a quiet device ---- */
int kfpos_get_state(kfpos_handle *h, double *x, double *P, uint32_t *flags) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    HIPCHK(hipDeviceSynchronize());
    return bank_transfer<false>(h, x, P, flags, nullptr, nullptr);
}

int kfpos_set_state(kfpos_handle *h, const double *x, const double *P, const uint32_t *flags) {
    g_err.clear();
    if (!h) return KFPOS_ERR_ARG;
    DevScope dev_(h->cfg.device);
    HIPCHK(hipDeviceSynchronize());
    const int rc = bank_transfer<true>(h, x, P, flags, nullptr, nullptr);
    if (rc) return rc;
    if (flags) planar_latch_bits(h, flags, h->cfg.n_tags);
    h->stepped = true;
    return KFPOS_OK;
}

int kfpos_latch_dim(const kfpos_handle *h) {
    g_err.clear();
    return h ? latch_width(h->n) : 0;
}

int kfpos_get_latch(kfpos_handle *h, double *latch) { return latch_call<false>(h, latch); }
int kfpos_set_latch(kfpos_handle *h, const double *latch) { return latch_call<true>(h, latch); }
int kfpos_get_height(kfpos_handle *h, double *z) { return height_call<false>(h, z); }
int kfpos_set_height(kfpos_handle *h, const double *z) { return height_call<true>(h, z); }

/* ---- per-tag lifecycle ---- */
int kfpos_get_tags(kfpos_handle *h, const int32_t *rows, int32_t n, double *x, double *P, uint32_t *flags,
                   double *latch, double *height) {
    const char *who = "kfpos_get_tags";
    return tags_call(h, who, rows, n, false, [&] { return height_refusal(h, who, height); },
                     [&] { return tags_transfer<false>(h, rows, n, x, P, flags, latch, height); });
}

int kfpos_set_tags(kfpos_handle *h, const int32_t *rows, int32_t n, const double *x, const double *P,
                   const uint32_t *flags, const double *latch, const double *height) {
    const char *who = "kfpos_set_tags";
    return tags_call(h, who, rows, n, true, [&] { return height_refusal(h, who, height); }, [&]() -> int {
        const int rc = tags_transfer<true>(h, rows, n, x, P, flags, latch, height);
        if (rc) return rc;
        if (flags) planar_latch_bits(h, flags, (size_t)n);
        h->stepped = true;
        return KFPOS_OK;
    });
}

int kfpos_reset_tags(kfpos_handle *h, const int32_t *rows, int32_t n, const double *init_xyz) {
    auto refusal = [&]() -> int {
        if (!init_xyz || h->cfg.use_init_pos) return KFPOS_OK;
        g_err = "kfpos_reset_tags: init_xyz on a handle without a fixed start (use_init_pos = 0): the tag's next epoch is its ML initialisation";
        return KFPOS_ERR_STATE;
    };
    return tags_call(h, "kfpos_reset_tags", rows, n, true, refusal, [&]() -> int {
        TagArgs a;
        tag_args(h, a);
        a.n_comp = fresh_table(h->n, h->psz, a.comp);
        for (int k = 0; k < 3; ++k) a.cst[k] = h->cfg.use_init_pos ? h->cfg.init_pos[k] : NAN;
        a.cst[3] = h->planar.fixed_height; /* mUWBtagZ / mAngle as kfpos_set_planar wrote them (0 / 0 if it never ran) */
        a.cst[4] = h->planar.init_angle;
        /* per listed tag: its start position (if given), its row index */
        const size_t rec = (init_xyz ? 3 * sizeof(double) : 0) + sizeof(int32_t);
        Route st = route_of(h);
        return by_chunks(st, rec, (size_t)n, [&](size_t c0, size_t m) -> int {
            const size_t off_rows = init_xyz ? m * 3 * sizeof(double) : 0;
            HIPCHK(st.up(off_rows, rows + c0, m * sizeof(int32_t)));
            if (init_xyz) HIPCHK(st.up(0, init_xyz + c0 * 3, m * 3 * sizeof(double)));
            a.n = (int)m;
            a.init = init_xyz ? (const double *)st.dev : nullptr;
            a.rows = (const int32_t *)(st.dev + off_rows);
            launch_tags(TAGS_RESET, h->cfg.storage, nullptr, a);
            return launched();
        });
    });
}

/* ---- pose for a row list ---- */
int kfpos_get_pose_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const double *dt_ahead, int32_t dt_len,
                        double *pos, double *cov3x3, double *vel, uint32_t *status) {
    double *const out[3] = {pos, cov3x3, vel};
    const int w[3] = {3, 9, 3};
    return pose_rows_host(h, "kfpos_get_pose_rows", rows, n, dt_ahead, dt_len, false, out, w, status);
}

int kfpos_get_predicted_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const double *dt_ahead, int32_t dt_len,
                             double *x, double *P, uint32_t *status) {
    double *const out[3] = {x, P, nullptr};
    const int w[3] = {h ? h->n : 0, h ? h->n * h->n : 0, 0};
    return pose_rows_host(h, "kfpos_get_predicted_rows", rows, n, dt_ahead, dt_len, true, out, w, status);
}

} // extern "C"
