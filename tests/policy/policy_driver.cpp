/* policy_driver.cpp -- roskfpos_amd/csrc/kfpos_policy.h against the rules of kfpos_create written out here in words (not
 * computed with the header's helpers), and roskfpos_amd/csrc/kfpos_owned.h against counting stand-ins for allocate and
 * release. `policy_driver <section>` prints "OK <section> <checks>" or the first disagreement. tests/test_policy.py builds
 * it with the address and undefined-behaviour sanitizers; no GPU, no library. */
#include <cstdio>
#include <cstring>
#include <utility>

#include "kfpos_owned.h"
#include "kfpos_policy.h"

using namespace kfpos_policy;

/* ---- the environment of a call: nine variables, each unset (null) or a text ---- */
static const char *const var_name[9] = {"KFPOS_GENERIC_KERNEL", "KFPOS_ONE_WAVE_BUILD", "KFPOS_PAIR9", "KFPOS_PAIR9_MEET", "KFPOS_IMU9_DIAG",
                                        "KFPOS_NO_COOP", "KFPOS_TRACE_CHUNK_STEPS", "KFPOS_SMALL_BANK_ELEMS", "KFPOS_SLOT_SPLIT_BYTES"};
enum { GENERIC, ONE_WAVE, PAIR9, MEET, DIAG, NO_COOP, CHUNK, SMALL, SPLIT, N_VARS };
static const char *var_value[N_VARS];
static int reads[N_VARS]; /* since clear_env() */
static const char *fake_env(const char *name) {
    for (int v = 0; v < N_VARS; ++v)
        if (std::strcmp(name, var_name[v]) == 0) return ++reads[v], var_value[v];
    std::printf("FAIL the policy asked for %s, which is none of its nine variables\n", name);
    std::exit(1);
}
static void clear_env() {
    for (int v = 0; v < N_VARS; ++v) var_value[v] = nullptr, reads[v] = 0;
}
static const char *const four[4] = {nullptr, "", "0", "1"}; /* unset, empty, 0, 1 */
static const char *shown(const char *v) { return v ? v : "(unset)"; }

static kfpos_config config(int model, int storage, int n_tags, int max_anchors, int use_init_pos, int ignore_worst, int top_n, int ml_variant) {
    kfpos_config c;
    std::memset(&c, 0, sizeof(c));
    c.model = model;
    c.storage = storage;
    c.n_tags = n_tags;
    c.max_anchors = max_anchors;
    c.use_init_pos = use_init_pos;
    c.ignore_worst = ignore_worst;
    c.top_n = top_n;
    c.ml_variant = ml_variant;
    return c;
}

static bool is_one(const char *v) { return v && v[0] == '1'; }

static int sweep() {
    const int models[4] = {KFPOS_MODEL_TOA, KFPOS_MODEL_TOA_IMU, KFPOS_MODEL_ML, KFPOS_MODEL_PLANAR};
    const int storages[4] = {KFPOS_STORE_F64, KFPOS_STORE_F32, KFPOS_STORE_MIXED, KFPOS_STORE_P48};
    const int anchors[4] = {7, 8, 9, 16};
    const int variants[3] = {KFPOS_ML_NORMAL, KFPOS_ML_IGNORE_N, KFPOS_ML_BEST};
    const long slots[3] = {0, 4, 1024};
    /* what the three numeric variables give for unset, empty, 0, 1 */
    const int chunk_of[4] = {128, 1, 1, 1};
    const size_t small_of[4] = {4096, 0, 0, 1}, split_of[4] = {0, 0, 0, 1};
    long accepted = 0, checks = 0;
    for (int model : models)
    for (int storage : storages)
    for (int A : anchors)
    for (int bits = 0; bits < 8; ++bits)
    for (int variant : variants)
    for (long S : slots)
    for (int k = 0; k < 5; ++k) {
        const long tags[5] = {1, 8192, 8193, 64 * S, 64 * S + 1};
        const bool fixed = !(bits & 1), loo = (bits & 2) != 0, topn = (bits & 4) != 0;
        const kfpos_config cfg = config(model, storage, (int)tags[k], A, fixed, loo, topn ? 2 : 0, variant);
        const bool toa = model == KFPOS_MODEL_TOA, ml = model == KFPOS_MODEL_ML;
        /* kfpos_create takes it: a tag at least, the ML estimator's variants for the ML estimator, leave-one-out for the
         * 6-state filter, top-N for the 6-state filter and the ML estimator */
        const bool takes = tags[k] >= 1 && (variant == KFPOS_ML_NORMAL || ml) && (!loo || toa) && (!topn || toa || ml);
        if ((config_refusal(cfg) == nullptr) != takes) {
            std::printf("FAIL config_refusal: model=%d storage=%d tags=%ld anchors=%d fixed=%d loo=%d topn=%d variant=%d: %s\n", model, storage,
                        tags[k], A, fixed, loo, topn, variant, shown(config_refusal(cfg)));
            return 1;
        }
        if (!takes) continue;
        ++accepted;
        /* one variable at a time through unset, empty, 0, 1 (setting 0 = all unset), then all of them at once -- but for
         * KFPOS_PAIR9_MEET, whose 0 and 1 are refusals -- at empty, 0, 1 */
        for (int setting = 0; setting < 1 + N_VARS * 3 + 3; ++setting) {
            clear_env();
            int val[N_VARS] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
            if (setting > N_VARS * 3) {
                for (int v = 0; v < N_VARS; ++v) val[v] = v == MEET ? 0 : setting - N_VARS * 3;
            } else if (setting > 0) val[(setting - 1) / 3] = 1 + (setting - 1) % 3;
            for (int v = 0; v < N_VARS; ++v) var_value[v] = four[val[v]];
            Policy p;
            std::memset(&p, 1, sizeof(p));
            const bool ok = policy(cfg, (size_t)S, fake_env, &p);
            /* the table, in the words of the rules */
            const bool full = toa && !fixed;                                          /* ML start: the non-symmetric layout */
            const bool generic = is_one(var_value[GENERIC]) || (full && loo && storage == KFPOS_STORE_P48);
            const bool two = !is_one(var_value[ONE_WAVE]) && S != 0 && (tags[k] + 63) / 64 > S; /* more wavefronts than slots */
            const bool pair9 = val[PAIR9] >= 2 ? val[PAIR9] == 3 : (storage == KFPOS_STORE_MIXED || storage == KFPOS_STORE_P48);
            const bool diag = val[DIAG] != 2;                                         /* off at 0 only */
            const bool coop = !is_one(var_value[NO_COOP]) && !generic && toa && fixed && !loo && !topn && A <= 8 && tags[k] <= 8192;
            const bool meet_ok = val[MEET] < 2;                                       /* "0" and "1" are not first,dense_until */
            const char *why = nullptr;
            if (ok != meet_ok) why = "accepted / refused";
            else if (!ok) why = nullptr;
            else if (p.force_generic != generic) why = "force_generic";
            else if (p.two_waves != two) why = "two_waves";
            else if (p.pair9 != pair9) why = "pair9";
            else if (p.pair9_first != 8 || p.pair9_dense_until != 10) why = "pair9_first, pair9_dense_until";
            else if (p.imu9_diag != diag) why = "imu9_diag";
            else if (p.coop != coop) why = "coop";
            else if (p.trace_chunk != chunk_of[val[CHUNK]]) why = "trace_chunk";
            else if (p.small_bank_elems != small_of[val[SMALL]]) why = "small_bank_elems";
            else if (p.slot_split_bytes != split_of[val[SPLIT]]) why = "slot_split_bytes";
            for (int v = 0; v < N_VARS && ok && !why; ++v)
                if (reads[v] != 1) why = "every variable is read once";
            /* the invariant: what the handle can hand the plan, before and after a sensor sample, with coop and without
             * (kfpos_set_anchor_cells), is producible */
            for (int s = 0; s < 4 && ok && !why; ++s) {
                Policy q = p;
                if (s & 2) q.coop = false;
                if ((s & 1) && model != KFPOS_MODEL_PLANAR) continue;
                if (!producible(plan_inputs(cfg, q, full, (s & 1) != 0))) why = "producible(plan_inputs(...))";
            }
            if (why) {
                std::printf("FAIL %s: model=%d storage=%d tags=%ld anchors=%d fixed=%d loo=%d topn=%d variant=%d slots=%ld\n", why, model, storage,
                            tags[k], A, fixed, loo, topn, variant, S);
                for (int v = 0; v < N_VARS; ++v) std::printf("  %s=%s\n", var_name[v], shown(var_value[v]));
                std::printf("  policy: generic=%d two_waves=%d pair9=%d meet=%d,%d diag=%d coop=%d chunk=%d small=%zu split=%zu\n", p.force_generic,
                            p.two_waves, p.pair9, p.pair9_first, p.pair9_dense_until, p.imu9_diag, p.coop, p.trace_chunk, p.small_bank_elems,
                            p.slot_split_bytes);
                return 1;
            }
            ++checks;
        }
    }
    std::printf("OK sweep %ld %ld\n", accepted, checks);
    return 0;
}

/* KFPOS_PAIR9_MEET as the sscanf("%d,%d%c") == 2 rule of kfpos_create reads it, then 1 <= first <= dense_until <= 20 */
static int meet() {
    const struct {
        const char *text;
        bool ok;
        int first, dense_until;
    } cases[12] = {{nullptr, true, 8, 10}, {"", true, 8, 10},   {"8,10", true, 8, 10}, {"8,8", true, 8, 8},
                   {"1,1", true, 1, 1},    {"20,20", true, 20, 20}, {"0,5", false, 0, 0}, {"9,8", false, 0, 0},
                   {"8,21", false, 0, 0},  {"8", false, 0, 0},  {"8,10x", false, 0, 0}, {",", false, 0, 0}};
    const kfpos_config cfg = config(KFPOS_MODEL_TOA_IMU, KFPOS_STORE_MIXED, 130, 8, 1, 0, 0, KFPOS_ML_NORMAL);
    for (const auto &c : cases) {
        clear_env();
        var_value[MEET] = c.text;
        Policy p;
        std::memset(&p, 1, sizeof(p));
        const bool ok = policy(cfg, 1024, fake_env, &p);
        if (ok != c.ok || (ok && (p.pair9_first != c.first || p.pair9_dense_until != c.dense_until))) {
            std::printf("FAIL KFPOS_PAIR9_MEET=%s: %s, %d,%d\n", shown(c.text), ok ? "accepted" : "refused", p.pair9_first, p.pair9_dense_until);
            return 1;
        }
    }
    if (std::strcmp(PAIR9_MEET_REFUSAL, "KFPOS_PAIR9_MEET must be first,dense_until with 1 <= first <= dense_until <= 20") != 0) {
        std::printf("FAIL the refusal's text: %s\n", PAIR9_MEET_REFUSAL);
        return 1;
    }
    /* the argument check of kfpos_pair9_meet_points */
    if (!pair9_meet_ok(1, 1) || !pair9_meet_ok(8, 10) || !pair9_meet_ok(20, 20) || pair9_meet_ok(0, 5) || pair9_meet_ok(9, 8) || pair9_meet_ok(8, 21) ||
        PAIR9_MEET_FIRST != 8 || PAIR9_MEET_DENSE_UNTIL != 10 || PAIR9_MEET_MAX != 20) {
        std::printf("FAIL pair9_meet_ok / PAIR9_MEET_*\n");
        return 1;
    }
    std::printf("OK meet 12\n");
    return 0;
}

static int chunk() {
    const struct {
        const char *text;
        int chunk;
    } cases[6] = {{nullptr, 128}, {"0", 1}, {"1", 1}, {"128", 128}, {"129", 128}, {"abc", 1}};
    const kfpos_config cfg = config(KFPOS_MODEL_TOA, KFPOS_STORE_F64, 130, 8, 1, 0, 0, KFPOS_ML_NORMAL);
    for (const auto &c : cases) {
        clear_env();
        var_value[CHUNK] = c.text;
        Policy p;
        if (!policy(cfg, 1024, fake_env, &p) || p.trace_chunk != c.chunk) {
            std::printf("FAIL KFPOS_TRACE_CHUNK_STEPS=%s: %d, not %d\n", shown(c.text), p.trace_chunk, c.chunk);
            return 1;
        }
    }
    std::printf("OK chunk 6\n");
    return 0;
}

/* one configuration per refusal, in kfpos_create's order, each otherwise acceptable; then two at once: the earlier text */
static int refusal() {
    const kfpos_config good = config(KFPOS_MODEL_TOA, KFPOS_STORE_F64, 130, 8, 1, 0, 0, KFPOS_ML_NORMAL);
    struct Case {
        kfpos_config cfg;
        const char *text;
    } cases[12];
    int n = 0;
    auto add = [&](const char *text) -> kfpos_config & {
        cases[n].cfg = good;
        cases[n].text = text;
        return cases[n++].cfg;
    };
    add(nullptr);
    add("kfpos_config.model is not one of KFPOS_MODEL_*").model = 4;
    add("kfpos_config.storage is not one of KFPOS_STORE_*").storage = -1;
    add("kfpos_config.n_tags must be >= 1").n_tags = 0;
    add("kfpos_config.max_anchors must be 1..64 (MAX_NUM_ANCS, Posgenerator.h:74)").max_anchors = 65;
    add("kfpos_config.max_anchors must be 1..64 (MAX_NUM_ANCS, Posgenerator.h:74)").max_anchors = 0;
    add("kfpos_config.top_n must be >= 0").top_n = -1;
    add("kfpos_config.ml_variant is not one of KFPOS_ML_*").ml_variant = 3;
    add("kfpos_config.ml_variant belongs to KFPOS_MODEL_ML (MLLocation's variants, MLLocation.h:5-7)").ml_variant = KFPOS_ML_BEST;
    {
        kfpos_config &c = add("ignore_worst exists for the 6-state filter only, top_n for the 6-state filter and the ML estimator");
        c.model = KFPOS_MODEL_TOA_IMU;
        c.top_n = 2;
    }
    {
        kfpos_config &c = add("ignore_worst exists for the 6-state filter only, top_n for the 6-state filter and the ML estimator");
        c.model = KFPOS_MODEL_ML;
        c.ignore_worst = 1;
    }
    { /* no tags and too many anchors: the tags are looked at first */
        kfpos_config &c = add("kfpos_config.n_tags must be >= 1");
        c.n_tags = 0;
        c.max_anchors = 65;
    }
    static_assert(KFPOS_MODEL_PLANAR == 3 && KFPOS_ML_BEST == 2, "4 is no model, 3 no variant");
    for (int i = 0; i < n; ++i) {
        const char *why = config_refusal(cases[i].cfg);
        if ((why == nullptr) != (cases[i].text == nullptr) || (why && std::strcmp(why, cases[i].text) != 0)) {
            std::printf("FAIL config_refusal, case %d: %s, not %s\n", i, shown(why), shown(cases[i].text));
            return 1;
        }
    }
    std::printf("OK refusal %d\n", n);
    return 0;
}

/* ---- the owner: stand-ins that count ---- */
static int acquired, released;
static int *acquire() { return new int(++acquired); }
static int give_back(int *p) {
    ++released;
    delete p;
    return 0;
}
static void acquire_into(int **out) { *out = acquire(); }
using Own = kfpos_owned::Owned<int *, give_back>;

#define EXPECT(cond)                                                                                   \
    do {                                                                                               \
        if (!(cond)) {                                                                                 \
            std::printf("FAIL owned, line %d: %s (acquired %d, released %d)\n", __LINE__, #cond, acquired, released); \
            return 1;                                                                                  \
        }                                                                                              \
    } while (0)

static int owned() {
    {
        Own nothing; /* null is never released */
        EXPECT(!nothing);
        nothing.reset();
        Own moved(std::move(nothing));
        moved = Own();
    }
    EXPECT(acquired == 0 && released == 0);
    {
        Own a(acquire()); /* the destructor releases once */
        int *raw = a;     /* ... and the owner reads as the raw handle */
        EXPECT(raw && *raw == 1 && *a == 1 && released == 0);
    }
    EXPECT(released == 1);
    {
        Own a(acquire());
        int *raw = a;
        Own b(std::move(a)); /* move construction hands it over */
        EXPECT(!a && b == raw && released == 1);
        Own c(acquire());
        int *raw_c = c;
        b = std::move(c); /* move assignment releases what the target held, then hands over */
        EXPECT(released == 2 && !c && b == raw_c);
        Own &same = b;
        b = std::move(same); /* self-move is harmless */
        EXPECT(released == 2 && b == raw_c);
    }
    EXPECT(released == 3);
    {
        Own a(acquire());
        a.reset(acquire()); /* reset releases the old value */
        EXPECT(released == 4 && *a == 5);
        int *mine = a.release(); /* release does not */
        EXPECT(released == 4 && !a && *mine == 5);
        give_back(mine); /* (the caller's now) */
        a.reset();
        EXPECT(released == 5);
        acquire_into(a.out()); /* out(): where an allocating call writes */
        EXPECT(*a == 6 && released == 5);
        acquire_into(a.out()); /* ... and what was held goes first */
        EXPECT(*a == 7 && released == 6);
    }
    {
        Own two[2]; /* members of an array, as the communicator's buffer sets */
        for (Own &o : two) acquire_into(o.out());
        two[0].reset();
        EXPECT(released == 8 && !two[0] && two[1]);
    }
    EXPECT(acquired == 9 && released == 9); /* as many releases as acquisitions at exit */
    std::printf("OK owned %d\n", released);
    return 0;
}

int main(int argc, char **argv) {
    const char *what = argc > 1 ? argv[1] : "";
    if (!std::strcmp(what, "sweep")) return sweep();
    if (!std::strcmp(what, "meet")) return meet();
    if (!std::strcmp(what, "chunk")) return chunk();
    if (!std::strcmp(what, "refusal")) return refusal();
    if (!std::strcmp(what, "owned")) return owned();
    std::printf("usage: policy_driver sweep|meet|chunk|refusal|owned\n");
    return 2;
}
