/* kfpos_k_toa6each.inc -- k_trace_toa6_each: ranging slots of the 6-state filter in one launch in which every tag has a
 * timeline of its own (kfpos_run_trace_each_dev), included by kfpos_k_toa6eachs.hip (symmetric covariance layout: fixed
 * start) and kfpos_k_toa6eachf.hip (full layout: ML initialisation), which instantiate one half each.
 * Every slot is a ranging epoch; who takes part in it, and at which timeLag, is per tag: dt_each[e][t] < 0 means tag t
 * sits slot e out, exactly as k_step_toa6 treats a per-tag dt array (KFPOS_ST_SKIPPED, nothing of the tag changes). The
 * state stays in registers from slot to slot and every slot a tag runs is the unchanged step_toa6<SYMM, HEUR>
 * (kfpos_core_toa6.h) on an epoch staged as k_step_toa6 stages it, so the launch computes bit for bit what as many
 * kfpos_step_toa_dev launches with that dt array would. k_step_toa6 with n_steps > 1 (kfpos_run_trace_dev) is the form
 * with one timeline for all tags. */
/* AS as in k_step_toa6: 8 = the epoch in registers, -8 / -16 = compile-time anchor loops over an LDS-resident epoch,
 * 0 = run-time loop. No occupancy is asked for: a bank of up to 65 536 tags is one wavefront per SIMD.
 * Fetching ahead: a lane's dt is fetched one slot AHEAD in every form (two registers; the participation branch hangs on
 * it), and so is the register-resident epoch (AS = 8), for every lane whoever takes part -- as k_step_toa6 fetches its
 * next epoch. The LDS forms stage their epoch where the slot runs, the whole wavefront, absent lanes included (their
 * entries are loaded and never used): LDS holds one epoch. */
template <bool SYMM, typename REAL, typename MREAL, int AS, int HEUR = 2>
__global__ __launch_bounds__(WAVE) void k_trace_toa6_each(const kfpos_k::TraceEachArgs ev) {
    extern __shared__ double lds[];
    const KArgs &a = ev.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    const Params pr = make_params(a);
    constexpr int NA = AS > 0 ? AS : 1;
    /* step_toa6's PEEL, as in k_step_toa6: here both 8-anchor forms with both heuristics spill inside the slot loop
     * with the peeled Gauss-Newton text and keep the unpeeled one */
    constexpr bool PEEL = !((AS == 8 || AS == -8) && HEUR == 2);
    constexpr int SZ = Cov<6, SYMM>::SZ;
    const int n = a.n_steps;
    auto load_dt = [&](int e) -> double { return (ev.dt_each + (size_t)e * T)[(uint32_t)opaque_lane(t)]; };

    /* load order = order of first use, the flags word in front (k_step_toa6) */
    const auto fl0 = a.flags[t32];
    double dt_next = load_dt(0);
    RawEpoch<MREAL, NA> raw;
    if constexpr (AS > 0) fetch_epoch<MREAL, AS>(a, t, 0, raw);
    Tag6<SYMM> tg;
#pragma unroll
    for (int k = 0; k < 3; ++k) tg.pos[k] = (a.pos + k * T)[t32];
#pragma unroll
    for (int k = 0; k < SZ; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, SZ, T, t32);

    bool ran = false; /* per lane: a slot of this launch ran on this lane */
    for (int e = 0; e < n; ++e) {
        const double dt = dt_next;
        const bool more = e + 1 < n;
        if (more) dt_next = load_dt(opaque_uniform(e + 1));
        const uint32_t tl = (uint32_t)opaque_lane(t);
        const bool run = !(dt < 0.0); /* THE predicate of the single calls: a NaN dt runs the slot */
        const bool last_status = !more && a.status;
        /* A wavefront in which nobody has anything in this slot passes it uniformly: no staging, no step -- only the
         * rows every slot writes, below. (One way round the loop, as in k_events_planar_each.) */
        const bool any = __builtin_amdgcn_ballot_w64(run) != 0; /* wave-uniform */
        uint32_t s = ST_SKIPPED; /* the lane sits the slot out: what skipped_lane() reports */
        if (any) {
            if constexpr (AS > 0) {
                RegScratch<AS> sc;
                unpack_epoch<MREAL, AS>(raw, sc);
                if (more) fetch_epoch<MREAL, AS>(a, tl, opaque_uniform(e + 1), raw); /* next slot in flight */
                if (run) s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt);
            } else if constexpr (AS < 0 && sizeof(MREAL) == 4) { /* compile-time count, epoch in LDS, 4-byte errorEstimations */
                StaticScratchF<-AS> sc = stage_epoch_lds_nf<-AS>(a, lds, lane, tl, opaque_uniform(e));
                if (run) s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt, lds + static_epoch_doubles<MREAL, -AS>() + lane, WAVE);
            } else if constexpr (AS < 0) { /* compile-time count, epoch in LDS */
                StaticScratch<-AS> sc = stage_epoch_lds_n<MREAL, -AS>(a, lds, lane, tl, opaque_uniform(e));
                if (run) s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt, lds + static_epoch_doubles<MREAL, -AS>() + lane, WAVE);
            } else {
                Scratch sc = stage_epoch_lds<MREAL>(a, lds, lane, tl, opaque_uniform(e));
                if (run) s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt, lds + 3 * (size_t)a.A * WAVE + lane, WAVE);
            }
            ran |= run;
        } else {
            if constexpr (AS > 0) {
                if (more) fetch_epoch<MREAL, AS>(a, tl, opaque_uniform(e + 1), raw);
            }
        }
        if (a.traj) { /* the pose a per-slot caller would have read back; a lane that sat out: the untouched position */
#pragma unroll
            for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[tl] = tg.pos[k];
        }
        if (ev.status_events || last_status) { /* the status word a single call would have returned for this slot */
            if (any) {
                bool fin = true;
#pragma unroll
                for (int k = 0; k < 3; ++k) fin &= isfinite(tg.pos[k]);
#pragma unroll
                for (int k = 0; k < SZ; ++k) fin &= isfinite(tg.P.a[k]);
                const bool waiting = !a.use_init_pos && isnan(tg.pos[0]); /* still waiting for its ML initialisation (open text: nonfinite_state() here changes the kernel's code) */
                if (run && !fin && !waiting) s |= ST_NONFINITE;
            }
            if (ev.status_events) (ev.status_events + (size_t)opaque_uniform(e) * T)[tl] = s;
            if (last_status) a.status[tl] = s;
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what the single launch of this slot would have kept in HBM */
            if (more && run) { /* only lanes that ran it */
#pragma unroll
                for (int k = 0; k < SZ; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }

    if (!ran) return; /* a tag that ran nothing keeps every stored byte, FL_STARTED and compact covariance planes included */
    const uint32_t ts = (uint32_t)opaque_lane(t); /* (offsets re-formed, not held across the loop) */
#pragma unroll
    for (int k = 0; k < 3; ++k) (a.pos + k * T)[ts] = tg.pos[k];
#pragma unroll
    for (int k = 0; k < SZ; ++k) stcov<REAL>(a.P, k, SZ, T, ts, tg.P.a[k]);
    a.flags[ts] = fl0 | FL_STARTED;
}

/* k_trace_toa6_each as a family of toa6_table (kfpos_kernels.h) */
struct TraceToa6Each {
    template <bool SYMM, typename REAL, typename MREAL, int AS, int HEUR>
    static constexpr kfpos_k::trace_each_kernel_t kernel() { return k_trace_toa6_each<SYMM, REAL, MREAL, AS, HEUR>; }
};
template <bool SYMM, typename REAL, typename MREAL>
kfpos_k::trace_each_kernel_t toa6_each_kernel(int as, int heur) { return toa6_table<TraceToa6Each, SYMM, REAL, MREAL>(as, heur); }
