/* kfpos_k_toa6.inc -- the 6-state step kernels (KalmanFilterTOA.cpp:70-156), included by kfpos_k_toa6s.hip (symmetric
 * covariance layout: fixed start) and kfpos_k_toa6f.hip (full layout: ML initialisation), which instantiate one half each,
 * and by kfpos_k_cells6s.hip / kfpos_k_cells6f.hip, which instantiate the same halves around CellArgs (anchor cells) */
/* ------------------------------------------------------------------ 6-state step kernel */
/* amdgpu_waves_per_eu(1, 2): never trade registers for a third wave per SIMD -- the LDS-resident 16-anchor variant
 * fits in 137-150 VGPRs when asked to (e.g. when pinned to two waves), and then runs 3-11 % slower than with the ~250 it
 * takes at two waves (measured again in round 3: 96.2 against 93.6 us per epoch). But the symmetric-layout 16-anchor
 * variants (BASELINE configs[4]: 262 144 tags = 4 wavefronts per SIMD) must not fall back to ONE wave either, and left the
 * choice the compiler once gave the 48-bit-covariance instantiation 255 + 2 registers -- two more than fit twice: 118
 * instead of 95 us per epoch, and no test noticed. The two registers were the second per-lane offset that storage mode
 * holds (two planes): the 16-anchor kernels re-form their offsets at the end of the launch instead of holding them across
 * the step (`ts` below), which leaves every instantiation at 251-253 registers, and `make check` verifies the occupancy of
 * every kernel that is meant to share a SIMD (tools/check_scratch.py --min-occupancy). */
/* ARGS: the argument block. KArgs: the anchor table is KArgs::anchors. CellArgs (a bank with anchor cells,
 * kfpos_set_anchor_cells; kfpos_k_cells6s.hip / kfpos_k_cells6f.hip instantiate these): the table of the workgroup's
 * cell -- the one line below that asks. step_toa6, the staging helpers and the order of every load and store are the
 * same text, so a block of cell c computes bit for bit what its rows compute with cell c's table in KArgs::anchors.
 * The parameter is the block itself and is named wherever a field is read: behind a reference to it, or inside a
 * function that both forms call, every KArgs instantiation came out with other code. */
template <bool SYMM, typename REAL, typename MREAL, int AS, int HEUR = 2, class ARGS = KArgs>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(1, 2))) void k_step_toa6(const ARGS a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    Params pr = make_params(a);
    if constexpr (cells_block<ARGS>) pr.anchors = cell_anchors(a);
    constexpr int NA = AS > 0 ? AS : 1;
    /* The Gauss-Newton solves in ml_estimate's peeled text (step_toa6's PEEL). The 8-anchor LDS form with both
     * heuristics -- up to 65 solves around one inlined solver -- spills inside its loops with it and keeps the
     * unpeeled text (make check's scratch rule decides). */
    constexpr bool PEEL = !(AS == -8 && HEUR == 2);
    if (a.n_steps == 1 && a.dt && a.dt[t] < 0.0) { /* no epoch for this tag in this call */
        skipped_lane(a, t, true);
        return;
    }

    /* Load order = order of first use: epoch and position feed the ML solve, the covariance is first
     * touched after it (step_toa6), so its 21-36 loads stay in flight behind ~2-3 k instructions. The flags word is
     * read here, in front of them, and written back behind the last store: read there (flags |= ...) its load was a
     * round trip of its own at the very end of every launch, with the wavefront holding its SIMD slot meanwhile. */
    const auto fl0 = a.flags[t];
    RawEpoch<MREAL, NA> raw;
    if constexpr (AS > 0) fetch_epoch<MREAL, AS>(a, t, 0, raw);
    Tag6<SYMM> tg;
#pragma unroll
    for (int k = 0; k < 3; ++k) tg.pos[k] = (a.pos + k * T)[t32];
#pragma unroll
    for (int k = 0; k < Cov<6, SYMM>::SZ; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, Cov<6, SYMM>::SZ, T, t32);

    uint32_t s = 0;
    for (int e = 0; e < a.n_steps; ++e) { /* the state stays in registers from epoch to epoch */
        const double dt = epoch_dt(a, t, e);
        if constexpr (AS > 0) {
            RegScratch<AS> sc;
            unpack_epoch<MREAL, AS>(raw, sc);
            if (e + 1 < a.n_steps) fetch_epoch<MREAL, AS>(a, t, e + 1, raw); /* next epoch in flight */
            s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt);
        } else if constexpr (AS < 0 && sizeof(MREAL) == 4) { /* compile-time count, epoch in LDS, 4-byte errorEstimations */
            StaticScratchF<-AS> sc = stage_epoch_lds_nf<-AS>(a, lds, lane, t, e);
            s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt, lds + static_epoch_doubles<MREAL, -AS>() + lane, WAVE);
        } else if constexpr (AS < 0) { /* compile-time count, epoch in LDS */
            StaticScratch<-AS> sc = stage_epoch_lds_n<MREAL, -AS>(a, lds, lane, t, e);
            s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt, lds + static_epoch_doubles<MREAL, -AS>() + lane, WAVE);
        } else {
            Scratch sc = stage_epoch_lds<MREAL>(a, lds, lane, t, e);
            s = step_toa6<SYMM, HEUR, 0, PEEL>(tg, sc, pr, dt, lds + 3 * (size_t)a.A * WAVE + lane, WAVE);
        }
        if (a.traj) { /* the pose a per-epoch caller would have read back (getPose at timeLag 0) */
#pragma unroll
            for (int k = 0; k < 3; ++k) (a.traj + ((size_t)e * 3 + k) * T)[t32] = tg.pos[k];
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what n single-epoch launches would have kept in HBM */
            if (e + 1 < a.n_steps) {
#pragma unroll
                for (int k = 0; k < Cov<6, SYMM>::SZ; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }

    bool fin = true;
    const uint32_t ts = AS == -16 ? (uint32_t)opaque_lane(t) : t32; /* (offsets re-formed, not held across the step) */
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        (a.pos + k * T)[ts] = tg.pos[k];
        fin &= isfinite(tg.pos[k]);
    }
#pragma unroll
    for (int k = 0; k < Cov<6, SYMM>::SZ; ++k) {
        stcov<REAL>(a.P, k, Cov<6, SYMM>::SZ, T, ts, tg.P.a[k]);
        fin &= isfinite(tg.P.a[k]);
    }
    if (nonfinite_state(fin, a.use_init_pos, tg.pos[0])) s |= ST_NONFINITE;
    a.flags[t] = fl0 | FL_STARTED;
    if (a.status) a.status[t] = s;
}

/* The plain 8-anchor 6-state step (symmetric layout, no outlier heuristic) in at most 256 registers, for banks with
 * more wavefronts than the chip has SIMDs (> 65 536 tags). Left to itself the compiler gives the register-resident
 * kernel above 305 registers: one wavefront per SIMD, which is all a bank of up to 65 536 tags can use -- but a bank
 * of 131 072 tags (BASELINE configs[3] on 8 GPUs) then runs as two rounds of one wavefront per SIMD instead of one
 * round of two that fill each other's idle cycles. Here the epoch sits in LDS ([anchor][lane], compile-time loops 8
 * wide as above) and most of the covariance joins it while the ML solve runs (step_toa6<..., PARKN>): 19.5 KB per
 * wavefront, eight wavefronts per CU. Same arithmetic, same bits (tests/test_two_waves_gpu.py). */
template <typename MREAL>
constexpr int toa6_w2_park() { return kfpos_plan::toa6_w2_park(sizeof(MREAL)); } /* what 160 KB / 8 leave next to the epoch */
template <typename REAL, typename MREAL>
__global__ __launch_bounds__(WAVE) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_step_toa6_w2(const KArgs a) {
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    const Params pr = make_params(a);
    if (a.n_steps == 1 && a.dt && a.dt[t] < 0.0) { /* no epoch for this tag in this call */
        skipped_lane(a, t, true);
        return;
    }
    const auto fl0 = a.flags[t]; /* (read in front of the state loads, written back at the end: see k_step_toa6) */
    Tag6<true> tg;
#pragma unroll
    for (int k = 0; k < 3; ++k) tg.pos[k] = (a.pos + k * T)[t32];
#pragma unroll
    for (int k = 0; k < Cov<6, true>::SZ; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, Cov<6, true>::SZ, T, t32);
    double *park = lds + static_epoch_doubles<MREAL, 8>() + lane;
    constexpr int PARKN = toa6_w2_park<MREAL>();
    uint32_t s = 0;
    for (int e = 0; e < a.n_steps; ++e) {
        const double dt = epoch_dt(a, opaque_lane(t), e);
        if constexpr (sizeof(MREAL) == 4) {
            StaticScratchF<8> sc = stage_epoch_lds_nf<8>(a, lds, lane, opaque_lane(t), opaque_uniform(e));
            s = step_toa6<true, 0, PARKN>(tg, sc, pr, dt, park, WAVE);
        } else {
            StaticScratch<8> sc = stage_epoch_lds_n<MREAL, 8>(a, lds, lane, opaque_lane(t), opaque_uniform(e));
            s = step_toa6<true, 0, PARKN>(tg, sc, pr, dt, park, WAVE);
        }
        if (a.traj) {
#pragma unroll
            for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what n single-epoch launches would have kept in HBM */
            if (e + 1 < a.n_steps) {
#pragma unroll
                for (int k = 0; k < Cov<6, true>::SZ; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        (a.pos + k * T)[t32] = tg.pos[k];
        fin &= isfinite(tg.pos[k]);
    }
#pragma unroll
    for (int k = 0; k < Cov<6, true>::SZ; ++k) {
        stcov<REAL>(a.P, k, Cov<6, true>::SZ, T, t32, tg.P.a[k]);
        fin &= isfinite(tg.P.a[k]);
    }
    if (!fin) s |= ST_NONFINITE; /* (a symmetric-layout bank has a fixed start: no tag waits for an initialisation) */
    a.flags[t] = fl0 | FL_STARTED;
    if (a.status) a.status[t] = s;
}

/* k_step_toa6 around one argument block, as a family of toa6_table (kfpos_kernels.h) */
template <class ARGS>
struct StepToa6 {
    template <bool SYMM, typename REAL, typename MREAL, int AS, int HEUR>
    static constexpr auto kernel() -> void (*)(const ARGS) { return k_step_toa6<SYMM, REAL, MREAL, AS, HEUR, ARGS>; }
};
/* the table, and in front of it the two-wavefront build, which only the plain step has */
template <bool SYMM, typename REAL, typename MREAL>
step_kernel_t toa6_kernel(int as, int heur, bool two_waves = false) {
    if constexpr (SYMM) {
        if (as == 8 && heur == 0 && two_waves) return k_step_toa6_w2<REAL, MREAL>;
    }
    return toa6_table<StepToa6<KArgs>, SYMM, REAL, MREAL>(as, heur);
}
template <bool SYMM, typename REAL, typename MREAL>
kfpos_k::cells_kernel_t cells_toa6_kernel(int as, int heur) { return toa6_table<StepToa6<CellArgs>, SYMM, REAL, MREAL>(as, heur); }

