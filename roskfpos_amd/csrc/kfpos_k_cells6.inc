/* kfpos_k_cells6.inc -- k_cells_toa6: the 6-state step of a bank with anchor cells (kfpos_set_anchor_cells), included by
 * kfpos_k_cells6s.hip (symmetric covariance layout: fixed start) and kfpos_k_cells6f.hip (full layout: ML initialisation),
 * which instantiate one half each.
 * The text of k_step_toa6 (kfpos_k_toa6.inc) with one difference: the anchor table is not KArgs::anchors but the table of
 * the workgroup's cell, cell_xyz + cell_of_block[blockIdx.x] * cell_stride, in device memory. One workgroup is one
 * wavefront is one block of KFPOS_CELL_TAGS rows, so the table is wave-uniform as ever: it is read through a pointer in
 * the constant address space (scalar loads, as the kernel-argument table is), and step_toa6<SYMM, HEUR, 0, PEEL>
 * (kfpos_core_toa6.h), the staging helpers and the order of every load and store are k_step_toa6's. A block of cell c
 * therefore computes bit for bit what k_step_toa6 computes for its rows with cell c's table in KArgs::anchors. The host
 * has checked every entry of cell_of_block against n_cells: the kernel indexes with it as it is. */
typedef const __attribute__((address_space(4))) double *cell_table_t;
typedef const __attribute__((address_space(4))) int32_t *cell_map_t;

/* AS as in k_step_toa6: 8 = the epoch in registers, -8 / -16 = compile-time anchor loops over an LDS-resident epoch,
 * 0 = run-time loop. No occupancy is asked for: the cells kernels are the one-wavefront build. */
template <bool SYMM, typename REAL, typename MREAL, int AS, int HEUR = 2>
__global__ __launch_bounds__(WAVE) void k_cells_toa6(const kfpos_k::CellArgs c) {
    extern __shared__ double lds[];
    const KArgs &a = c.k;
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    Params pr = make_params(a);
    const int cell = ((cell_map_t)c.cell_of_block)[blockIdx.x];
    pr.anchors = (const double *)((cell_table_t)c.cell_xyz + (size_t)cell * c.cell_stride);
    constexpr int NA = AS > 0 ? AS : 1;
    /* step_toa6's PEEL, as in k_step_toa6 */
    constexpr bool PEEL = !(AS == -8 && HEUR == 2);
    if (a.n_steps == 1 && a.dt && a.dt[t] < 0.0) { /* no epoch for this tag in this call */
        skipped_lane(a, t, true);
        return;
    }

    /* load order = order of first use, the flags word in front (k_step_toa6) */
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
    const bool waiting = !a.use_init_pos && isnan(tg.pos[0]); /* still waiting for its ML initialisation */
    if (!fin && !waiting) s |= ST_NONFINITE;
    a.flags[t] = fl0 | FL_STARTED;
    if (a.status) a.status[t] = s;
}

/* the table of toa6_each_kernel (kfpos_k_toa6each.inc): toa6_kernel's without the two-wavefront build. Combinations that
 * run the AS = 0 form because their own would touch scratch memory inside the epoch loop (make check): DESIGN.md section 6 */
template <bool SYMM, typename REAL, typename MREAL>
kfpos_k::cells_kernel_t cells_toa6_kernel(int as, int heur) {
    if constexpr (SYMM) {
        if (as == 8) return heur ? k_cells_toa6<true, REAL, MREAL, 8> : k_cells_toa6<true, REAL, MREAL, 8, 0>;
    } else {
        if (as == 8) {
            if (!heur) return k_cells_toa6<false, REAL, MREAL, -8, 0>;
            /* (leave-one-out with the 48-bit covariance on the full layout: never built, as in toa6_kernel) */
            if constexpr (!std::is_same<REAL, p48>::value) return k_cells_toa6<false, REAL, MREAL, -8>;
        }
    }
    if (as == -16) return heur == 1 ? k_cells_toa6<SYMM, REAL, MREAL, -16, 1> : k_cells_toa6<SYMM, REAL, MREAL, -16>;
    return heur ? k_cells_toa6<SYMM, REAL, MREAL, 0> : k_cells_toa6<SYMM, REAL, MREAL, 0, 0>;
}
