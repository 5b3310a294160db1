/* kfpos_k_imu9.inc -- k_step_imu9: the 9-state UWB + IMU step (KalmanFilterTOAIMU.cpp:100-195), included by
 * kfpos_k_imu9.hip (around KArgs: the bench kernel among them) and kfpos_k_cells9.hip (around CellArgs: the ranging rounds
 * of a bank with anchor cells), each with its selector and its own instantiations */
/* a 4-byte value that is (and stays) in an accumulation register at this point */
template <typename W>
__device__ inline void in_agpr(W &w) {
    static_assert(sizeof(W) == 4, "one register");
    asm volatile("" : "+a"(w));
}

/* v holds nothing in particular from here on: ends the life of whatever it held, without an instruction */
__device__ inline void forget(double &v) { asm volatile("" : "=v"(v)); }

/* ------------------------------------------------------------------ 9-state step kernel */
/* RANGING = false: the IMU-only call (MODE_IMU_ONLY), a kernel of its own */
/* ARGS: the argument block, itself the parameter and named wherever a field is read (k_step_toa6 says why). KArgs: the
 * anchor table is KArgs::anchors. CellArgs: the table of the workgroup's cell, and the plain order of an epoch: PAIRS. */
template <typename REAL, typename MREAL, int AS, bool RANGING = true, class ARGS = KArgs>
__global__ __launch_bounds__(WAVE) void k_step_imu9(const ARGS a) {
    /* PAIRS: the 8-anchor ranging kernels around KArgs may end their gain iteration on pairs of lanes and rotate their
     * epoch loop (ROTATE, below). Around CellArgs every form keeps the plain order of an epoch -- step_imu9_state +
     * step_imu9_cov, which computes the same bits (DESIGN.md 6a): no pairs' tail, no rotated loop, no copy of the anchor
     * table in LDS, no padding instruction.
     * TAIL: a pair trip reads registers only (iekf9_pairs_held) -- the 4-byte-measurement kernels with an 8-byte or 6-byte
     * covariance, the two the bench configurations run. With 8-byte measurements (22 more registers across the step) or
     * the 4-byte covariance's rounding code the held values do not fit: those two keep the tail that reads the park and
     * a copy of the anchor table in every trip (iekf9_pairs). */
    constexpr bool PAIRS = AS == 8 && RANGING && !cells_block<ARGS>;
    constexpr bool TAIL = PAIRS && sizeof(MREAL) == 4 && !std::is_same<REAL, float>::value;
    /* Four bytes of padding, executed once per launch. The text that reads KArgs::pair9_first / pair9_dense_until moved
     * every loop of this kernel by 4 bytes modulo 8, and with the same instructions in every trip loop the wavefronts
     * then took 0.55 % (MIXED) / 0.45 % (P48) more cycles per epoch than with this instruction in front, at the same
     * schedule: where a loop lies modulo 8 bytes is worth as much as the schedule (profiles/HISTORY.md, "Where the
     * lanes meet"). Whoever changes the instruction count in front of the loops measures both phases again. */
    if constexpr (TAIL)
        __builtin_amdgcn_s_setprio(0); /* (the priority a wavefront starts with: does nothing) */
    extern __shared__ double lds[];
    const int lane = threadIdx.x;
    const size_t t = (size_t)blockIdx.x * WAVE + lane;
    if (t >= (size_t)a.T) return;
    const size_t T = a.T;
    const uint32_t t32 = (uint32_t)t;
    Params pr = make_params(a);
    if constexpr (cells_block<ARGS>) pr.anchors = cell_anchors(a);
    constexpr bool has_ranging = RANGING;
    /* the next epoch's measurements are fetched one epoch AHEAD, behind the current epoch's arithmetic -- in the
     * KFPOS_STORE_MIXED instantiation (the bench configuration); the other two (8-byte measurements: 22 more registers
     * per lane across the whole step; 4-byte covariance: its rounding code) do not have the registers for that (they
     * spill), so they fetch between two epochs instead */
    constexpr bool AHEAD = sizeof(MREAL) == 4 && !std::is_same<REAL, float>::value;
    const bool fresh_imu = a.mode != MODE_TOA;
    constexpr int NA = AS > 0 ? AS : 1;
    double dt_tag = a.dt_shared; /* the dt of a single-epoch call */
    if (a.n_steps == 1 && a.dt) {
        dt_tag = a.dt[t32];
        if (dt_tag < 0.0) { /* no epoch / sample for this tag in this call */
            skipped_lane(a, t, true);
            return;
        }
    }

    /* load order = order of first use (see k_step_toa6): flags, epoch, position, velocity, IMU sample, then the
     * 45 covariance entries, which are not needed until the ML solve is over. The flags word goes first: the compiler
     * parks it in an AGPR straight away, and vmcnt counts loads in order -- as the last load of the first group it
     * made that move wait for the whole group before the second group (IMU sample, covariance) was even issued */
    uint32_t fl = a.flags[t32];
    RawEpoch<MREAL, NA> raw;
    RawImu<MREAL> rawi;
    if constexpr (AS > 0) {
        if (has_ranging) fetch_epoch<MREAL, AS>(a, t, 0, raw);
    }
    Tag9 tg;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        tg.pos[k] = (a.pos + k * T)[t32];
        tg.vel[k] = (a.vel + k * T)[t32];
    }
    /* the covariance and B^-1 wait in LDS while the gain iteration runs, the accelerometer whitener for the whole
     * launch: [78][lane], behind the generic kernel's epoch scratch */
    const CovPark9 park{lds + ((AS == 0 && has_ranging) ? 3 * (size_t)a.A * WAVE : 0) + lane, WAVE};
    Imu imu;
    imu.has = false;
    imu.ci = park.a + 66 * WAVE;
    imu.ci_stride = WAVE;
    /* The Gauss-Newton solves in ml_estimate's peeled text (step_imu9_state). The two 8-anchor instantiations that do
     * not fetch ahead, short of registers, spill inside the epoch loop with it and keep the unpeeled text. */
    constexpr bool PEEL = AS != 8 || AHEAD;
    if constexpr (TAIL) {
        pr.pair9 = a.pair9 != 0;
        pr.pair9_first = a.pair9_first;
        pr.pair9_dense_until = a.pair9_dense_until;
    } else if constexpr (PAIRS) { /* the anchor table once more, where lanes can index it one by one */
        if (a.pair9) {
            double *tab = lds + 78 * WAVE;
#pragma unroll
            for (int k = 0; k < 24; ++k) tab[k] = a.anchors[k]; /* (every lane writes the same 24 numbers) */
            pr.pair_anchor_tab = tab;
        }
    }
    double cv[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    MREAL rawc[9];
    if (fresh_imu) {
        fetch_imu<MREAL>(a, t, 0, rawi);
        fetch_imu_cov<MREAL>(a, t, 0, rawc);
    } else if (fl & FL_HAS_IMU) { /* re-fuse the latched sample (KalmanFilterTOAIMU.cpp:68-72) */
        imu.has = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) imu.acc[k] = ldrow<MREAL>(a.imu_acc, k, T, t32);
        cv[0] = ldrow<MREAL>(a.imu_cov, 0, T, t32);
        cv[3] = ldrow<MREAL>(a.imu_cov, 1, T, t32);
        cv[4] = ldrow<MREAL>(a.imu_cov, 2, T, t32);
        cv[6] = ldrow<MREAL>(a.imu_cov, 3, T, t32);
        cv[7] = ldrow<MREAL>(a.imu_cov, 4, T, t32);
        cv[8] = ldrow<MREAL>(a.imu_cov, 5, T, t32);
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) tg.P.a[k] = ldcov<REAL>(a.P, k, 45, T, t32);
    if (fresh_imu) { /* the covariance of the first (usually: of every) epoch of this launch */
        imu.has = true;
#pragma unroll
        for (int k = 0; k < 9; ++k) cv[k] = (double)rawc[k];
        if (a.latch) latch_imu_cov<MREAL>(a, T, t32, cv);
    }
    if (imu.has) imu_whitener(cv, imu.ci, imu.ci_stride);
    /* Diagonal accelerometer covariance (what IMU drivers publish): the gain iteration then runs the diagonal form of its
     * pass, which leaves out terms that are exact zeros -- the same bits for every tag. Decided once per launch (the
     * whitener is per launch) and per wavefront: every lane's COMPUTED Sigma^-1 has zeros off its diagonal (a lane
     * without a sample never looks at it). KFPOS_IMU9_DIAG=0 forces the full form (tests, A/B runs). */
    bool diag = false;
    if (a.imu9_diag) {
        const bool mine = !imu.has || (imu.Wi(1) == 0.0 && imu.Wi(2) == 0.0 && imu.Wi(4) == 0.0);
        diag = __builtin_amdgcn_ballot_w64(mine) == __builtin_amdgcn_ballot_w64(true);
    }
    /* ... and every lane has a sample (imu.has does not change during this launch; always so with a fresh sample per
     * epoch): the pass then forms the sample's terms without a per-lane branch. A wavefront with a lane that has
     * nothing latched (MODE_TOA) takes the full per-lane form, diagonal or not: two forms of the trip loop, not four */
    const bool fast = imu9_fast(diag, imu.has);

    /* dt: in a multi-epoch launch it is wave-uniform and sits in the kernel arguments -- read one epoch ahead with a
     * scalar load, so that the epoch loop holds no vector load (and no vmcnt wait) for it; the per-tag dt of a
     * single-epoch call was read at the top */
    const bool multi = a.n_steps > 1; /* wave-uniform */
    double dt_next = multi ? a.dt_steps[0] : dt_tag;
    /* the accelerometer sample of the next epoch travels with its ranges where the two are fetched together (below) */
    constexpr bool IMU_WITH_EPOCH = AHEAD && AS > 0 && RANGING;
    /* the order of an epoch's phases: rotated (below) in the KFPOS_STORE_MIXED instantiation with 8 anchors, the bench
     * kernel; the others keep the order of step_imu9_state. KFPOS_STORE_P48 with 8 anchors was built and measured in the
     * rotated order too: its register allocation came out with as many copies as before, in other places, and 0.5 %
     * slower (profiles/HISTORY.md); 8-byte measurements, 4-byte covariance, the generic anchor loop and the IMU-only
     * kernel do not fetch ahead and were left alone */
    constexpr bool ROTATE = IMU_WITH_EPOCH && PAIRS && std::is_same<REAL, double>::value;

    /* Everything loaded so far has arrived before the loop is entered (the first thing a step does is predict the
     * covariance, so nothing is lost): a wait for these loads INSIDE the loop would be repeated in every epoch, where it
     * waits for the epoch that was only just prefetched. 0x0F70 = vmcnt(0), the other counters untouched. */
    __builtin_amdgcn_s_waitcnt(0x0F70);
    uint32_t s = 0;
    if constexpr (ROTATE) {
        /* The covariance is at home in the park: the head of an epoch's covariance work (prediction, B, the park stores,
         * B^-1) runs behind the update of the epoch before it -- on the P that is in registers there anyway, with the dt
         * that is in a scalar register one epoch ahead -- and the first one here, behind the loads. Across the back-edge a
         * lane carries position, velocity, its words and `invertible`, nothing of P: the ways a step can end (ML
         * initialisation, too few ranges, update skipped, either form of the iteration) all end with P read from the park,
         * so their join copies nothing. The epoch's measurements are unpacked at the top of the body, where the register
         * file is empty, and the next epoch is fetched right there, once, on a path every lane takes. */
        /* (a launch holds at least one epoch -- no host entry point launches a kernel for none --, so the P this head
         * predicts is always consumed by a body) */
        bool invertible = step_imu9_head(tg, pr, dt_next, park);
        double latched[3] = {0.0, 0.0, 0.0};
        if (!fresh_imu && imu.has) {
#pragma unroll
            for (int k = 0; k < 3; ++k) latched[k] = imu.acc[k];
        }
        for (int e = 0; e < a.n_steps; ++e) {
            const double dt = dt_next;
            const bool more = e + 1 < a.n_steps;
            if (multi && more) dt_next = a.dt_steps[opaque_uniform(e + 1)];
            /* the raw words are read where the prefetch put them (accumulation registers: the directly addressable half
             * of the file is taken while they arrive) -- said aloud, so that they cross the back-edge there instead of
             * being copied out in front of it and back in behind it */
#pragma unroll
            for (int k = 0; k < NA; ++k) { in_agpr(raw.mm[k]); in_agpr(raw.e[k]); }
            if (fresh_imu) {
#pragma unroll
                for (int k = 0; k < 3; ++k) in_agpr(rawi.acc[k]);
            }
            /* (written as a choice between the fresh sample and the latched one, which does not change during a launch:
             * the sample is then formed anew in every epoch instead of being carried round the loop) */
#pragma unroll
            for (int k = 0; k < 3; ++k) imu.acc[k] = fresh_imu ? (double)rawi.acc[k] : latched[k];
            RegScratch<NA> sc;
            unpack_epoch<MREAL, NA>(raw, sc);
            /* unpacked before the next epoch is fetched: the new words then land in the registers the old ones leave */
#pragma unroll
            for (int k = 0; k < NA; ++k) { kfpos::kf_pin(sc.r[k]); kfpos::kf_pin(sc.e[k]); }
#pragma unroll
            for (int k = 0; k < 3; ++k) kfpos::kf_pin(imu.acc[k]);
            asm volatile("" ::: "memory");
            /* (unconditional: behind a test of `more` the raw words would be carried round the loop as a choice between
             * the old and the new ones, through a second set of registers; the last epoch fetches itself once more) */
            const int ahead = opaque_uniform(more ? e + 1 : e);
            fetch_epoch<MREAL, NA>(a, opaque_lane(t), ahead, raw);
            if (fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), ahead, rawi);
            Iekf9Out o;
            /* a step that ends early leaves `o` unwritten, and the compiler then carries the last epoch's values round
             * the loop for it: say that they start out as nothing in particular (no instruction) */
#pragma unroll
            for (int k = 0; k < 6; ++k) { forget(o.w[k]); forget(o.mrlast[k]); }
#pragma unroll
            for (int k = 0; k < 3; ++k) forget(o.dlast[k]);
            const bool update = step_imu9_state_parked<RANGING, true, TAIL, PEEL>(tg, sc, pr, dt, imu, park, fast, invertible, o, s);
            if (a.traj) { /* the pose store between the two parts: see the other order below */
#pragma unroll
                for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
            }
            if (update) s = step_imu9_cov(tg, o, imu);
            if (more) {
                static_assert(!cov_is_rounded<REAL>(), "a rounded covariance is rounded here, in front of the head");
                invertible = step_imu9_head(tg, pr, dt_next, park);
                /* P is in the park now, and the next body reads it from there whichever way it goes: nothing of it is
                 * alive in registers (the compiler does not see that `more` means one more trip, and would keep all 45
                 * entries through the inversion for the stores behind the loop) */
#pragma unroll
                for (int k = 0; k < 45; ++k) forget(tg.P.a[k]);
            }
        }
    } else
    for (int e = 0; e < a.n_steps; ++e) { /* the state stays in registers from epoch to epoch */
        const double dt = dt_next;
        if (multi && e + 1 < a.n_steps) dt_next = a.dt_steps[opaque_uniform(e + 1)];
        if (fresh_imu) { /* fresh sample: newIMUMeasurement latches it (KalmanFilterTOAIMU.cpp:78-89) */
#pragma unroll
            for (int k = 0; k < 3; ++k) imu.acc[k] = (double)rawi.acc[k];
            if constexpr (AHEAD && !IMU_WITH_EPOCH) {
                if (e + 1 < a.n_steps) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
            }
        }
        /* The step in two parts with the pose store between them: the pose a per-epoch caller would have read back
         * (getPose at timeLag 0) is final before the covariance update, and vmcnt counts stores too -- the wait at the
         * loop's back-edge (for the prefetched epoch) would otherwise sit right behind this store and wait for its
         * acknowledgement in every epoch. One store for every lane, whichever way it left the first part. */
        Iekf9Out o;
        auto finish = [&](bool update) {
            if (a.traj) {
#pragma unroll
                for (int k = 0; k < 3; ++k) (a.traj + ((size_t)opaque_uniform(e) * 3 + k) * T)[t32] = tg.pos[k];
            }
            if (update) s = step_imu9_cov(tg, o, imu);
        };
        if constexpr (AS > 0) {
            RegScratch<AS> sc;
            if (has_ranging) {
                unpack_epoch<MREAL, AS>(raw, sc);
                if (e + 1 < a.n_steps) {
                    if constexpr (AHEAD) {
                        fetch_epoch<MREAL, AS>(a, opaque_lane(t), opaque_uniform(e + 1), raw);
                        if constexpr (IMU_WITH_EPOCH) {
                            if (fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
                        }
                    }
                }
            } else {
#pragma unroll
                for (int k = 0; k < AS; ++k) sc.r[k] = sc.e[k] = sc.w[k] = 0.0;
            }
            finish(step_imu9_state<RANGING, true, TAIL, true, PEEL>(tg, sc, pr, dt, imu, park, fast, o, s));
            if constexpr (!AHEAD) { /* 8-byte measurements: the next epoch is fetched when this one is over */
                if (e + 1 < a.n_steps) {
                    if (fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
                    if (has_ranging) fetch_epoch<MREAL, AS>(a, opaque_lane(t), opaque_uniform(e + 1), raw);
                }
            }
        } else {
            Scratch sc{nullptr, nullptr, nullptr, WAVE};
            if (has_ranging) sc = stage_epoch_lds<MREAL>(a, lds, lane, t, opaque_uniform(e));
            finish(step_imu9_state<RANGING, true, TAIL, true, PEEL>(tg, sc, pr, dt, imu, park, fast, o, s));
            if constexpr (!AHEAD) { /* the ranges are staged per epoch above; the next accelerometer sample is not */
                if (e + 1 < a.n_steps && fresh_imu) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);
            }
        }
        if constexpr (cov_is_rounded<REAL>()) { /* what n single-epoch launches would have kept in HBM */
            if (e + 1 < a.n_steps) {
#pragma unroll
                for (int k = 0; k < 45; ++k) tg.P.a[k] = round_cov<REAL>(tg.P.a[k]);
            }
        }
    }

    if (fresh_imu && a.latch) { /* the last epoch's sample stays latched (lastImuMeasurement, KalmanFilterTOAIMU.cpp:78-89) */
#pragma unroll
        for (int k = 0; k < 3; ++k) strow<MREAL>(a.imu_acc, k, T, t32, imu.acc[k]);
        fl |= FL_HAS_IMU;
    }
    bool fin = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        (a.pos + k * T)[t32] = tg.pos[k];
        (a.vel + k * T)[t32] = tg.vel[k];
        fin &= isfinite(tg.pos[k]) & isfinite(tg.vel[k]);
    }
#pragma unroll
    for (int k = 0; k < 45; ++k) {
        stcov<REAL>(a.P, k, 45, T, t32, tg.P.a[k]);
        fin &= isfinite(tg.P.a[k]);
    }
    if (nonfinite_state(fin, a.use_init_pos, tg.pos[0])) s |= ST_NONFINITE;
    a.flags[t32] = fl | FL_STARTED;
    if (a.status) a.status[t32] = s;
}
