/*
 * kfpos.h -- C ABI of the MI355X batched EKF positioning core (libkfpos_hip.so).
 *
 * Drop-in boundary: the reference's estimator interface
 *   class PositionEstimationAlgorithm   src/kfpos/algorithms/PositionEstimationAlgorithm.h:8-37
 * as implemented by
 *   KalmanFilterTOA      src/kfpos/algorithms/KalmanFilterTOA.{h,cpp}     (ALGORITHM_KF_TOA)
 *   KalmanFilterTOAIMU   src/kfpos/algorithms/KalmanFilterTOAIMU.{h,cpp}  (ALGORITHM_KF_TOA_IMU)
 * and called from PosGenerator (src/kfpos/publishers/Posgenerator.cpp:491 newTOAMeasurement,
 * :139 newIMUMeasurement, :537 init, :543 getPose). The reference runs ONE filter for ONE tag per
 * process; this library runs T independent filters per handle, one per GPU lane, with the same
 * per-filter semantics. The wall clock the reference reads inside the estimator
 * (KalmanFilterTOA.cpp:76-88) is passed in as dt. Plain C types only: no exceptions cross this
 * boundary, per-tag conditions are reported in a status word instead.
 *
 * Host-side mirrors of the reference classes on top of this ABI: roskfpos_amd/csrc/kfpos_adaptor.h.
 * The binding a reference maintainer would add: INTEGRATION.md.
 */
#ifndef KFPOS_H
#define KFPOS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KFPOS_VERSION 102 /* 0.1.2: KFPOS_STORE_P48 keeps 40 significant bits (0.1.1: kfpos_config.ml_variant, kfpos_comm_*) */

/* ---- return codes (every entry point returns one; 0 = success) ---- */
#define KFPOS_OK            0
#define KFPOS_ERR_ARG       1 /* NULL / out-of-range argument */
#define KFPOS_ERR_HIP       2 /* a HIP call failed; kfpos_last_error() has the text */
#define KFPOS_ERR_NO_DEVICE 3 /* no usable gfx950 device */
#define KFPOS_ERR_MODEL     4 /* call not defined for this handle's model */
#define KFPOS_ERR_STATE     5 /* e.g. anchors not set yet (Posgenerator.cpp:92-96 drops ranges until then) */
#define KFPOS_ERR_COMM      6 /* an RCCL call failed, or librccl could not be opened; kfpos_last_error() has the text */

/* ---- models: the `algorithm` launch parameter (node_pos.cpp:48-58) ---- */
#define KFPOS_MODEL_TOA     0 /* ALGORITHM_KF_TOA     -> KalmanFilterTOA, 6 states p,v */
#define KFPOS_MODEL_TOA_IMU 1 /* ALGORITHM_KF_TOA_IMU -> KalmanFilterTOAIMU, 9 states p,v,a (3-token repair) */
#define KFPOS_MODEL_ML      2 /* ALGORITHM_ML -> MLLocation as the estimator (MLLocation.cpp:421-486): 3-D, variant NORMAL
                               (top_n = 0), IGNORE_N (top_n = numRangingsToIgnore) or BEST (kfpos_config.ml_variant);
                               state = position, P = its 3x3 covariance; dt is ignored, use_init_pos selects the
                               solver's seed ({1,1,4} otherwise) */
#define KFPOS_MODEL_PLANAR  3 /* ALGORITHM_KF -> KalmanFilter (KalmanFilter.cpp): 8 states [x y vx vy ax ay theta omega] at a
                               fixed height, fed by ranging epochs and, optionally, PX4Flow / IMU / magnetometer /
                               compass samples (kfpos_step_sensor). Configure with kfpos_set_planar() before stepping */

/* ---- storage precision of the covariance and of the measurements in HBM; arithmetic is always f64 ----
 * Positions and velocities are kept as double in every mode, ranges are exact integer mm. F32 rounds the covariance to
 * 24 bits between epochs: the 6-state filter stays at 3e-9 m from the CPU reference, the 9-state filter amplifies that
 * rounding to 1.6e-6 m RMS over 100 epochs of the BASELINE trace -- above the 1e-6 m bar: use P48 or MIXED there.
 * F64 and MIXED keep the covariance exactly. */
#define KFPOS_STORE_F64   0 /* covariance double, measurements (kfpos_real) double */
#define KFPOS_STORE_F32   1 /* covariance float,  measurements (kfpos_real) float */
#define KFPOS_STORE_MIXED 2 /* covariance double, measurements (kfpos_real) float: exact filter state, compact inputs */
#define KFPOS_STORE_P48   3 /* covariance in 6 bytes per entry -- sign, 8 exponent bits (single's range), 39 mantissa bits,
                               rounded to nearest (roskfpos_amd/csrc/kfpos_p48.h) --, measurements float: the compact mode
                               that keeps the 9-state filter inside the 1e-6 m bar (1e-9 m on the 100-epoch BASELINE trace;
                               6.6e-8 m RMS over 2 048 tags x 2 000 epochs, no single epoch above 6e-7 m; F32's 24 bits give
                               1.6e-6 m after 100 epochs). Over 10 000 epochs one epoch of capped steps takes it to 2.7e-6 m
                               (MIXED: 1e-8 m): the mode for the 25 % smaller state, not for the last digits. An infinite
                               entry is stored as NaN. DESIGN.md section 3 */

#define KFPOS_MAX_ANCHORS 64 /* MAX_NUM_ANCS, Posgenerator.h:74 */

/* ---- per-tag status word ---- */
#define KFPOS_ST_UPDATE_SKIPPED 0x01u /* the std::runtime_error the reference swallows (KalmanFilterTOA.cpp:151-153); the
                                         9-state and planar filters have no try/catch (the node would abort): here the
                                         tag keeps its predicted covariance and reports this bit. Also: ML initialisation
                                         whose covariance is exactly singular, planar sensor row with zero variance */
#define KFPOS_ST_ML_FALLBACK    0x02u /* ML position NaN -> predicted position (KalmanFilterTOA.cpp:270-272) */
#define KFPOS_ST_FEW_RANGES     0x04u /* < 4 ranges this epoch (< 3 for the planar filter's 2-D solve): ML returned its seed
                                         (MLLocation.cpp:158-161, :54-58) */
#define KFPOS_ST_ML_INIT        0x08u /* this epoch was consumed by the ML initialisation (KalmanFilterTOA.cpp:90-108) */
#define KFPOS_ST_NOT_STARTED    0x10u /* getPose() == false: no measurement yet (KalmanFilterTOA.cpp:442-447) */
#define KFPOS_ST_NONFINITE      0x20u /* state not finite after the call */
#define KFPOS_ST_SKIPPED        0x40u /* dt < 0 was passed for this tag: no estimator call, filter untouched */
#define KFPOS_ST_GAIN_ITERS(s)  (((s) >> 8) & 0xffu)  /* IEKF gain iterations (KalmanFilterTOA.cpp:293-324); KFPOS_MODEL_ML with
                                                         top_n > 0: Gauss-Newton iterations of the solve that ranks the
                                                         residuals (estimatePositionIgnoreN's first, MLLocation.cpp:318) */
#define KFPOS_ST_ML_ITERS(s)    (((s) >> 16) & 0xffu) /* ML Gauss-Newton iterations, saturating (MLLocation.cpp:168-225) */
#define KFPOS_ST_IGNORED(s)     ((int)(((s) >> 24) & 0xffu) - 1) /* index among this epoch's >0 ranges of the anchor the
                                                                    leave-one-out heuristic dropped, -1 if none */

/* Construction parameters: the constructor arguments of KalmanFilterTOA (KalmanFilterTOA.h:21-22) and
 * KalmanFilterTOAIMU (KalmanFilterTOAIMU.h:19-20) plus the batch shape. Launch-file names in brackets. */
typedef struct kfpos_config {
    int32_t model;          /* KFPOS_MODEL_*                                   [algorithm] */
    int32_t n_tags;         /* T, filters in this handle (>= 1) */
    int32_t max_anchors;    /* A, columns of the range matrix, 1..KFPOS_MAX_ANCHORS */
    int32_t storage;        /* KFPOS_STORE_* */
    double  accel_noise;    /* accelerationNoise                               [accelNoise], kfpos_toa.launch:13 */
    double  jolt;           /* jolt (9-state process noise)                    [jolt], kfpos_toa_imu.launch */
    int32_t ignore_worst;   /* ignoreWorstAnchorMode (6-state only)            [useHeuristicIgnoreWorst] */
    double  cost_threshold; /* ignoreCostThreshold                             [heuristicIgnoreThreshold] */
    int32_t top_n;          /* ranges dropped by residual ranking, 0 = off     [numRangingsToIgnore], BASELINE config 5 */
    int32_t use_init_pos;   /* 1: fixed initial position, P0 = 0; 0: ML initialisation on the first epoch
                               (the reference's mUseFixedInitialPosition)      [useStartPosition] */
    double  init_pos[3];    /* initialPosition for every tag                   [initPositionX/Y/Z]; per-tag values:
                               kfpos_set_init_positions() */
    int32_t device;         /* HIP device ordinal */
    int32_t ml_variant;     /* KFPOS_MODEL_ML only (0 otherwise): KFPOS_ML_NORMAL / _IGNORE_N / _BEST  [variant],
                               MLLocation.h:5-7, Posgenerator.cpp:79-83 */
} kfpos_config;
#define KFPOS_ML_NORMAL   0 /* estimatePosition (MLLocation.cpp:153-257); with top_n > 0 it acts as IGNORE_N */
#define KFPOS_ML_IGNORE_N 1 /* estimatePositionIgnoreN (:307-347) with numRangingsToIgnore = top_n */
#define KFPOS_ML_BEST     2 /* estimatePositionBestGroup (:348-414): every subset of 4 ranges, smallest covariance trace
                               wins. Defined by the reference for 4 or 5 ranges only -- its erase loop (:377-381) runs past
                               the end of the vector from 6 ranges on -- so kfpos_set_anchors refuses more than 5 anchors
                               for this variant (KFPOS_ERR_MODEL); top_n is ignored, as numRangingsToIgnore is there.
                               Status word: KFPOS_ST_IGNORED = the range the winning group did without, KFPOS_ST_GAIN_ITERS
                               = the most Gauss-Newton passes any group took */

/* KFPOS_MODEL_PLANAR only: the attributes KalmanFilter::loadConfigurationFiles reads from the four XML
 * parameters (KalmanFilter.cpp:748-842; config_uwb.xml / config_px4flow.xml / config_imu.xml / config_mag.xml
 * of src/kfpos/config) plus the constructor's initialAngle (KalmanFilter.h:32). */
typedef struct kfpos_planar_config {
    int32_t use_fixed_height;  /* <uwb useFixedHeight/>: 1 = 2-D ML initialisation at fixed_height, 0 = 3-D ML
                                  initialisation whose z becomes the height (KalmanFilter.cpp:252-258) */
    double  fixed_height;      /* <uwb fixedHeight/> = mUWBtagZ */
    double  init_angle;        /* initialAngle [initAngle] */
    double  px4_height;        /* <px4flow sensorHeight/> */
    double  px4_arm_p1;        /* <px4flow armP0/> */
    double  px4_arm_p2;        /* <px4flow armP1/> */
    double  px4_cov_velocity;  /* <px4flow covarianceVelocity/> */
    double  px4_cov_gyro_z;    /* <px4flow covarianceGyroZ/> */
    int32_t imu_use_fixed_cov_acc;       /* <imu useFixedCovarianceAcceleration/> */
    double  imu_cov_acc;                 /* <imu covarianceAcceleration/> */
    int32_t imu_use_fixed_cov_ang_vel_z; /* <imu useFixedCovarianceAngularVelocityZ/> */
    double  imu_cov_ang_vel_z;           /* <imu covarianceAngularVelocityZ/> */
    double  mag_angle_offset;  /* <mag angleOffset/> */
    double  mag_cov;           /* <mag covarianceMag/> */
} kfpos_planar_config;

/* sensor kinds of kfpos_step_sensor: the other four entry points of PositionEstimationAlgorithm */
#define KFPOS_SENSOR_PX4FLOW 1 /* newPX4FlowMeasurement (KalmanFilter.cpp:102-135): 5 values per tag = integrationX,
                                  integrationY, integrationRotationZ, integrationTime [us], quality. A sample with
                                  quality 0 is dropped on entry (status KFPOS_ST_SKIPPED) */
#define KFPOS_SENSOR_IMU     2 /* newIMUMeasurement (:139-182): 24 values = angularVelocity[3], its covariance[9],
                                  linearAcceleration[3], its covariance[9] (row-major 3x3) */
#define KFPOS_SENSOR_MAG     3 /* newMAGMeasurement (:185-199): 3 values = mag x, y, z (its covariance argument is
                                  ignored by the reference and is not part of this ABI) */
#define KFPOS_SENSOR_COMPASS 4 /* newCompassMeasurement (:201-229): 1 value = heading in radians */

typedef struct kfpos_handle kfpos_handle;

/* ---- lifetime: PosGenerator::setAlgorithm (Posgenerator.cpp:510-538) ----
 * kfpos_create answers, in this order: KFPOS_ERR_ARG for a null argument, for a configuration it refuses and for a bad
 * KFPOS_PAIR9_MEET (kfpos_last_error says which), KFPOS_ERR_NO_DEVICE, KFPOS_ERR_HIP where an allocation failed. Every
 * KFPOS_* environment variable that bears on a handle is read here, once -- KFPOS_SLOT_SPLIT_BYTES included, which
 * setting between kfpos_create and the first slot call therefore does not change (README.md lists them). */
int kfpos_create(const kfpos_config *cfg, kfpos_handle **out);
int kfpos_destroy(kfpos_handle *h);
/* PositionEstimationAlgorithm::init(). Returns KFPOS_OK (the reference's `true`). */
int kfpos_init(kfpos_handle *h);
/* Beacon table: what PosGenerator keeps in `beacons` from the anchors topic (Posgenerator.cpp:15-39)
 * and zips into newTOAMeasurement's `beacons` argument (:486-487). xyz: n_anchors*3 doubles, metres.
 * ids may be NULL (kept for the caller's id->column map only). */
int kfpos_set_anchors(kfpos_handle *h, const double *xyz, const int32_t *ids, int32_t n_anchors);
/* Per-tag fixed start positions, n_tags*3 doubles (batched form of the initialPosition ctor argument).
 * Only before the first step and only with use_init_pos = 1. */
int kfpos_set_init_positions(kfpos_handle *h, const double *xyz);

/* ---- anchor cells: one bank, one launch, an anchor table per block of KFPOS_CELL_TAGS rows ----
 * A bank of many rooms: rows [64 b, 64 b + 64) form block b (the last block may be partial), and every block ranges
 * against the table of the cell cell_of_block[b]. xyz: [n_cells][n_anchors][3] doubles, metres; cell_of_block:
 * [(n_tags + 63) / 64] entries, each in [0, n_cells). n_anchors is ONE count for the handle, 1 .. max_anchors; a cell with
 * fewer anchors pads its table with zeros, as kfpos_set_anchors pads, and sends no range (<= 0) in those columns. A tag
 * that roams to another room moves to a row of a block of that room: kfpos_get_tags -> kfpos_set_tags ->
 * kfpos_reset_tags. KFPOS_VERSION is unchanged: detect the feature by symbol.
 *
 * What it computes. Take a handle R with the same kfpos_config, created under KFPOS_NO_COOP=1, on which
 * kfpos_set_anchors(table of cell c, NULL, n_anchors) was called. After the same calls with the same inputs every status
 * word, every trajectory row and every stored byte (state, covariance in the handle's storage encoding, flags, latch)
 * of every row of every block assigned to cell c is bit-identical in this handle and in R.
 *
 * Honoured by every whole-bank ranging round: kfpos_step_toa, kfpos_step_toa_imu, their _dev forms, whole-bank slot
 * rounds (KFPOS_SLOT_RANGES_D16 included), the mapped-block path of small banks, and kfpos_run_trace_dev, which stays
 * FUSED: up to KFPOS_TRACE_CHUNK_STEPS epochs per launch, as without cells. Unaffected (they read no anchor): IMU-only
 * rounds, the pose calls, the lifecycle calls, the state accessors, the pose gather.
 * Refused on a handle with cells, with KFPOS_ERR_MODEL and a kfpos_last_error() that says why:
 *   kfpos_step_*_rows and kfpos_slot_submit_rows -- the compact work bank of a row list mixes rows of different cells in
 *     one wavefront, and the anchors are wave-uniform;
 *   kfpos_run_events_dev, kfpos_run_events_each_dev and kfpos_run_trace_each_dev -- their kernels read the one table of
 *     the kernel arguments; no cells form of them is built yet.
 *
 * Errors, all found on the host before anything is written (after an error nothing has changed, and the kernels never see
 * an unchecked cell index): KFPOS_ERR_ARG for a NULL pointer, n_cells < 1, n_anchors outside 1 .. max_anchors, or a cell
 * index outside [0, n_cells) -- kfpos_last_error() names the first offending block. KFPOS_ERR_MODEL on KFPOS_MODEL_ML and
 * KFPOS_MODEL_PLANAR: no cells kernel is built for them. KFPOS_ERR_STATE on a handle that runs the 8-lanes-per-tag kernel
 * (small plain 6-state banks) and has already stepped: that kernel sums in another order. Such a handle that has NOT
 * stepped leaves that kernel for good with its first kfpos_set_anchor_cells and from then on behaves like one created
 * under KFPOS_NO_COOP=1 -- also after a later kfpos_set_anchors.
 *
 * The call may be repeated at any time -- to remap blocks, move anchors, change n_cells -- and takes effect for the calls
 * made after it. It is a configuration call, the table lives in device memory: it first waits for everything the slots
 * have in flight and for the handle's device (hipDeviceSynchronize). kfpos_set_anchors afterwards returns the handle to
 * one table. A bank of more than 65 536 tags runs the one-wavefront build of its kernel while it has cells: the same
 * bits, slower. */
#define KFPOS_CELL_TAGS 64   /* rows per block: rows [64 b, 64 b + 64) form block b; the last block may be partial */
int kfpos_set_anchor_cells(kfpos_handle *h, int32_t n_cells, int32_t n_anchors,
                           const double *xyz,             /* [n_cells][n_anchors][3], metres */
                           const int32_t *cell_of_block); /* [(n_tags + 63) / 64], each in [0, n_cells) */
int kfpos_anchor_cells(const kfpos_handle *h);            /* cells in force, 0 = one table (kfpos_set_anchors) */

/* KFPOS_MODEL_PLANAR: what KalmanFilter::init() loads. Before the first step; every tag starts at
 * fixed_height / init_angle. KFPOS_ERR_MODEL on other models. */
int kfpos_set_planar(kfpos_handle *h, const kfpos_planar_config *cfg);

/* size in bytes of kfpos_real for this handle (8 or 4) */
int kfpos_real_size(const kfpos_handle *h);

/* ---- synchronous host-buffer API (pointers are borrowed until the call returns) ---- */

/* One ranging epoch for every tag = T calls of newTOAMeasurement (KalmanFilterTOA.cpp:43-61,
 * KalmanFilterTOAIMU.cpp:49-73) -> estimatePositionKF (predict + iterated update).
 *   range_mm  n_tags x max_anchors, row-major, integer millimetres exactly as PosGenerator stores them
 *             (Posgenerator.cpp:213); <= 0 = no range from that anchor this epoch (:483)
 *   err_est   n_tags x max_anchors, kfpos_real, m^2, must be > 0 where a range is present (:485)
 *   dt        seconds since the previous estimate of each tag (the reference's wall-clock timeLag;
 *             0.1 on a filter's first call, KalmanFilterTOA.cpp:81); dt_len = 1 (shared) or n_tags.
 *             With dt_len = n_tags a NEGATIVE dt[t] means "tag t has no epoch in this call": its filter is
 *             left untouched (tags report asynchronously; kfpos_ingest.h batches whoever flushed)
 *   status    n_tags words or NULL
 * A 9-state handle fuses the latched IMU sample again, as the reference does (KalmanFilterTOAIMU.cpp:68-72). */
int kfpos_step_toa(kfpos_handle *h, const int32_t *range_mm, const void *err_est,
                   const double *dt, int32_t dt_len, uint32_t *status);

/* One IMU sample for every tag = T calls of newIMUMeasurement (KalmanFilterTOAIMU.cpp:76-92): latch
 * linearAcceleration + covarianceAcceleration, then predict + IMU-only update. angularVelocity and its
 * covariance are ignored by the reference and are not part of this ABI. 6-state handles: no-op
 * (KalmanFilterTOA.cpp:64), returns KFPOS_OK.
 *   accel n_tags x 3, cov n_tags x 9 (row-major 3x3, symmetric positive definite), kfpos_real */
int kfpos_step_imu(kfpos_handle *h, const void *accel, const void *cov,
                   const double *dt, int32_t dt_len, uint32_t *status);

/* Fused epoch: latch the IMU sample, then the ranging epoch -- exactly the reference sequence
 * { newIMUMeasurement at timeLag 0 ; newTOAMeasurement at timeLag dt } (the IMU-only estimate is the
 * identity at timeLag 0). 9-state handles only. */
int kfpos_step_toa_imu(kfpos_handle *h, const int32_t *range_mm, const void *err_est,
                       const void *accel, const void *cov,
                       const double *dt, int32_t dt_len, uint32_t *status);

/* KFPOS_MODEL_PLANAR: one sample of one of the other four sensors for every tag = T calls of
 * newPX4FlowMeasurement / newIMUMeasurement / newMAGMeasurement / newCompassMeasurement: latch the sample, then
 * predict + update with that sensor's rows (the compass call also carries the latched PX4Flow and IMU samples,
 * KalmanFilter.cpp:213-226). From then on every ranging epoch of that tag carries its latched samples
 * (:84-98). data: n_tags x C doubles row-major, C by kind (KFPOS_SENSOR_*); dt / dt_len / status as in
 * kfpos_step_toa. Other models: the reference's empty virtuals, returns KFPOS_OK and status 0. */
int kfpos_step_sensor(kfpos_handle *h, int32_t kind, const double *data,
                      const double *dt, int32_t dt_len, uint32_t *status);
/* mUWBtagZ of every tag (n_tags doubles): the configured height, or the ML initialisation's z. kfpos_set_height puts
 * it back when a checkpoint is restored (with useFixedHeight = 0 the 3-D ML initialisation replaced the configured
 * value, KalmanFilter.cpp:252-258). KFPOS_MODEL_PLANAR only. */
int kfpos_get_height(kfpos_handle *h, double *z);
int kfpos_set_height(kfpos_handle *h, const double *z);

/* getPose for every tag (KalmanFilterTOA.cpp:438-473, KalmanFilterTOAIMU.cpp:476-510): predict-only
 * extrapolation by dt_ahead, filter state untouched. pos n_tags x 3, cov3x3 n_tags x 9 (position block of
 * the predicted covariance; the only block stateToPose fills, KalmanFilterTOA.cpp:159-183), vel n_tags x 3
 * (linearSpeed*, 9-state; zeros for 6-state), all double; any may be NULL. A tag without a measurement
 * yet reports KFPOS_ST_NOT_STARTED and NaN (getPose() == false). */
int kfpos_get_pose(kfpos_handle *h, double dt_ahead, double *pos, double *cov3x3, double *vel,
                   uint32_t *status);
/* Same with one extrapolation time per tag (dt_ahead: n_tags doubles): tags report asynchronously, so
 * "now minus the time of my last estimate" differs from tag to tag (KalmanFilterTOA.cpp:451-452). */
int kfpos_get_pose_each(kfpos_handle *h, const double *dt_ahead, double *pos, double *cov3x3, double *vel,
                        uint32_t *status);

/* The whole predict-only extrapolation getPose computes before stateToPose thins it out
 * (KalmanFilterTOA.cpp:455-468, KalmanFilterTOAIMU.cpp:492-506): x n_tags x n, P n_tags x n x n row-major,
 * double; dt_len = 1 (shared) or n_tags. Tags without a measurement yet report KFPOS_ST_NOT_STARTED.
 * Used by the adaptor to fill Vector3::covarianceMatrix exactly as stateToPose does. */
int kfpos_get_predicted(kfpos_handle *h, const double *dt_ahead, int32_t dt_len, double *x, double *P,
                        uint32_t *status);

/* Raw filter members for tests and checkpoint/restore: x n_tags x n ([p, v(, a = 0)]; planar:
 * [x y vx vy 0 0 theta omega]), P n_tags x n x n row-major, double. n = kfpos_state_dim(). flags: n_tags
 * words (bit 0 started, bit 1 has latched IMU; planar: bits 5..7 latched PX4Flow / IMU / magnetometer), may
 * be NULL. */
int kfpos_state_dim(const kfpos_handle *h);
int kfpos_get_state(kfpos_handle *h, double *x, double *P, uint32_t *flags);
int kfpos_set_state(kfpos_handle *h, const double *x, const double *P, const uint32_t *flags);
/* The latched sensor samples (lastImuMeasurement etc.), the rest of a checkpoint: n_tags x kfpos_latch_dim() doubles.
 * 9-state: 12 = linearAcceleration[3] + its covariance 3x3 row-major (KalmanFilterTOAIMU.h:58-59); planar: 15 =
 * PX4Flow {vx, vy, gyroz, covarianceVelocity, covarianceGyroZ}, IMU {ax, ay, angularVelocityZ,
 * covarianceAccelerationXY[4], covarianceAngularVelocityZ}, magnetometer {angle, covarianceMag}
 * (sensor_types.h:32-60); ALGORITHM_ML: 3 = _previousEstimation, the seed of every solve (MLLocation.cpp:3-22);
 * 6-state filter: 0, both calls are no-ops. Which samples are live is in the flags word. A complete checkpoint of a
 * handle = kfpos_get_state + flags, kfpos_get_latch and, for the planar filter, kfpos_get_height. */
int kfpos_latch_dim(const kfpos_handle *h);
int kfpos_get_latch(kfpos_handle *h, double *latch);
int kfpos_set_latch(kfpos_handle *h, const double *latch);

/* ---- per-tag lifecycle: reset, read and write CHOSEN tags, on the device ----
 * The accessors above move the whole bank. These three work on a list: `rows` is a host array of n row indices into
 * the bank, and what crosses the bus is that list plus the listed tags' values -- the cost follows n, not n_tags. They
 * make a row of the bank reusable: a tag that left is reset and the row serves another (kfpos_ingest.h:
 * releaseRows / bindRows), a tag moves to another handle by kfpos_get_tags there + kfpos_set_tags here.
 * KFPOS_VERSION is unchanged by them: detect them by symbol (dlsym / hasattr), not by version number.
 *
 * Common rules:
 *   validation  happens before any write: h == NULL, rows == NULL with n > 0, n < 0, a row outside [0, n_tags) ->
 *               KFPOS_ERR_ARG; a row listed twice in kfpos_reset_tags / kfpos_set_tags -> KFPOS_ERR_ARG (kfpos_get_tags
 *               may repeat rows); height != NULL on a handle that is not KFPOS_MODEL_PLANAR -> KFPOS_ERR_MODEL.
 *               kfpos_last_error() names the first offending entry of the list, whichever of these rules it breaks.
 *               After an error nothing has been written. This host-side check IS the bounds check: the kernels never
 *               see an index that was not checked.
 *   n == 0      KFPOS_OK, nothing happens.
 *   ordering    like the other synchronous calls: first everything the streaming slots have in flight completes, and
 *               the call returns when its own work is complete. Runs on the handle's device, leaves the caller's
 *               current device as it was.
 *   tags not listed are not written at all.
 *
 * kfpos_reset_tags: the listed tags go back to the state kfpos_create (+ kfpos_set_planar) leaves a tag in: flags 0
 * (getPose() == false, KFPOS_ST_NOT_STARTED), covariance all-zero in the handle's storage encoding, velocity 0, latched
 * samples cleared. From then on the tag cannot be told from the same row of a handle just created with the same
 * configuration: every later status word, state and covariance is bit-identical.
 *   use_init_pos = 1: position (and, KFPOS_MODEL_ML, the solver's seed) = init_xyz[i] (n x 3 doubles, row-major), or
 *                     kfpos_config.init_pos when init_xyz is NULL.
 *   use_init_pos = 0: position NaN, i.e. the tag's next ranging epoch is its ML initialisation; init_xyz must be NULL
 *                     (KFPOS_ERR_STATE otherwise, as kfpos_set_init_positions answers).
 *   KFPOS_MODEL_PLANAR: height = kfpos_planar_config.fixed_height whatever init_xyz's z says (kfpos_set_init_positions
 *                     does the same), angle = init_angle, angular speed 0, as kfpos_set_planar wrote them.
 * Unlike kfpos_set_tags a reset does not count as a step: a handle that has never stepped is still "fresh" after it,
 * as its rows are, so kfpos_set_init_positions / kfpos_set_planar remain legal there -- and rewrite every tag, the
 * reset ones included.
 * Which kernel a planar handle runs for its ranging epochs (with or without latched samples) is a property of the
 * handle, not of a tag: a reset does not change it. */
int kfpos_reset_tags(kfpos_handle *h, const int32_t *rows, int32_t n, const double *init_xyz);

/* kfpos_get_state + kfpos_get_latch + kfpos_get_height for the listed tags only: entry i of every output is, bit for
 * bit, row rows[i] of what those calls return (the 9-state x carries a = 0, the planar x is [x y vx vy 0 0 theta omega],
 * P is expanded from the packed or full layout, F32 / P48 entries are decoded). x n x dim, P n x dim x dim, flags n,
 * latch n x kfpos_latch_dim(), height n (planar). Any output may be NULL. */
int kfpos_get_tags(kfpos_handle *h, const int32_t *rows, int32_t n,
                   double *x, double *P, uint32_t *flags, double *latch, double *height);
/* The inverse: stores what kfpos_set_state / kfpos_set_latch / kfpos_set_height would store for those rows (symmetric
 * layouts read the upper triangle j >= i of P, P48 entries are rounded and encoded as the kernels do, the 9-state latch
 * is kept as acceleration + lower triangle of its covariance in kfpos_real). Any input may be NULL = leave that part
 * of the listed tags as it is. Like kfpos_set_state it counts as a step (kfpos_set_init_positions / kfpos_set_planar
 * are refused afterwards), and restored planar latch bits switch the handle's ranging epochs to the instantiation
 * that honours them. */
int kfpos_set_tags(kfpos_handle *h, const int32_t *rows, int32_t n,
                   const double *x, const double *P, const uint32_t *flags, const double *latch, const double *height);

/* ---- row-list steps: an epoch for the tags that REPORTED ----
 * Tags report asynchronously: a round usually carries a fraction of the bank. The calls above are whole-bank (a tag
 * without an epoch is marked by dt < 0, and all n_tags x max_anchors inputs cross the bus); these take a list, like
 * the lifecycle calls: `rows` = n row indices, inputs row-major PER LISTED TAG -- entry i belongs to tag rows[i] --, and
 * what crosses the bus and what the GPU touches follows n.
 *   semantics   exactly the whole-bank call of the same name with the listed tags' inputs and dt < 0 for every other
 *               tag: every status word, state, covariance and latch comes out bit-identical (the same kernel runs, on
 *               a compact copy of the listed tags that is gathered before and scattered after it). A tag that is not
 *               listed is not written. A negative dt[i] still skips tag rows[i] (KFPOS_ST_SKIPPED).
 *   dt          dt_len = 1 (shared by the listed tags) or n;  status: n words or NULL
 *   validation  on the host before any write: h == NULL, n < 0, rows == NULL with n > 0, a row outside [0, n_tags) or
 *               listed twice -> KFPOS_ERR_ARG, kfpos_last_error() names the first offending entry. The kernels never see
 *               an unchecked index, which is why there is no _dev variant: a device-resident list could not be checked
 *               without a synchronisation.
 *   n == 0      KFPOS_OK, nothing happens.
 *   ordering, device, model errors and no-ops (6-state IMU, non-planar sensor: KFPOS_OK, status 0) as the whole-bank
 *               calls; the call counts as a step, and a sensor call switches a planar handle's ranging epochs to the
 *               instantiation that honours latches, as kfpos_step_sensor does.
 * KFPOS_VERSION is unchanged by them: detect them by symbol. */
int kfpos_step_toa_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const int32_t *range_mm /* n x max_anchors */,
                        const void *err_est /* n x max_anchors */, const double *dt, int32_t dt_len, uint32_t *status);
int kfpos_step_imu_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const void *accel /* n x 3 */,
                        const void *cov /* n x 9 */, const double *dt, int32_t dt_len, uint32_t *status);
int kfpos_step_toa_imu_rows(kfpos_handle *h, const int32_t *rows, int32_t n, const int32_t *range_mm, const void *err_est,
                            const void *accel, const void *cov, const double *dt, int32_t dt_len, uint32_t *status);
int kfpos_step_sensor_rows(kfpos_handle *h, const int32_t *rows, int32_t n, int32_t kind, const double *data /* n x C */,
                           const double *dt, int32_t dt_len, uint32_t *status);

/* ---- pose for a row list: getPose for the tags that REPORTED ----
 * What a node publishes is getPose -- position, its 3x3 covariance and the velocity, extrapolated by "now minus my last
 * estimate" (Posgenerator.cpp:541-548). kfpos_get_pose / kfpos_get_pose_each / kfpos_get_predicted compute it for the
 * whole bank; these take a list, like the lifecycle calls and the row-list steps: `rows` = n row indices, and what
 * crosses the bus -- the list, dt_ahead, the listed entries' results -- and what the GPU touches follows n, not n_tags.
 *   semantics   entry i of every output is, bit for bit, row rows[i] of what kfpos_get_pose_each / kfpos_get_predicted
 *               return when that row's dt_ahead is dt_ahead[dt_len == 1 ? 0 : i] (the same per-tag code runs). Outputs
 *               are row-major per listed ENTRY: pos n x 3, cov3x3 n x 9, vel n x 3, x n x dim, P n x dim x dim, status
 *               n. dt_ahead belongs to the entry, not to the row: a row listed twice with two values comes back twice,
 *               extrapolated by each. A tag that has not started reports KFPOS_ST_NOT_STARTED and NaN. Any output of
 *               kfpos_get_pose_rows may be NULL; x and P of kfpos_get_predicted_rows may not. The filter state is not
 *               touched.
 *   validation  on the host before anything is enqueued: h == NULL, n < 0, rows == NULL with n > 0, a row outside
 *               [0, n_tags), dt_ahead == NULL, dt_len other than 1 or n, x or P == NULL -> KFPOS_ERR_ARG;
 *               kfpos_last_error() names the first offending entry. Rows may repeat, as in kfpos_get_tags. Nothing has
 *               been written after an error. This check IS the bounds check: the kernel never sees an unchecked index.
 *   n == 0      KFPOS_OK, nothing happens.
 *   ordering    like kfpos_get_tags: first everything the streaming slots have in flight completes, and the call returns
 *               when its own work is complete. Runs on the handle's device, leaves the caller's current device as it was.
 * KFPOS_VERSION is unchanged by them: detect them by symbol. */
int kfpos_get_pose_rows(kfpos_handle *h, const int32_t *rows, int32_t n,
                        const double *dt_ahead, int32_t dt_len /* 1 or n */,
                        double *pos /* n x 3 */, double *cov3x3 /* n x 9 */, double *vel /* n x 3 */,
                        uint32_t *status /* n */);
int kfpos_get_predicted_rows(kfpos_handle *h, const int32_t *rows, int32_t n,
                             const double *dt_ahead, int32_t dt_len,
                             double *x /* n x dim */, double *P /* n x dim x dim */, uint32_t *status);

/* ---- streaming host API: epochs pipelined through kfpos_slot_count() slots of pinned host memory ----
 * For a node that feeds epoch after epoch from the CPU (PosGenerator's table flushes, Posgenerator.cpp:155-198, batched
 * over many tags): the synchronous calls above copy pageable arrays, turn their layout on the device and wait; here
 * the caller ASSEMBLES each epoch directly in a slot -- host-pinned memory owned by the handle, component-major like the
 * device layout ([max_anchors][n_tags] etc., see below) -- and submits it. A submission only enqueues: inputs go to the
 * GPU by DMA on a copy stream, the step runs on a compute stream, status words and the poses after the epoch come back
 * on a third; while earlier slots are in flight the caller fills the next one. Submissions execute in the order they
 * were made.
 *   kfpos_slot_acquire  waits until the slot's previous submission has completed (its outputs are then in the slot,
 *                       its inputs may be overwritten) and returns the slot's pointers
 *   kfpos_slot_submit   flags = one KFPOS_SLOT_* kind | options; dt_shared is used unless KFPOS_SLOT_DT_PER_TAG
 *   kfpos_slot_wait     waits for the slot's submission; status / pos of the slot are valid afterwards
 * The synchronous host API and the state accessors first wait for everything the slots have in flight. */
typedef struct kfpos_epoch_slot {
    int32_t  *range_mm; /* [max_anchors][n_tags] integer mm, <= 0 = absent */
    void     *err_est;  /* [max_anchors][n_tags] kfpos_real */
    void     *accel;    /* [3][n_tags] kfpos_real (9-state handles) */
    void     *cov;      /* [9][n_tags] kfpos_real, row-major 3x3 index first */
    double   *dt;       /* [n_tags], read with KFPOS_SLOT_DT_PER_TAG (negative = tag has no epoch in this submission) */
    uint32_t *status;   /* out: [n_tags] status words of the submission */
    double   *pos;      /* out: [3][n_tags] positions after the epoch (getPose at timeLag 0), unless KFPOS_SLOT_NO_POSE */
} kfpos_epoch_slot;
#define KFPOS_SLOT_TOA        0 /* kfpos_step_toa: a ranging epoch (a 9-state handle re-fuses its latched IMU sample) */
#define KFPOS_SLOT_IMU        1 /* kfpos_step_imu: latch accel / cov, IMU-only estimate */
#define KFPOS_SLOT_TOA_IMU    2 /* kfpos_step_toa_imu: latch + ranging epoch */
#define KFPOS_SLOT_DT_PER_TAG 0x100 /* dt comes from the slot's dt array instead of dt_shared */
#define KFPOS_SLOT_REUSE_ERR  0x200 /* errorEstimations are those of the previous submission: not copied again */
#define KFPOS_SLOT_REUSE_COV  0x400 /* the accelerometer covariance is that of the previous submission (a sensor with a
                                       fixed covariance): not copied again */
#define KFPOS_SLOT_NO_POSE    0x800 /* do not write / return pos */
int kfpos_slot_count(const kfpos_handle *h); /* 3: one being filled, one on the bus, one computing / returning */
int kfpos_slot_acquire(kfpos_handle *h, int32_t slot, kfpos_epoch_slot *out);
int kfpos_slot_submit(kfpos_handle *h, int32_t slot, int32_t flags, double dt_shared);
int kfpos_slot_wait(kfpos_handle *h, int32_t slot);

/* A slot can also carry a row-list round (see "row-list steps"): same three slots, streams, ordering and kfpos_slot_wait;
 * a slot serves one kind of round at a time, and acquire waits for its previous submission, whichever kind it was.
 * Whole-bank and row-list submissions may be interleaved freely and execute in submission order.
 *   rows        [capacity] the row list; inputs ROW-MAJOR per listed tag, so one reporter's record is contiguous:
 *               range_mm [n][max_anchors], err_est [n][max_anchors], accel [n][3], cov [n][9], dt [n]
 *               (KFPOS_SLOT_DT_PER_TAG; negative = skip tag rows[i])
 *   out         status [n], pos [3][n] (stride n; unless KFPOS_SLOT_NO_POSE)
 *   capacity    n_tags. The arrays other than `rows` are the slot's kfpos_epoch_slot arrays seen through another layout.
 * kfpos_slot_submit_rows(flags, n): flags as kfpos_slot_submit; the list is validated on the host, in O(n), before
 * anything is enqueued (KFPOS_ERR_ARG as above, n > capacity included); n == 0 is KFPOS_OK and enqueues nothing. Only
 * bytes proportional to n cross the bus, in either direction. KFPOS_SLOT_REUSE_ERR / _COV are refused (KFPOS_ERR_ARG),
 * and a row-list round never becomes "the previous submission" a later whole-bank KFPOS_SLOT_REUSE_* refers to. */
typedef struct kfpos_rows_slot {
    int32_t  *rows;
    int32_t  *range_mm;
    void     *err_est;
    void     *accel;
    void     *cov;
    double   *dt;
    uint32_t *status;
    double   *pos;
    int32_t   capacity;
} kfpos_rows_slot;
int kfpos_slot_acquire_rows(kfpos_handle *h, int32_t slot, kfpos_rows_slot *out);
int kfpos_slot_submit_rows(kfpos_handle *h, int32_t slot, int32_t flags, int32_t n, double dt_shared);

/* A row-list round that returns what is published. KFPOS_SLOT_POSE_COV is honoured by kfpos_slot_submit_rows only
 * (kfpos_slot_submit ignores the bit): after the round's scatter, getPose at timeLag 0 runs on the compute stream for the
 * round's list, and the covariance and the velocity travel back behind status and pos. kfpos_slot_pose_rows hands out
 * the slot's pinned arrays -- cov3x3 [n][9] and vel [n][3], row-major per listed tag --, valid after kfpos_slot_wait
 * until the slot's next submission: entry i is, bit for bit, what kfpos_get_pose_rows(rows, n, &zero, 1, ...) returns
 * right after that round. The arrays (capacity x 12 doubles, pinned and on the device) are allocated by the slot's first
 * round that carries the flag; rounds without it enqueue what they always did.
 *   KFPOS_SLOT_POSE_COV | KFPOS_SLOT_NO_POSE -> KFPOS_ERR_ARG
 *   kfpos_slot_pose_rows on a slot whose last row-list round did not carry the flag (or enqueued nothing: n == 0, the
 *   IMU round of a filter without one) -> KFPOS_ERR_STATE. Either pointer may be NULL. */
#define KFPOS_SLOT_POSE_COV   0x1000
int kfpos_slot_pose_rows(kfpos_handle *h, int32_t slot, double **cov3x3 /* [n][9] */, double **vel /* [n][3] */);

/* Streaming slots: ranges as 16-bit deltas, decoded on the device. What crosses the bus in a whole-bank ranging round is
 * mostly range_mm [max_anchors][n_tags] int32; a range changes by centimetres between two epochs of one tag, so it fits an
 * int16 delta against the previous value, and the exceptions (a tag that first appears, an NLOS jump, a range beyond
 * 32.767 m from a zero base) fit a short list. With KFPOS_SLOT_RANGES_D16 a round sends one int16 code per element plus
 * that list, and a kernel (k_decode_d16) rebuilds the int32 matrix the unchanged step kernels read. Codes, encoder
 * (kfpos_d16_put) and reference decoder: kfpos_d16.h, which also defines
 *   typedef struct kfpos_delta_slot {
 *       int16_t *code;         pinned, [max_anchors][n_tags]
 *       int32_t *esc;          pinned, [esc_capacity][2]: flat index, value
 *       int32_t *n_esc;        entries used; kfpos_slot_delta sets it to 0
 *       int32_t  esc_capacity; max_anchors * n_tags: any matrix is representable
 *       int32_t *base;         host mirror [max_anchors][n_tags], shared by the slots
 *       int32_t  n_tags, max_anchors;
 *   } kfpos_delta_slot;
 * The base is one int32 [max_anchors][n_tags] matrix per handle, zero at first, and changes only through D16 rounds:
 * a host mirror (moved by the encoder) and a device copy (moved by the decode kernel), kept equal by construction.
 * Plain rounds and row-list rounds never touch the base; they may be interleaved freely with D16 rounds.
 *
 * kfpos_slot_delta(slot, out): the slot must be acquired (kfpos_slot_acquire) and not busy; opens it for a D16 round
 *   and sets *n_esc = 0. At most one slot is open at a time: opening a second one is KFPOS_ERR_STATE. The D16 blocks
 *   are allocated by the first call, as the KFPOS_SLOT_POSE_COV arrays are (per slot: code | esc, pinned and on the
 *   device; per handle: the mirror and the device base). max_anchors * n_tags > INT32_MAX -> KFPOS_ERR_ARG.
 * kfpos_slot_encode_ranges(slot, flags): convenience for callers that keep filling range_mm: encodes the open slot's int32
 *   matrix through kfpos_d16_put, in ascending order. With KFPOS_SLOT_DT_PER_TAG in `flags`, tags whose slot dt < 0 are
 *   left out. It costs a CPU pass over the matrix; producers that care write codes directly.
 * kfpos_slot_submit(flags | KFPOS_SLOT_RANGES_D16): a round without ranging (KFPOS_SLOT_IMU) -> KFPOS_ERR_ARG;
 *   kfpos_slot_submit_rows with the flag -> KFPOS_ERR_ARG; the slot was not opened -> KFPOS_ERR_STATE. The escape list
 *   is validated on the host in O(n_esc) before anything is enqueued: 0 <= n_esc <= capacity, indices strictly
 *   ascending and inside the matrix, values > 0, code[index] == KFPOS_D16_ESCAPE; otherwise KFPOS_ERR_ARG and
 *   kfpos_last_error() names the first offending entry: the kernel never sees an unchecked index. Then code and the used
 *   pairs go up on the copy stream (one copy) instead of the ranges region, the decode kernel runs on the compute
 *   stream behind them, writing the slot's device ranges region and the device base, and the step and everything after
 *   it are what they are without the flag; err, accel, cov, dt and the REUSE flags behave as ever. The submit closes
 *   the slot, whatever it returns.
 * RESTART RULE: any D16 submit that returns other than KFPOS_OK restarts the base at zero on both sides at the next
 *   kfpos_slot_delta (one rule for every refusal after the mirror has moved). So does an open slot that is submitted
 *   without the flag, as a row-list round, or opened again.
 * SKIPPED TAGS: with KFPOS_SLOT_DT_PER_TAG the codes and escape entries of a tag whose dt < 0 are not read: the tag
 *   decodes to 0 and its base is kept, so a producer may leave stale codes for silent tags (an entry's index is still
 *   checked against the matrix and the list's order).
 * KFPOS_VERSION is unchanged: detect the feature by symbol. */
#include "kfpos_d16.h"
#define KFPOS_SLOT_RANGES_D16 0x2000
int kfpos_slot_delta(kfpos_handle *h, int32_t slot, kfpos_delta_slot *out);
int kfpos_slot_encode_ranges(kfpos_handle *h, int32_t slot, int32_t flags);

/* ---- asynchronous device-buffer API (inputs already resident in HBM) ----
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = the default stream). Calls
 * enqueue work and return; the caller synchronises. Device layouts are component-major so that the
 * 64 lanes of a wavefront read 64 consecutive elements:
 *   range_mm [max_anchors][n_tags] int32      err_est [max_anchors][n_tags] kfpos_real
 *   accel    [3][n_tags] kfpos_real           cov     [9][n_tags] kfpos_real (row-major 3x3 index first)
 *   dt       [n_tags] double, or NULL to use the shared dt_shared
 *   status   [n_tags] uint32 or NULL
 *   pos      [3][n_tags] double               cov3x3  [9][n_tags] double      vel [3][n_tags] double */
int kfpos_step_toa_dev(kfpos_handle *h, const int32_t *range_mm, const void *err_est,
                       const double *dt, double dt_shared, uint32_t *status, void *stream);
int kfpos_step_imu_dev(kfpos_handle *h, const void *accel, const void *cov,
                       const double *dt, double dt_shared, uint32_t *status, void *stream);
/* latch != 0 also stores the sample in the handle (needed if a later kfpos_step_toa* call is to
 * re-fuse it); latch = 0 skips that write when every epoch brings its own sample. */
int kfpos_step_toa_imu_dev(kfpos_handle *h, const int32_t *range_mm, const void *err_est,
                           const void *accel, const void *cov, int32_t latch,
                           const double *dt, double dt_shared, uint32_t *status, void *stream);
/* kfpos_step_sensor on device buffers: data is component-major [C][n_tags] doubles */
int kfpos_step_sensor_dev(kfpos_handle *h, int32_t kind, const double *data,
                          const double *dt, double dt_shared, uint32_t *status, void *stream);
int kfpos_get_pose_dev(kfpos_handle *h, double dt_ahead, double *pos, double *cov3x3, double *vel,
                       uint32_t *status, void *stream);

/* Replay a whole trace resident in HBM: n_steps epochs, epoch s reading range_mm + s*stride_ranges
 * elements etc. (strides in elements; err_est / cov strides may be 0 to reuse one array). Equivalent, bit
 * for bit, to n_steps calls of kfpos_step_toa_dev / kfpos_step_toa_imu_dev (accel != NULL) with
 * dt_steps[s] (host array) shared by all tags -- but up to 128 epochs run inside ONE launch with every
 * tag's state resident in registers, so state traffic and launch boundaries are paid once per launch
 * instead of once per epoch (KFPOS_TRACE_CHUNK_STEPS=n in the environment caps the epochs per launch;
 * 1 = one launch per epoch).
 *   trajectory  [n_steps][3][n_tags] double or NULL: the position after every epoch, i.e. what a caller
 *               polling getPose at timeLag 0 after each epoch would have read (Posgenerator.cpp:541-548)
 *   status      [n_tags] status words of the LAST epoch, or NULL */
int kfpos_run_trace_dev(kfpos_handle *h, int32_t n_steps,
                        const int32_t *range_mm, int64_t stride_ranges,
                        const void *err_est, int64_t stride_err,
                        const void *accel, int64_t stride_accel,
                        const void *cov, int64_t stride_cov,
                        const double *dt_steps, double *trajectory, uint32_t *status, void *stream);

/* Replay an IMU-rate event schedule of the 9-state filter (KFPOS_MODEL_TOA_IMU) resident in HBM, in the node's own
 * call sequence: newIMUMeasurement arrives at the IMU's rate, several samples per ranging epoch, each a complete
 * predict + IMU-only update at its own timeLag, and newTOAMeasurement re-fuses the latched sample
 * (KalmanFilterTOAIMU.cpp:49-92). Equivalent, bit for bit, to the same events as single calls in order -- a
 * KFPOS_EVENT_IMU event is kfpos_step_imu_dev(accel_i, cov, NULL, dt_e, ...), a KFPOS_EVENT_TOA event is
 * kfpos_step_toa_dev(range_j, err_j, NULL, dt_e, ...): state, covariance as the handle stores it (compact storage is
 * rounded after every event), flags, the latched sample and its covariance, every status word and trajectory row --
 * but up to 128 events run inside ONE launch with every tag's state resident in registers
 * (KFPOS_TRACE_CHUNK_STEPS applies, as in kfpos_run_trace_dev). A TOA event that precedes the first IMU event of
 * the call fuses what the handle held latched before the call: that sample with ITS covariance, or nothing.
 * The call ends with its last sample and `cov` latched, as the single calls would leave them.
 *   kinds, dt_events  HOST arrays of n_events entries: what each event is, and its timeLag, shared by all tags
 *   range_mm, err_est the j-th TOA event reads base + j * stride elements (stride_err may be 0: one array)
 *   accel             the i-th IMU event reads base + i * stride_accel elements
 *   cov               [9][n_tags], ONE array for the whole call: a sensor covariance per sample is not supported
 *                     here -- callers that have one use the single calls
 *   trajectory        [n_events][3][n_tags] double or NULL: the position after every event
 *   status_events     [n_events][n_tags] status word of every event, or NULL
 *   status            [n_tags] status words of the LAST event, or NULL
 * Decided on the host before anything is enqueued: NULL handle, n_events < 0, a kind other than 0 or 1, or a missing
 * array for a kind that occurs (kinds / dt_events included) -> KFPOS_ERR_ARG; a handle of another model ->
 * KFPOS_ERR_MODEL; anchors unset with at least one TOA event -> KFPOS_ERR_STATE. n_events == 0 is KFPOS_OK and
 * changes nothing. KFPOS_VERSION is unchanged: detect the call by symbol. */
#define KFPOS_EVENT_IMU 0 /* newIMUMeasurement: latch the sample, predict + IMU-only update */
#define KFPOS_EVENT_TOA 1 /* newTOAMeasurement: ranging epoch, re-fusing whatever sample is latched */
int kfpos_run_events_dev(kfpos_handle *h, int32_t n_events,
                         const uint8_t *kinds, const double *dt_events,
                         const int32_t *range_mm, int64_t stride_ranges,
                         const void *err_est, int64_t stride_err,
                         const void *accel, int64_t stride_accel,
                         const void *cov,
                         double *trajectory, uint32_t *status_events, uint32_t *status, void *stream);

/* kfpos_run_events_dev for a bank whose tags each have a timeline of their own (the name follows kfpos_get_pose_each):
 * every tag carries its IMU on its own clock, ranging rounds reach tags at different moments, and in any round some
 * tags are absent. The caller merges the tags' timelines into event SLOTS. A slot's kind is shared by the bank; who
 * takes part in it, and at which timeLag, is per tag: dt_events_dev[e * n_tags + t] < 0.0 means tag t sits slot e out
 * (exactly this predicate, as in every single call with a dt array: a NaN dt runs the event). Tags that have nothing
 * in a slot get a negative dt.
 * Equivalent, bit for bit, to the slots as single calls in order -- kfpos_step_imu_dev(accel_i, cov,
 * dt_events_dev + e * n_tags, 0, ...) for a KFPOS_EVENT_IMU slot, kfpos_step_toa_dev(range_j, err_j,
 * dt_events_dev + e * n_tags, 0, ...) for a KFPOS_EVENT_TOA slot: state, covariance as the handle stores it (compact
 * storage is rounded after every event a tag ran), flags, the latched sample and its six latched covariance entries,
 * every status word and trajectory row -- but up to 128 slots run inside ONE launch (KFPOS_TRACE_CHUNK_STEPS applies).
 * A tag that sits a slot out: its status_events word is KFPOS_ST_SKIPPED, its trajectory row is its untouched position,
 * nothing of it changes, and the slot's input entries for it are never used (they may be NaN). A tag that runs no event
 * of the call keeps every stored byte: the flags word (a fresh tag stays not started), the latch, compact covariance
 * planes.
 * The latched sample: a tag's TOA events ahead of ITS OWN first IMU event in the call re-fuse what that tag had latched
 * before the call, with that sample's covariance, or nothing; from its first IMU event on the tag uses `cov`. At the end
 * only tags that sampled in the call have their last sample and `cov` latched.
 *   kinds             HOST array of n_events entries: KFPOS_EVENT_IMU / KFPOS_EVENT_TOA
 *   dt_events_dev     DEVICE, [n_events][n_tags] double: each tag's timeLag in each slot, < 0 = absent
 *   range_mm, err_est the j-th TOA slot reads base + j * stride elements (stride_err may be 0: one array); j counts
 *                     slots, not a tag's own events
 *   accel             the i-th IMU slot reads base + i * stride_accel elements
 *   cov               [9][n_tags], ONE array for the whole call (a covariance per sample: use the single calls)
 *   trajectory        [n_events][3][n_tags] double or NULL: the position after every slot
 *   status_events     [n_events][n_tags] status word of every slot, or NULL
 *   status            [n_tags] status words of the LAST slot (KFPOS_ST_SKIPPED for tags absent from it), or NULL
 * Decided on the host before anything is enqueued: NULL handle, n_events < 0, NULL kinds or dt_events_dev with
 * n_events > 0, a kind other than 0 or 1 (kfpos_last_error() names the event), or a missing array for a kind that
 * occurs -> KFPOS_ERR_ARG; a handle of another model -> KFPOS_ERR_MODEL; anchors unset with at least one TOA slot ->
 * KFPOS_ERR_STATE. n_events == 0 is KFPOS_OK and touches nothing; accel / cov may be NULL when no IMU slot occurs,
 * range_mm / err_est when no TOA slot does. KFPOS_VERSION is unchanged: detect the call by symbol. */
int kfpos_run_events_each_dev(kfpos_handle *h, int32_t n_events,
                              const uint8_t *kinds,          /* HOST, n_events: KFPOS_EVENT_IMU / KFPOS_EVENT_TOA */
                              const double *dt_events_dev,   /* DEVICE, [n_events][n_tags] */
                              const int32_t *range_mm, int64_t stride_ranges,
                              const void *err_est, int64_t stride_err,
                              const void *accel, int64_t stride_accel,
                              const void *cov,
                              double *trajectory, uint32_t *status_events, uint32_t *status, void *stream);

/* kfpos_run_trace_dev for a 6-state bank (KFPOS_MODEL_TOA) whose tags each have a timeline of their own (the ranging-only
 * counterpart of kfpos_run_events_each_dev): tags range in their own TDMA slots, so each tag's timeLag is its own, and in
 * any round part of the bank is silent. The caller merges the tags' timelines into SLOTS, every one a ranging epoch. Who
 * takes part in a slot, and at which timeLag, is per tag: dt_steps_dev[s * n_tags + t] < 0.0 means tag t sits slot s out
 * (exactly this predicate, as in every single call with a dt array: a NaN dt runs the slot). Tags that have nothing in a
 * slot get a negative dt.
 * Equivalent, bit for bit, to the slots as single calls in order -- kfpos_step_toa_dev(range_s, err_s,
 * dt_steps_dev + s * n_tags, 0, ...): position, velocity, covariance as the handle stores it (compact storage is
 * rounded after every slot a tag ran), flags, every status word (KFPOS_ST_NONFINITE judged after that slot) and every
 * trajectory row -- but up to 128 slots run inside ONE launch with every tag's state resident in registers
 * (KFPOS_TRACE_CHUNK_STEPS applies, as in kfpos_run_trace_dev), and a wavefront in which nobody takes part in a slot
 * passes it. The ordinal s counts SLOTS, not a tag's own epochs.
 * A tag that sits a slot out: its status_steps word is KFPOS_ST_SKIPPED, its trajectory row is its untouched stored
 * position (NaN for a tag still waiting for its ML initialisation), nothing of it changes, and the slot's input entries
 * for it are never used. A tag that runs no slot of the call keeps every stored byte: the flags word (a fresh tag stays
 * not started) and the compact covariance planes.
 * Not fused on one kind of handle: a small plain bank that runs the 8-lanes-per-tag kernel (at most 8 192 tags, fixed
 * start, no outlier heuristic, at most 8 anchors; KFPOS_NO_COOP=1 disables it) computes in another summation order, so
 * there the call runs its slots through that kernel, one launch per slot: the same bits as the handle's single calls,
 * without the saving.
 *   dt_steps_dev      DEVICE, [n_steps][n_tags] double: each tag's timeLag in each slot, < 0.0 = absent
 *   range_mm, err_est slot s reads base + s * stride elements (stride_err may be 0: one array)
 *   trajectory        [n_steps][3][n_tags] double or NULL: the position after every slot
 *   status_steps      [n_steps][n_tags] status word of every slot, or NULL
 *   status            [n_tags] status words of the LAST slot (KFPOS_ST_SKIPPED for tags absent from it), or NULL
 * Decided on the host before anything is enqueued, in this order: NULL handle or n_steps < 0 -> KFPOS_ERR_ARG;
 * n_steps == 0 -> KFPOS_OK, nothing touched; NULL dt_steps_dev, range_mm or err_est -> KFPOS_ERR_ARG; a handle that is
 * not KFPOS_MODEL_TOA -> KFPOS_ERR_MODEL (9-state banks: kfpos_run_events_each_dev with all kinds KFPOS_EVENT_TOA;
 * planar banks: kfpos_run_planar_events_each_dev); anchors unset -> KFPOS_ERR_STATE. The call runs on the handle's
 * device and leaves the caller's current device as it was. KFPOS_VERSION is unchanged: detect the call by symbol. */
int kfpos_run_trace_each_dev(kfpos_handle *h, int32_t n_steps,
                             const double *dt_steps_dev,   /* DEVICE, [n_steps][n_tags]; < 0.0 = tag sits the slot out */
                             const int32_t *range_mm, int64_t stride_ranges,
                             const void *err_est, int64_t stride_err,      /* stride_err may be 0: one array */
                             double *trajectory,           /* [n_steps][3][n_tags] or NULL */
                             uint32_t *status_steps,       /* [n_steps][n_tags] or NULL */
                             uint32_t *status,             /* [n_tags], the LAST slot's words, or NULL */
                             void *stream);

/* Replay a multi-sensor event schedule of the 8-state planar filter (KFPOS_MODEL_PLANAR) resident in HBM, in the
 * node's own call sequence: ranging epochs plus PX4Flow, IMU, magnetometer and compass samples, each at its own rate
 * and its own timeLag (KalmanFilter.cpp:84-229). Equivalent, bit for bit, to the same events as single calls in order
 * -- a KFPOS_PLANAR_EVENT_TOA event is kfpos_step_toa_dev(range_j, err_j, NULL, dt_e, ...), an event of kind
 * KFPOS_SENSOR_* is kfpos_step_sensor_dev(kind, sample_i, NULL, dt_e, ...): state, height, covariance as the handle
 * stores it (compact storage is rounded after every event), flags, all 15 latch rows, every status word and
 * trajectory row -- but up to 128 events run inside ONE launch with every tag's state and latched samples resident in
 * registers (KFPOS_TRACE_CHUNK_STEPS applies, as in kfpos_run_trace_dev). A PX4Flow sample of quality 0 is dropped
 * per tag, as the single call drops it: that tag sits the event out (status KFPOS_ST_SKIPPED, trajectory row = the
 * untouched position). Ranging events ahead of the call's first sensor event on a handle that never had a sensor
 * sample run the ranging-only kernel, as single calls would.
 *   kinds, dt_events  HOST arrays of n_events entries: what each event is (0..4), and its timeLag, shared by all tags
 *   in                device pointers, component-major; the n-th event of a kind reads base + n * stride elements.
 *                     Arrays of kinds that do not occur may be NULL. Zero-initialise the struct.
 *   trajectory        [n_events][3][n_tags] double or NULL: x, y, height after every event
 *   status_events     [n_events][n_tags] status word of every event, or NULL
 *   status            [n_tags] status words of the LAST event, or NULL
 * Decided on the host before anything is enqueued: NULL handle, n_events < 0, a kind outside 0..4, missing kinds /
 * dt_events / in, or a missing array for a kind that occurs -> KFPOS_ERR_ARG (kfpos_last_error() names the first
 * offending event); a handle of another model -> KFPOS_ERR_MODEL; anchors unset with at least one ranging event ->
 * KFPOS_ERR_STATE. n_events == 0 is KFPOS_OK and changes nothing. KFPOS_VERSION is unchanged: detect the call by
 * symbol. */
#define KFPOS_PLANAR_EVENT_TOA 0 /* newTOAMeasurement; the other kinds are KFPOS_SENSOR_PX4FLOW .. _COMPASS (1..4) */
typedef struct kfpos_planar_inputs {
    const int32_t *range_mm; int64_t stride_ranges;  /* j-th ranging event: [max_anchors][n_tags] */
    const void    *err_est;  int64_t stride_err;     /* kfpos_real; stride may be 0: one array */
    const double  *px4flow;  int64_t stride_px4flow; /* i-th PX4Flow event: [5][n_tags] */
    const double  *imu;      int64_t stride_imu;     /* [24][n_tags] */
    const double  *mag;      int64_t stride_mag;     /* [3][n_tags] */
    const double  *compass;  int64_t stride_compass; /* [1][n_tags] */
} kfpos_planar_inputs;
int kfpos_run_planar_events_dev(kfpos_handle *h, int32_t n_events,
                                const uint8_t *kinds, const double *dt_events,
                                const kfpos_planar_inputs *in,
                                double *trajectory, uint32_t *status_events, uint32_t *status, void *stream);

/* kfpos_run_planar_events_dev for a bank whose tags each have a timeline of their own (the planar counterpart of
 * kfpos_run_events_each_dev): every robot carries its PX4Flow, IMU, magnetometer and compass on its own clock, ranging
 * rounds reach tags at different moments, and in any round some tags are absent. The caller merges the tags' timelines
 * into event SLOTS. A slot's kind is shared by the bank; who takes part in it, and at which timeLag, is per tag:
 * dt_events_dev[e * n_tags + t] < 0.0 means tag t sits slot e out (exactly this predicate, as in every single call with
 * a dt array: a NaN dt runs the event). Tags that have nothing in a slot get a negative dt.
 * Equivalent, bit for bit, to the slots as single calls in order, each with the slot's row of dt_events_dev as the
 * per-tag dt array -- kfpos_step_toa_dev(range_j, err_j, dt_events_dev + e * n_tags, 0, ...) for a
 * KFPOS_PLANAR_EVENT_TOA slot, kfpos_step_sensor_dev(kind, sample_i, dt_events_dev + e * n_tags, 0, ...) for a
 * KFPOS_SENSOR_* slot: state, height, covariance as the handle stores it (compact storage is rounded after every event
 * a tag ran), flags, all 15 latch rows, every status word and trajectory row -- but up to 128 slots run inside ONE
 * launch (KFPOS_TRACE_CHUNK_STEPS applies). The ordinals j and i count SLOTS of that kind, not a tag's own events.
 * A tag that sits a slot out: its status_events word is KFPOS_ST_SKIPPED, its trajectory row is its untouched x, y,
 * height, nothing of it changes, it does NOT latch the slot's sample (dt is looked at ahead of the sample), and the
 * slot's input entries for it are never used (they may be NaN). A present tag whose PX4Flow sample has quality 0 is
 * dropped as in the single call: KFPOS_ST_SKIPPED, an untouched row, nothing latched. A tag that runs no event of the
 * call keeps every stored byte: position, velocity, compact covariance planes, latch rows and the flags word (a fresh
 * tag stays not started).
 * Latches: a slot carries what THAT tag has latched at that moment -- a compass slot the PX4Flow and IMU rows the tag
 * latched before it, a ranging slot everything the tag has latched. At the end only the latch rows of kinds a tag
 * sampled itself are written; rows never latched keep what the handle holds.
 * Ranging slots ahead of the call's first sensor slot on a handle that never had a sensor sample run the ranging-only
 * kernel, one launch per slot, as single calls would.
 *   kinds             HOST array of n_events entries: 0..4 as in kfpos_run_planar_events_dev
 *   dt_events_dev     DEVICE, [n_events][n_tags] double: each tag's timeLag in each slot, < 0.0 = absent
 *   in                device pointers, component-major; the n-th slot of a kind reads base + n * stride elements.
 *                     Arrays of kinds that do not occur may be NULL. Zero-initialise the struct.
 *   trajectory        [n_events][3][n_tags] double or NULL: x, y, height after every slot
 *   status_events     [n_events][n_tags] status word of every slot, or NULL
 *   status            [n_tags] status words of the LAST slot (KFPOS_ST_SKIPPED for tags absent from it), or NULL
 * Decided on the host before anything is enqueued: NULL handle, n_events < 0, NULL kinds / dt_events_dev / in with
 * n_events > 0, a kind outside 0..4, or a missing array for a kind that occurs -> KFPOS_ERR_ARG (kfpos_last_error()
 * names the first offending slot); a handle of another model -> KFPOS_ERR_MODEL; anchors unset with at least one
 * ranging slot -> KFPOS_ERR_STATE. n_events == 0 is KFPOS_OK and touches nothing. The call runs on the handle's device
 * and leaves the caller's current device as it was. KFPOS_VERSION is unchanged: detect the call by symbol. */
int kfpos_run_planar_events_each_dev(kfpos_handle *h, int32_t n_events,
                                     const uint8_t *kinds,          /* HOST, n_events: 0..4 as kfpos_run_planar_events_dev */
                                     const double *dt_events_dev,   /* DEVICE, [n_events][n_tags]; < 0 = tag sits the slot out */
                                     const kfpos_planar_inputs *in,
                                     double *trajectory, uint32_t *status_events, uint32_t *status, void *stream);

/* ---- multi-GPU: contiguous tag shards + ONE collective, the RCCL all-gather of poses ----
 * The reference runs one filter in one process (node_pos.cpp:176-181) and has no counterpart. Here a node that serves
 * more tags than one GPU holds cuts the batch into contiguous ranges, one handle per GPU; the filters never talk to each
 * other, and what is published -- the pose of EVERY tag (Posgenerator.cpp:541-548, batched) -- is brought together by one
 * ncclAllGather per epoch (or per launch of K epochs) over xGMI, on a side stream, double-buffered, so that it overlaps
 * the next epoch's compute. librccl is opened on first use; a process that never calls kfpos_comm_* does not load it.
 *
 * One process per GPU (MPI / a launcher of your own / torchrun):
 *     rank 0:     kfpos_comm_unique_id(id);  ...ship the 128 bytes to every rank by whatever you bootstrap with...
 *     every rank: kfpos_comm_create(world, rank, id, device, &comm);
 *                 kfpos_comm_set_total(comm, total_tags, &lo, &hi);   -> this rank's handle holds tags [lo, hi)
 *                 per epoch: kfpos_step_*_dev(h, ...); kfpos_allgather_poses(h, comm, NULL, 3, pos_all, stream);
 *                 before reading pos_all: kfpos_comm_wait(comm, stream)  (or kfpos_comm_sync(comm) on the host)
 * One process driving n GPUs from one thread:
 *     kfpos_comm_create_all(n, devices, comms);  then kfpos_allgather_poses_multi(...) once per epoch for all of them.
 */
#define KFPOS_COMM_ID_BYTES 128 /* sizeof(ncclUniqueId) */
typedef struct kfpos_comm kfpos_comm;

/* Contiguous shard [lo, hi) of `rank` out of `world`: sizes differ by at most one tag, the first total % world ranks
 * hold the extra one. Pure host arithmetic (no GPU, no RCCL). */
int kfpos_shard_range(int64_t total_tags, int32_t world, int32_t rank, int64_t *lo, int64_t *hi);

/* ncclGetUniqueId: 128 bytes that rank 0 creates and every rank passes to kfpos_comm_create. */
int kfpos_comm_unique_id(void *id_out);
/* ncclCommInitRank on `device` (collective: returns when all `world` ranks have called it). */
int kfpos_comm_create(int32_t world, int32_t rank, const void *unique_id, int32_t device, kfpos_comm **out);
/* ncclCommInitAll: n communicators of one clique for one process; devices = NULL means 0..n-1. out: n pointers. */
int kfpos_comm_create_all(int32_t n_devices, const int32_t *devices, kfpos_comm **out);
int kfpos_comm_destroy(kfpos_comm *c);
int kfpos_comm_world(const kfpos_comm *c);
int kfpos_comm_rank(const kfpos_comm *c);
/* The size of the whole batch; fixes this rank's shard (returned in lo / hi, may be NULL) and the padded block size of
 * the collective. Call before the first gather, on every rank with the same total (>= world). */
int kfpos_comm_set_total(kfpos_comm *c, int64_t total_tags, int64_t *lo, int64_t *hi);

/* All-gather of pose blocks (device pointers, component-major, double):
 *   pos_local  [rows][t_local] this rank's block, or NULL with rows = 3 for the handle's current positions (what
 *              getPose at timeLag 0 returns for every tag of the shard); rows = 3 for one epoch, 3 K for the K epochs
 *              of a kfpos_run_trace_dev trajectory. It is copied on `stream` before the call returns to the caller,
 *              so it may be overwritten by later work on `stream` at once
 *   pos_all    [rows][total_tags] in global tag order, written on the communicator's side stream: valid after
 *              kfpos_comm_wait (device-side: `stream` waits for the last gather) or kfpos_comm_sync (host blocks)
 *   h          the shard's handle (checked against the communicator's shard size and device), or NULL when pos_local is given
 * Unequal shards are padded to the largest inside the call (an all-gather wants equal contributions) and the padding
 * is dropped again when pos_all is assembled. Two gathers may be in flight: the third waits for the first. */
int kfpos_allgather_poses(kfpos_handle *h, kfpos_comm *c, const double *pos_local, int32_t rows, double *pos_all,
                          void *stream);
/* The same for n communicators of one process (kfpos_comm_create_all) in ONE RCCL group; arrays of n entries;
 * handles, pos_local and streams may be NULL (= all NULL). */
int kfpos_allgather_poses_multi(int32_t n, kfpos_handle *const *handles, kfpos_comm *const *comms,
                                const double *const *pos_local, int32_t rows, double *const *pos_all,
                                void *const *streams);
/* How the blocks of a gather travel. COLLECTIVE: ncclAllGather, RCCL's own schedule. DIRECT: every rank sends its block
 * to each other rank and receives theirs in one RCCL group (ncclSend / ncclRecv) -- on MI355X every pair of GPUs has its
 * own xGMI link, so a rank's world-1 transfers run side by side, one hop each, where a ring passes every block through
 * world-1 hops. Same result, same buffers; which is faster at a given size is for the machine to say (bench.py times
 * both). All ranks must choose alike; default COLLECTIVE, or KFPOS_GATHER_ALGO=direct in the environment at creation. */
#define KFPOS_GATHER_COLLECTIVE 0
#define KFPOS_GATHER_DIRECT     1
int kfpos_comm_set_algorithm(kfpos_comm *c, int32_t algorithm);
int kfpos_comm_algorithm(const kfpos_comm *c);
int kfpos_comm_wait(kfpos_comm *c, void *stream);
int kfpos_comm_sync(kfpos_comm *c);
/* The assembly step alone, for a caller that gathers with a collective of its own (torch.distributed, MPI):
 * staged [world][rows][t_pad] (t_pad = largest shard of kfpos_shard_range) -> out [rows][total_tags]. */
int kfpos_assemble_poses_dev(int32_t world, int32_t rows, int64_t total_tags, const double *staged, double *out,
                             int32_t device, void *stream);
/* NCCL version code of the RCCL that was opened (e.g. 22707), 0 if none could be */
int kfpos_comm_backend_version(void);

/* ---- diagnostics ---- */
const char *kfpos_last_error(void);  /* thread-local detail of the last error (HIP failures, rejected configurations, calls out of sequence) */
const char *kfpos_strerror(int code);
int kfpos_version(void);
/* The solve counts at which the lanes of a wavefront of the 9-state kernel meet to hand the tail of the gain iteration
 * to pairs of lanes, for KFPOS_PAIR9_MEET=first,dense_until (read at kfpos_create; results do not depend on it): the
 * kernel's own schedule function on the host. out[0 .. return value) ascending, the last one 20; at most 20 entries.
 * Outside 1 <= first <= dense_until <= 20 (what kfpos_create refuses too), or out == NULL: returns -1. No GPU needed. */
int kfpos_pair9_meet_points(int32_t first, int32_t dense_until, int32_t *out);
/* name / duration helpers for benchmarks: time the last n enqueued step kernels with HIP events on the
 * stream they were launched on. kfpos_timing_begin records, kfpos_timing_end synchronises and returns ms. */
int kfpos_timing_begin(kfpos_handle *h, void *stream);
int kfpos_timing_end(kfpos_handle *h, void *stream, float *elapsed_ms);

#ifdef __cplusplus
}
#endif
#endif /* KFPOS_H */
