"""ctypes binding of libkfpos_hip.so (include/kfpos.h) -- the only compute path of this package.

There is no CPU fallback: importing works anywhere, but creating a bank raises if the HIP
library has not been built (`python -c "import __graft_entry__ as g; g.build()"`) or no GPU
is present. Mirrors the reference's estimator interface batched over T tags:
PositionEstimationAlgorithm (src/kfpos/algorithms/PositionEstimationAlgorithm.h:8-37).
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KFPOS_LIB_PATH") or os.path.join(_DIR, "csrc", "libkfpos_hip.so")  # override: A/B builds

MODEL_TOA, MODEL_TOA_IMU, MODEL_ML, MODEL_PLANAR = 0, 1, 2, 3
SENSOR_PX4FLOW, SENSOR_IMU, SENSOR_MAG, SENSOR_COMPASS = 1, 2, 3, 4
_SENSOR_WIDTH = {1: 5, 2: 24, 3: 3, 4: 1}
STORE_F64, STORE_F32, STORE_MIXED, STORE_P48 = 0, 1, 2, 3
ML_NORMAL, ML_IGNORE_N, ML_BEST = 0, 1, 2
MAX_ANCHORS = 64
CELL_TAGS = 64  # KFPOS_CELL_TAGS: rows per block of a bank with anchor cells
ST_UPDATE_SKIPPED, ST_ML_FALLBACK, ST_FEW_RANGES, ST_ML_INIT, ST_NOT_STARTED, ST_NONFINITE = 1, 2, 4, 8, 16, 32
ST_SKIPPED = 64


def st_flags(s):
    """the ST_* bits of status words (numpy)"""
    return np.asarray(s).astype(np.uint32) & 0xFF


def st_gain_iters(s):
    """KFPOS_ST_GAIN_ITERS"""
    return (np.asarray(s).astype(np.uint32) >> 8) & 0xFF


def st_ml_iters(s):
    """KFPOS_ST_ML_ITERS"""
    return (np.asarray(s).astype(np.uint32) >> 16) & 0xFF


def st_ignored(s):
    """KFPOS_ST_IGNORED: -1 where no range was left out"""
    return ((np.asarray(s).astype(np.uint32) >> 24) & 0xFF).astype(np.int32) - 1


# every symbol include/kfpos.h declares
EXPORTS = [
    "kfpos_create", "kfpos_destroy", "kfpos_init", "kfpos_set_anchors", "kfpos_set_init_positions",
    "kfpos_set_anchor_cells", "kfpos_anchor_cells",
    "kfpos_real_size", "kfpos_step_toa", "kfpos_step_imu", "kfpos_step_toa_imu", "kfpos_get_pose",
    "kfpos_get_pose_each", "kfpos_get_predicted",
    "kfpos_state_dim", "kfpos_get_state", "kfpos_set_state", "kfpos_step_toa_dev", "kfpos_step_imu_dev",
    "kfpos_step_toa_imu_dev", "kfpos_get_pose_dev", "kfpos_run_trace_dev", "kfpos_run_events_dev",
    "kfpos_run_events_each_dev", "kfpos_run_planar_events_dev", "kfpos_run_planar_events_each_dev",
    "kfpos_run_trace_each_dev", "kfpos_last_error",
    "kfpos_strerror", "kfpos_version", "kfpos_pair9_meet_points", "kfpos_timing_begin", "kfpos_timing_end",
    "kfpos_set_planar", "kfpos_step_sensor", "kfpos_step_sensor_dev", "kfpos_get_height", "kfpos_set_height",
    "kfpos_latch_dim", "kfpos_get_latch", "kfpos_set_latch",
    "kfpos_reset_tags", "kfpos_get_tags", "kfpos_set_tags",
    "kfpos_slot_count", "kfpos_slot_acquire", "kfpos_slot_submit", "kfpos_slot_wait",
    "kfpos_step_toa_rows", "kfpos_step_imu_rows", "kfpos_step_toa_imu_rows", "kfpos_step_sensor_rows",
    "kfpos_slot_acquire_rows", "kfpos_slot_submit_rows",
    "kfpos_get_pose_rows", "kfpos_get_predicted_rows", "kfpos_slot_pose_rows",
    "kfpos_slot_delta", "kfpos_slot_encode_ranges",
    "kfpos_shard_range", "kfpos_comm_unique_id", "kfpos_comm_create", "kfpos_comm_create_all", "kfpos_comm_destroy",
    "kfpos_comm_world", "kfpos_comm_rank", "kfpos_comm_set_total", "kfpos_allgather_poses",
    "kfpos_allgather_poses_multi", "kfpos_comm_wait", "kfpos_comm_sync", "kfpos_assemble_poses_dev",
    "kfpos_comm_backend_version", "kfpos_comm_set_algorithm", "kfpos_comm_algorithm",
]
GATHER_COLLECTIVE, GATHER_DIRECT = 0, 1
COMM_ID_BYTES = 128
SLOT_TOA, SLOT_IMU, SLOT_TOA_IMU = 0, 1, 2
EVENT_IMU, EVENT_TOA = 0, 1  # kfpos_run_events_dev: newIMUMeasurement / newTOAMeasurement
PLANAR_EVENT_TOA = 0  # kfpos_run_planar_events_dev: newTOAMeasurement; the other kinds are SENSOR_PX4FLOW .. SENSOR_COMPASS
SLOT_DT_PER_TAG, SLOT_REUSE_ERR, SLOT_REUSE_COV, SLOT_NO_POSE = 0x100, 0x200, 0x400, 0x800
SLOT_POSE_COV = 0x1000  # slot_submit_rows only: the round also returns cov3x3 and vel of its tags (slot_pose_rows)
SLOT_RANGES_D16 = 0x2000  # slot_submit only: the ranges travel as int16 codes + an escape list (slot_delta, kfpos_d16.h)
D16_ABSENT, D16_ESCAPE, D16_DELTA_MIN, D16_DELTA_MAX = -32768, -32767, -32766, 32767


class KfposError(RuntimeError):
    pass


class _Config(C.Structure):
    _fields_ = [("model", C.c_int32), ("n_tags", C.c_int32), ("max_anchors", C.c_int32),
                ("storage", C.c_int32), ("accel_noise", C.c_double), ("jolt", C.c_double),
                ("ignore_worst", C.c_int32), ("cost_threshold", C.c_double), ("top_n", C.c_int32),
                ("use_init_pos", C.c_int32), ("init_pos", C.c_double * 3), ("device", C.c_int32),
                ("ml_variant", C.c_int32)]


class PlanarConfig(C.Structure):
    """kfpos_planar_config: what KalmanFilter::loadConfigurationFiles reads + initialAngle."""
    _fields_ = [("use_fixed_height", C.c_int32), ("fixed_height", C.c_double), ("init_angle", C.c_double),
                ("px4_height", C.c_double), ("px4_arm_p1", C.c_double), ("px4_arm_p2", C.c_double),
                ("px4_cov_velocity", C.c_double), ("px4_cov_gyro_z", C.c_double),
                ("imu_use_fixed_cov_acc", C.c_int32), ("imu_cov_acc", C.c_double),
                ("imu_use_fixed_cov_ang_vel_z", C.c_int32), ("imu_cov_ang_vel_z", C.c_double),
                ("mag_angle_offset", C.c_double), ("mag_cov", C.c_double)]


class _EpochSlot(C.Structure):
    """kfpos_epoch_slot: pointers into one slot of the handle's pinned host memory."""
    _fields_ = [("range_mm", C.c_void_p), ("err_est", C.c_void_p), ("accel", C.c_void_p), ("cov", C.c_void_p),
                ("dt", C.c_void_p), ("status", C.c_void_p), ("pos", C.c_void_p)]


class _RowsSlot(C.Structure):
    """kfpos_rows_slot: the same pinned block seen as a row-list round, plus the slot's row list."""
    _fields_ = [("rows", C.c_void_p), ("range_mm", C.c_void_p), ("err_est", C.c_void_p), ("accel", C.c_void_p),
                ("cov", C.c_void_p), ("dt", C.c_void_p), ("status", C.c_void_p), ("pos", C.c_void_p),
                ("capacity", C.c_int32)]


class _DeltaSlot(C.Structure):
    """kfpos_delta_slot: one slot opened for a D16 round (kfpos_d16.h)."""
    _fields_ = [("code", C.c_void_p), ("esc", C.c_void_p), ("n_esc", C.c_void_p), ("esc_capacity", C.c_int32),
                ("base", C.c_void_p), ("n_tags", C.c_int32), ("max_anchors", C.c_int32)]


class PlanarInputs(C.Structure):
    """kfpos_planar_inputs: device pointers and strides (elements) of a planar event schedule's inputs."""
    _fields_ = [("range_mm", C.c_void_p), ("stride_ranges", C.c_int64), ("err_est", C.c_void_p), ("stride_err", C.c_int64),
                ("px4flow", C.c_void_p), ("stride_px4flow", C.c_int64), ("imu", C.c_void_p), ("stride_imu", C.c_int64),
                ("mag", C.c_void_p), ("stride_mag", C.c_int64), ("compass", C.c_void_p), ("stride_compass", C.c_int64)]


_lib = None


def load():
    """Load the HIP library; raises KfposError (never falls back) when it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise KfposError(f"{LIB_PATH} is not built: run __graft_entry__.build() (hipcc --offload-arch=gfx950)")
    try:
        # PyTorch wheels bundle their own libamdhip64.so.7; whichever copy is loaded first serves the whole
        # process. If torch is going to share this process (device tensors, RCCL) its copy has to be that
        # one, otherwise torch.cuda later reports "No HIP GPUs are available".
        import torch  # noqa: F401
    except Exception:
        pass
    L = C.CDLL(LIB_PATH)
    vp, i32, f64 = C.c_void_p, C.c_int32, C.c_double

    def sig(name, argtypes):
        # an A/B build from an older revision (KFPOS_LIB_PATH) may lack the newest entry points: calling one then
        # fails with AttributeError, everything else works
        if hasattr(L, name):
            getattr(L, name).argtypes = argtypes

    sig("kfpos_create", [C.POINTER(_Config), C.POINTER(vp)])
    sig("kfpos_destroy", [vp])
    sig("kfpos_init", [vp])
    sig("kfpos_set_anchors", [vp, vp, vp, i32])
    sig("kfpos_set_init_positions", [vp, vp])
    sig("kfpos_set_anchor_cells", [vp, i32, i32, vp, vp])
    sig("kfpos_anchor_cells", [vp])
    sig("kfpos_real_size", [vp])
    sig("kfpos_state_dim", [vp])
    sig("kfpos_step_toa", [vp, vp, vp, vp, i32, vp])
    sig("kfpos_step_imu", [vp, vp, vp, vp, i32, vp])
    sig("kfpos_step_toa_imu", [vp, vp, vp, vp, vp, vp, i32, vp])
    sig("kfpos_get_pose", [vp, f64, vp, vp, vp, vp])
    sig("kfpos_get_pose_each", [vp, vp, vp, vp, vp, vp])
    sig("kfpos_get_predicted", [vp, vp, i32, vp, vp, vp])
    sig("kfpos_get_state", [vp, vp, vp, vp])
    sig("kfpos_set_state", [vp, vp, vp, vp])
    sig("kfpos_step_toa_dev", [vp, vp, vp, vp, f64, vp, vp])
    sig("kfpos_step_imu_dev", [vp, vp, vp, vp, f64, vp, vp])
    sig("kfpos_step_toa_imu_dev", [vp, vp, vp, vp, vp, i32, vp, f64, vp, vp])
    sig("kfpos_get_pose_dev", [vp, f64, vp, vp, vp, vp, vp])
    L.kfpos_run_trace_dev.argtypes = [vp, i32, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64,
                                      vp, vp, vp, vp]
    sig("kfpos_run_events_dev", [vp, i32, vp, vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp])
    sig("kfpos_run_events_each_dev", [vp, i32, vp, vp, vp, C.c_int64, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp, vp])
    sig("kfpos_run_planar_events_dev", [vp, i32, vp, vp, C.POINTER(PlanarInputs), vp, vp, vp, vp])
    sig("kfpos_run_planar_events_each_dev", [vp, i32, vp, vp, C.POINTER(PlanarInputs), vp, vp, vp, vp])
    sig("kfpos_run_trace_each_dev", [vp, i32, vp, vp, C.c_int64, vp, C.c_int64, vp, vp, vp, vp])
    sig("kfpos_set_planar", [vp, C.POINTER(PlanarConfig)])
    sig("kfpos_step_sensor", [vp, i32, vp, vp, i32, vp])
    sig("kfpos_step_sensor_dev", [vp, i32, vp, vp, f64, vp, vp])
    sig("kfpos_get_height", [vp, vp])
    sig("kfpos_set_height", [vp, vp])
    sig("kfpos_latch_dim", [vp])
    sig("kfpos_get_latch", [vp, vp])
    sig("kfpos_set_latch", [vp, vp])
    sig("kfpos_reset_tags", [vp, vp, i32, vp])
    sig("kfpos_get_tags", [vp, vp, i32, vp, vp, vp, vp, vp])
    sig("kfpos_set_tags", [vp, vp, i32, vp, vp, vp, vp, vp])
    sig("kfpos_slot_count", [vp])
    sig("kfpos_slot_acquire", [vp, i32, C.POINTER(_EpochSlot)])
    sig("kfpos_slot_submit", [vp, i32, i32, f64])
    sig("kfpos_slot_wait", [vp, i32])
    sig("kfpos_step_toa_rows", [vp, vp, i32, vp, vp, vp, i32, vp])
    sig("kfpos_step_imu_rows", [vp, vp, i32, vp, vp, vp, i32, vp])
    sig("kfpos_step_toa_imu_rows", [vp, vp, i32, vp, vp, vp, vp, vp, i32, vp])
    sig("kfpos_step_sensor_rows", [vp, vp, i32, i32, vp, vp, i32, vp])
    sig("kfpos_slot_acquire_rows", [vp, i32, C.POINTER(_RowsSlot)])
    sig("kfpos_slot_submit_rows", [vp, i32, i32, i32, f64])
    sig("kfpos_get_pose_rows", [vp, vp, i32, vp, i32, vp, vp, vp, vp])
    sig("kfpos_get_predicted_rows", [vp, vp, i32, vp, i32, vp, vp, vp])
    sig("kfpos_slot_pose_rows", [vp, i32, C.POINTER(vp), C.POINTER(vp)])
    sig("kfpos_slot_delta", [vp, i32, C.POINTER(_DeltaSlot)])
    sig("kfpos_slot_encode_ranges", [vp, i32, i32])
    sig("kfpos_timing_begin", [vp, vp])
    sig("kfpos_timing_end", [vp, vp, C.POINTER(C.c_float)])
    i64 = C.c_int64
    sig("kfpos_shard_range", [i64, i32, i32, C.POINTER(i64), C.POINTER(i64)])
    sig("kfpos_comm_unique_id", [vp])
    sig("kfpos_comm_create", [i32, i32, vp, i32, C.POINTER(vp)])
    sig("kfpos_comm_create_all", [i32, vp, C.POINTER(vp)])
    sig("kfpos_comm_destroy", [vp])
    sig("kfpos_comm_world", [vp])
    sig("kfpos_comm_rank", [vp])
    sig("kfpos_comm_set_total", [vp, i64, C.POINTER(i64), C.POINTER(i64)])
    sig("kfpos_allgather_poses", [vp, vp, vp, i32, vp, vp])
    sig("kfpos_allgather_poses_multi", [i32, vp, vp, vp, i32, vp, vp])
    sig("kfpos_comm_wait", [vp, vp])
    sig("kfpos_comm_sync", [vp])
    sig("kfpos_assemble_poses_dev", [i32, i32, i64, vp, vp, i32, vp])
    sig("kfpos_comm_backend_version", [])
    sig("kfpos_comm_set_algorithm", [vp, i32])
    sig("kfpos_comm_algorithm", [vp])
    L.kfpos_last_error.restype = C.c_char_p
    L.kfpos_strerror.restype = C.c_char_p
    sig("kfpos_strerror", [C.c_int])
    sig("kfpos_pair9_meet_points", [i32, i32, C.POINTER(i32)])
    _lib = L
    return L


def _ptr(x):
    """device pointer from an int, None, or anything with data_ptr() (torch tensors)."""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return x.data_ptr()
    return int(x)


class KfposBank:
    """T independent filters on one GPU (KalmanFilterTOA or KalmanFilterTOAIMU semantics per tag)."""

    def __init__(self, model, n_tags, anchors, storage=STORE_F64, accel_noise=0.5, jolt=0.5,
                 ignore_worst=False, cost_threshold=0.5, top_n=0, init_pos=None, device=0,
                 max_anchors=None, planar=None, ml_variant=0):
        self._h = None
        self.lib = load()
        anchors = np.ascontiguousarray(anchors, dtype=np.float64)
        self.T, self.A = int(n_tags), int(max_anchors or anchors.shape[0])
        self.model, self.storage = model, storage
        self.real = np.float64 if storage == STORE_F64 else np.float32  # kfpos_real: measurement element type
        cfg = _Config()
        cfg.model, cfg.n_tags, cfg.max_anchors, cfg.storage = model, self.T, self.A, storage
        cfg.accel_noise, cfg.jolt = accel_noise, jolt
        cfg.ignore_worst, cfg.cost_threshold, cfg.top_n = int(ignore_worst), cost_threshold, top_n
        cfg.use_init_pos = int(init_pos is not None)
        per_tag = None
        if init_pos is not None:
            ip = np.asarray(init_pos, dtype=np.float64)
            if ip.shape == (3,):
                cfg.init_pos = (C.c_double * 3)(*ip)
            else:
                assert ip.shape == (self.T, 3)
                per_tag = np.ascontiguousarray(ip)
        cfg.device = device
        cfg.ml_variant = ml_variant  # MODEL_ML: ML_NORMAL / ML_IGNORE_N / ML_BEST
        h = C.c_void_p()
        self._chk(self.lib.kfpos_create(C.byref(cfg), C.byref(h)))
        self._h = h
        self._chk(self.lib.kfpos_init(h))
        self._chk(self.lib.kfpos_set_anchors(h, anchors.ctypes.data, None, anchors.shape[0]))
        if model == MODEL_PLANAR:  # KalmanFilter::init(): the XML configuration (dict of PlanarConfig fields)
            self.planar = PlanarConfig(**(planar or {}))
            self._chk(self.lib.kfpos_set_planar(h, C.byref(self.planar)))
        if per_tag is not None:
            self._chk(self.lib.kfpos_set_init_positions(h, per_tag.ctypes.data))
        self.n = self.lib.kfpos_state_dim(h)

    def _chk(self, rc):
        if rc != 0:
            msg = self.lib.kfpos_strerror(rc).decode()
            detail = self.lib.kfpos_last_error().decode()
            if detail:
                msg += ": " + detail
            raise KfposError(msg)

    def close(self):
        if self._h:
            self.lib.kfpos_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- anchor cells: an anchor table per block of CELL_TAGS rows, one launch for all of them ----
    def set_anchor_cells(self, tables, cell_of_block):
        """kfpos_set_anchor_cells: tables (n_cells, n_anchors, 3) in metres, n_anchors <= max_anchors; cell_of_block
        ((T + 63) // 64,): the cell of rows [64 b, 64 b + 64). Whole-bank ranging rounds then range every block against
        its cell's table, bit for bit what a bank with that one table computes for those rows; row-list steps and the
        event / per-tag replays refuse such a bank (KfposError). May be repeated; set_anchors() returns to one table."""
        t = np.ascontiguousarray(tables, dtype=np.float64)
        m = np.ascontiguousarray(cell_of_block, dtype=np.int32)
        assert t.ndim == 3 and t.shape[2] == 3, t.shape
        assert m.shape == ((self.T + CELL_TAGS - 1) // CELL_TAGS,), m.shape
        self._chk(self.lib.kfpos_set_anchor_cells(self._h, t.shape[0], t.shape[1], t.ctypes.data, m.ctypes.data))

    @property
    def anchor_cells(self):
        """cells in force; 0 = one table for the whole bank"""
        return int(self.lib.kfpos_anchor_cells(self._h))

    def set_anchors(self, anchors):
        """kfpos_set_anchors: one table (n_anchors, 3) for the whole bank (a bank with cells returns to one table)"""
        a = np.ascontiguousarray(anchors, dtype=np.float64)
        assert a.ndim == 2 and a.shape[1] == 3, a.shape
        self._chk(self.lib.kfpos_set_anchors(self._h, a.ctypes.data, None, a.shape[0]))

    # ---- host-buffer API ------------------------------------------------------
    def _dt(self, dt):
        d = np.atleast_1d(np.ascontiguousarray(dt, dtype=np.float64))
        assert d.size in (1, self.T)
        return d

    def step_toa(self, range_mm, err_est, dt):
        r = np.ascontiguousarray(range_mm, dtype=np.int32)
        e = np.ascontiguousarray(err_est, dtype=self.real)
        assert r.shape == (self.T, self.A) and e.shape == (self.T, self.A)
        d, st = self._dt(dt), np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_toa(self._h, r.ctypes.data, e.ctypes.data, d.ctypes.data, d.size,
                                          st.ctypes.data))
        return st

    def step_imu(self, accel, cov, dt):
        a = np.ascontiguousarray(accel, dtype=self.real)
        c = np.ascontiguousarray(cov, dtype=self.real)
        assert a.shape == (self.T, 3) and c.shape == (self.T, 9)
        d, st = self._dt(dt), np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_imu(self._h, a.ctypes.data, c.ctypes.data, d.ctypes.data, d.size,
                                          st.ctypes.data))
        return st

    def step_toa_imu(self, range_mm, err_est, accel, cov, dt):
        r = np.ascontiguousarray(range_mm, dtype=np.int32)
        e = np.ascontiguousarray(err_est, dtype=self.real)
        a = np.ascontiguousarray(accel, dtype=self.real)
        c = np.ascontiguousarray(cov, dtype=self.real)
        assert r.shape == (self.T, self.A) and e.shape == (self.T, self.A)
        assert a.shape == (self.T, 3) and c.shape == (self.T, 9)
        d, st = self._dt(dt), np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_toa_imu(self._h, r.ctypes.data, e.ctypes.data, a.ctypes.data,
                                              c.ctypes.data, d.ctypes.data, d.size, st.ctypes.data))
        return st

    def step_sensor(self, kind, data, dt):
        """KalmanFilter's other four entry points (MODEL_PLANAR): SENSOR_PX4FLOW (T, 5), SENSOR_IMU (T, 24),
        SENSOR_MAG (T, 3), SENSOR_COMPASS (T,)."""
        x = np.ascontiguousarray(data, dtype=np.float64).reshape(self.T, -1)
        assert x.shape[1] == _SENSOR_WIDTH[kind]
        d, st = self._dt(dt), np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_sensor(self._h, kind, x.ctypes.data, d.ctypes.data, d.size, st.ctypes.data))
        return st

    def step_px4flow(self, flow, dt):
        return self.step_sensor(SENSOR_PX4FLOW, flow, dt)

    def step_planar_imu(self, ang_vel, cov_ang_vel, lin_acc, cov_acc, dt):
        return self.step_sensor(SENSOR_IMU, np.concatenate([ang_vel, cov_ang_vel, lin_acc, cov_acc], axis=1), dt)

    def step_mag(self, mag_xyz, dt):
        return self.step_sensor(SENSOR_MAG, mag_xyz, dt)

    def step_compass(self, compass, dt):
        return self.step_sensor(SENSOR_COMPASS, compass, dt)

    def get_height(self):
        z = np.zeros(self.T)
        self._chk(self.lib.kfpos_get_height(self._h, z.ctypes.data))
        return z

    def set_height(self, z):
        a = np.ascontiguousarray(z, dtype=np.float64)
        assert a.shape == (self.T,)
        self._chk(self.lib.kfpos_set_height(self._h, a.ctypes.data))

    def get_pose(self, dt_ahead=0.0):
        pos, cov, vel = np.zeros((self.T, 3)), np.zeros((self.T, 9)), np.zeros((self.T, 3))
        st = np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_get_pose(self._h, dt_ahead, pos.ctypes.data, cov.ctypes.data,
                                          vel.ctypes.data, st.ctypes.data))
        return pos, cov.reshape(self.T, 3, 3), vel, st

    def get_pose_each(self, dt_ahead):
        d = np.ascontiguousarray(dt_ahead, dtype=np.float64)
        assert d.shape == (self.T,)
        pos, cov, vel = np.zeros((self.T, 3)), np.zeros((self.T, 9)), np.zeros((self.T, 3))
        st = np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_get_pose_each(self._h, d.ctypes.data, pos.ctypes.data, cov.ctypes.data,
                                               vel.ctypes.data, st.ctypes.data))
        return pos, cov.reshape(self.T, 3, 3), vel, st

    def get_predicted(self, dt_ahead):
        d = np.atleast_1d(np.ascontiguousarray(dt_ahead, dtype=np.float64))
        assert d.size in (1, self.T)
        x, P = np.zeros((self.T, self.n)), np.zeros((self.T, self.n, self.n))
        st = np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_get_predicted(self._h, d.ctypes.data, d.size, x.ctypes.data, P.ctypes.data,
                                               st.ctypes.data))
        return x, P, st

    def get_state(self):
        x, P = np.zeros((self.T, self.n)), np.zeros((self.T, self.n, self.n))
        fl = np.zeros(self.T, dtype=np.uint32)
        self._chk(self.lib.kfpos_get_state(self._h, x.ctypes.data, P.ctypes.data, fl.ctypes.data))
        return x, P, fl

    def set_state(self, x, P, flags=None):
        x = np.ascontiguousarray(x, dtype=np.float64)
        P = np.ascontiguousarray(P, dtype=np.float64)
        fl = None if flags is None else np.ascontiguousarray(flags, dtype=np.uint32)
        self._chk(self.lib.kfpos_set_state(self._h, x.ctypes.data, P.ctypes.data,
                                           None if fl is None else fl.ctypes.data))

    def get_latch(self):
        """Latched sensor samples (T, kfpos_latch_dim): with get_state() a complete checkpoint."""
        out = np.zeros((self.T, self.lib.kfpos_latch_dim(self._h)))
        self._chk(self.lib.kfpos_get_latch(self._h, out.ctypes.data if out.size else None))
        return out

    def set_latch(self, latch):
        a = np.ascontiguousarray(latch, dtype=np.float64)
        assert a.shape == (self.T, self.lib.kfpos_latch_dim(self._h))
        self._chk(self.lib.kfpos_set_latch(self._h, a.ctypes.data if a.size else None))

    # ---- per-tag lifecycle: chosen rows only, on the device (cost follows len(rows), not T) ----
    @staticmethod
    def _rows(rows):
        r = np.ascontiguousarray(rows, dtype=np.int32)
        assert r.ndim == 1
        return r

    def reset_tags(self, rows, init_pos=None):
        """The listed tags go back to what a fresh bank holds: not started, P = 0, latches cleared; position =
        init_pos ((3,) or (len(rows), 3)), the bank's init_pos when None, NaN on a bank that starts by ML."""
        r = self._rows(rows)
        ip = None
        if init_pos is not None:
            ip = np.ascontiguousarray(np.broadcast_to(np.asarray(init_pos, dtype=np.float64), (r.size, 3)))
        self._chk(self.lib.kfpos_reset_tags(self._h, r.ctypes.data, r.size, None if ip is None else ip.ctypes.data))

    def get_tags(self, rows):
        """Rows `rows` of get_state() / get_latch() / get_height(): (x, P, flags, latch, height or None)."""
        r = self._rows(rows)
        m = r.size
        x, P = np.zeros((m, self.n)), np.zeros((m, self.n, self.n))
        fl = np.zeros(m, dtype=np.uint32)
        latch = np.zeros((m, self.lib.kfpos_latch_dim(self._h)))
        z = np.zeros(m) if self.model == MODEL_PLANAR else None
        self._chk(self.lib.kfpos_get_tags(self._h, r.ctypes.data, m, x.ctypes.data, P.ctypes.data, fl.ctypes.data,
                                          latch.ctypes.data if latch.shape[1] else None,
                                          None if z is None else z.ctypes.data))
        return x, P, fl, latch, z

    def set_tags(self, rows, x=None, P=None, flags=None, latch=None, height=None):
        """The inverse of get_tags; a part left None stays as it is in the listed tags."""
        r = self._rows(rows)
        m = r.size

        def arr(v, shape, dtype=np.float64):
            if v is None:
                return None
            a = np.ascontiguousarray(v, dtype=dtype)
            assert a.shape == shape, (a.shape, shape)
            return a

        x, P = arr(x, (m, self.n)), arr(P, (m, self.n, self.n))
        fl = arr(flags, (m,), np.uint32)
        L = self.lib.kfpos_latch_dim(self._h)
        latch = arr(latch, (m, L))
        z = arr(height, (m,))
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        self._chk(self.lib.kfpos_set_tags(self._h, r.ctypes.data, m, ptr(x), ptr(P), ptr(fl),
                                          None if L == 0 else ptr(latch), ptr(z)))

    # ---- row-list steps: an epoch for the listed rows only; inputs are per listed tag, (len(rows), ...) ----
    def _dt_rows(self, dt, m):
        d = np.atleast_1d(np.ascontiguousarray(dt, dtype=np.float64))
        assert d.size in (1, m)
        return d

    def step_toa_rows(self, rows, range_mm, err_est, dt):
        """step_toa for the tags in `rows` (everyone else: untouched, as with dt < 0); returns their status words."""
        q = self._rows(rows)
        r = np.ascontiguousarray(range_mm, dtype=np.int32)
        e = np.ascontiguousarray(err_est, dtype=self.real)
        assert r.shape == (q.size, self.A) and e.shape == (q.size, self.A)
        d, st = self._dt_rows(dt, q.size), np.zeros(q.size, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_toa_rows(self._h, q.ctypes.data, q.size, r.ctypes.data, e.ctypes.data,
                                               d.ctypes.data, d.size, st.ctypes.data))
        return st

    def step_imu_rows(self, rows, accel, cov, dt):
        q = self._rows(rows)
        a = np.ascontiguousarray(accel, dtype=self.real)
        c = np.ascontiguousarray(cov, dtype=self.real)
        assert a.shape == (q.size, 3) and c.shape == (q.size, 9)
        d, st = self._dt_rows(dt, q.size), np.zeros(q.size, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_imu_rows(self._h, q.ctypes.data, q.size, a.ctypes.data, c.ctypes.data,
                                               d.ctypes.data, d.size, st.ctypes.data))
        return st

    def step_toa_imu_rows(self, rows, range_mm, err_est, accel, cov, dt):
        q = self._rows(rows)
        r = np.ascontiguousarray(range_mm, dtype=np.int32)
        e = np.ascontiguousarray(err_est, dtype=self.real)
        a = np.ascontiguousarray(accel, dtype=self.real)
        c = np.ascontiguousarray(cov, dtype=self.real)
        assert r.shape == (q.size, self.A) and e.shape == (q.size, self.A)
        assert a.shape == (q.size, 3) and c.shape == (q.size, 9)
        d, st = self._dt_rows(dt, q.size), np.zeros(q.size, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_toa_imu_rows(self._h, q.ctypes.data, q.size, r.ctypes.data, e.ctypes.data,
                                                   a.ctypes.data, c.ctypes.data, d.ctypes.data, d.size,
                                                   st.ctypes.data))
        return st

    def step_sensor_rows(self, rows, kind, data, dt):
        q = self._rows(rows)
        x = np.ascontiguousarray(data, dtype=np.float64).reshape(q.size, -1)
        assert x.shape[1] == _SENSOR_WIDTH[kind]
        d, st = self._dt_rows(dt, q.size), np.zeros(q.size, dtype=np.uint32)
        self._chk(self.lib.kfpos_step_sensor_rows(self._h, q.ctypes.data, q.size, kind, x.ctypes.data,
                                                  d.ctypes.data, d.size, st.ctypes.data))
        return st

    # ---- pose for a row list: getPose for the listed rows only (cost follows len(rows), not T) ----
    def get_pose_rows(self, rows, dt_ahead):
        """get_pose_each for the entries of `rows` (rows may repeat): dt_ahead is one value or one per ENTRY. Returns
        (pos (m, 3), cov (m, 3, 3), vel (m, 3), status (m,)), bit for bit the whole-bank call's rows."""
        r = self._rows(rows)
        m = r.size
        d = self._dt_rows(dt_ahead, m)
        pos, cov, vel = np.zeros((m, 3)), np.zeros((m, 9)), np.zeros((m, 3))
        st = np.zeros(m, dtype=np.uint32)
        self._chk(self.lib.kfpos_get_pose_rows(self._h, r.ctypes.data, m, d.ctypes.data, d.size, pos.ctypes.data,
                                               cov.ctypes.data, vel.ctypes.data, st.ctypes.data))
        return pos, cov.reshape(m, 3, 3), vel, st

    def get_predicted_rows(self, rows, dt_ahead):
        """get_predicted for the entries of `rows`: (x (m, n), P (m, n, n), status (m,))."""
        r = self._rows(rows)
        m = r.size
        d = self._dt_rows(dt_ahead, m)
        x, P = np.zeros((m, self.n)), np.zeros((m, self.n, self.n))
        st = np.zeros(m, dtype=np.uint32)
        self._chk(self.lib.kfpos_get_predicted_rows(self._h, r.ctypes.data, m, d.ctypes.data, d.size, x.ctypes.data,
                                                    P.ctypes.data, st.ctypes.data))
        return x, P, st

    # ---- streaming host API: epochs assembled in place in pinned, component-major slots ----
    def slot_acquire(self, slot):
        """Wait for the slot's previous submission; returns numpy views over the slot's pinned memory:
        dict(range_mm [A][T] int32, err_est [A][T], accel [3][T], cov [9][T], dt [T], status [T], pos [3][T])."""
        sl = _EpochSlot()
        self._chk(self.lib.kfpos_slot_acquire(self._h, slot, C.byref(sl)))
        T, A = self.T, self.A

        def view(ptr, shape, dtype):
            n = int(np.prod(shape))
            buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

        return {"range_mm": view(sl.range_mm, (A, T), np.int32), "err_est": view(sl.err_est, (A, T), self.real),
                "accel": view(sl.accel, (3, T), self.real), "cov": view(sl.cov, (9, T), self.real),
                "dt": view(sl.dt, (T,), np.float64), "status": view(sl.status, (T,), np.uint32),
                "pos": view(sl.pos, (3, T), np.float64)}

    def slot_submit(self, slot, flags, dt_shared=0.0):
        self._chk(self.lib.kfpos_slot_submit(self._h, slot, int(flags), float(dt_shared)))

    def slot_wait(self, slot):
        self._chk(self.lib.kfpos_slot_wait(self._h, slot))

    def slot_acquire_rows(self, slot):
        """The slot as a row-list round: numpy views at full capacity (T listed tags), row-major per listed tag:
        dict(rows [T], range_mm [T][A], err_est [T][A], accel [T][3], cov [T][9], dt [T], status [T], pos (flat 3 T:
        after a round of n tags its first 3 n doubles are [3][n])). Fill the first n entries, then slot_submit_rows."""
        sl = _RowsSlot()
        self._chk(self.lib.kfpos_slot_acquire_rows(self._h, slot, C.byref(sl)))
        T, A = self.T, self.A

        def view(ptr, shape, dtype):
            n = int(np.prod(shape))
            buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

        return {"rows": view(sl.rows, (T,), np.int32),
                "range_mm": view(sl.range_mm, (T, A), np.int32), "err_est": view(sl.err_est, (T, A), self.real),
                "accel": view(sl.accel, (T, 3), self.real), "cov": view(sl.cov, (T, 9), self.real),
                "dt": view(sl.dt, (T,), np.float64), "status": view(sl.status, (T,), np.uint32),
                "pos": view(sl.pos, (3 * T,), np.float64)}

    def slot_submit_rows(self, slot, flags, n, dt_shared=0.0):
        self._chk(self.lib.kfpos_slot_submit_rows(self._h, slot, int(flags), int(n), float(dt_shared)))

    def slot_pose_rows(self, slot, n):
        """After slot_wait of a round submitted with SLOT_POSE_COV: views (cov (n, 3, 3), vel (n, 3)) over the slot's
        pinned arrays -- what get_pose_rows(rows, 0.0) returned right after that round."""
        cov, vel = C.c_void_p(), C.c_void_p()
        self._chk(self.lib.kfpos_slot_pose_rows(self._h, slot, C.byref(cov), C.byref(vel)))

        def view(ptr, shape):
            cnt = int(np.prod(shape))
            buf = (C.c_char * (cnt * 8)).from_address(ptr)
            return np.frombuffer(buf, dtype=np.float64, count=cnt).reshape(shape)

        return view(cov.value, (int(n), 3, 3)), view(vel.value, (int(n), 3))

    def slot_delta(self, slot):
        """Open an acquired slot for a D16 round (submit it with SLOT_RANGES_D16): numpy views over the slot's pinned
        memory and the handle's host mirror: dict(code (A, T) int16, esc (cap, 2) int32: flat index, value, n_esc (1,)
        int32, base (A, T) int32). Codes and the encoder's rule: include/kfpos_d16.h."""
        sl = _DeltaSlot()
        self._chk(self.lib.kfpos_slot_delta(self._h, slot, C.byref(sl)))
        T, A = self.T, self.A

        def view(ptr, shape, dtype):
            n = int(np.prod(shape))
            buf = (C.c_char * (n * np.dtype(dtype).itemsize)).from_address(ptr)
            return np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)

        return {"code": view(sl.code, (A, T), np.int16), "esc": view(sl.esc, (sl.esc_capacity, 2), np.int32),
                "n_esc": view(sl.n_esc, (1,), np.int32), "base": view(sl.base, (A, T), np.int32)}

    def slot_encode_ranges(self, slot, flags=0):
        """Encode the open slot's range_mm into its codes and escape list (with SLOT_DT_PER_TAG in flags: tags whose
        slot dt < 0 are left out)."""
        self._chk(self.lib.kfpos_slot_encode_ranges(self._h, slot, int(flags)))

    # ---- device-buffer API (pointers: ints or torch tensors; layouts in include/kfpos.h) ----
    def step_toa_dev(self, range_mm, err_est, dt, status=None, stream=None, dt_dev=None):
        self._chk(self.lib.kfpos_step_toa_dev(self._h, _ptr(range_mm), _ptr(err_est), _ptr(dt_dev), float(dt),
                                              _ptr(status), _ptr(stream)))

    def step_imu_dev(self, accel, cov, dt, status=None, stream=None, dt_dev=None):
        self._chk(self.lib.kfpos_step_imu_dev(self._h, _ptr(accel), _ptr(cov), _ptr(dt_dev), float(dt),
                                              _ptr(status), _ptr(stream)))

    def step_toa_imu_dev(self, range_mm, err_est, accel, cov, dt, latch=True, status=None, stream=None,
                         dt_dev=None):
        self._chk(self.lib.kfpos_step_toa_imu_dev(self._h, _ptr(range_mm), _ptr(err_est), _ptr(accel),
                                                  _ptr(cov), int(latch), _ptr(dt_dev), float(dt),
                                                  _ptr(status), _ptr(stream)))

    def step_sensor_dev(self, kind, data, dt, status=None, stream=None, dt_dev=None):
        self._chk(self.lib.kfpos_step_sensor_dev(self._h, int(kind), _ptr(data), _ptr(dt_dev), float(dt),
                                                 _ptr(status), _ptr(stream)))

    def get_pose_dev(self, dt_ahead, pos=None, cov=None, vel=None, status=None, stream=None):
        self._chk(self.lib.kfpos_get_pose_dev(self._h, float(dt_ahead), _ptr(pos), _ptr(cov), _ptr(vel),
                                              _ptr(status), _ptr(stream)))

    def run_trace_dev(self, n_steps, range_mm, stride_ranges, err_est, stride_err, dt_steps, accel=None,
                      stride_accel=0, cov=None, stride_cov=0, trajectory=None, status=None, stream=None):
        d = np.ascontiguousarray(dt_steps, dtype=np.float64)
        assert d.size >= n_steps
        self._chk(self.lib.kfpos_run_trace_dev(self._h, n_steps, _ptr(range_mm), stride_ranges, _ptr(err_est),
                                               stride_err, _ptr(accel), stride_accel, _ptr(cov), stride_cov,
                                               d.ctypes.data, _ptr(trajectory), _ptr(status), _ptr(stream)))

    def run_events_dev(self, kinds, dt_events, range_mm=None, stride_ranges=0, err_est=None, stride_err=0,
                       accel=None, stride_accel=0, cov=None, trajectory=None, status_events=None, status=None,
                       stream=None):
        """kfpos_run_events_dev: kinds (EVENT_IMU / EVENT_TOA) and dt_events are host arrays of one entry per event;
        the j-th TOA event reads range_mm / err_est + j * stride, the i-th IMU event accel + i * stride_accel; cov is
        one [9][T] array for the call. Bit for bit the same events as single step_imu_dev / step_toa_dev calls."""
        k = np.ascontiguousarray(kinds, dtype=np.uint8)
        d = np.ascontiguousarray(dt_events, dtype=np.float64)
        assert k.ndim == 1 and d.shape == k.shape
        self._chk(self.lib.kfpos_run_events_dev(self._h, k.size, k.ctypes.data, d.ctypes.data, _ptr(range_mm),
                                                stride_ranges, _ptr(err_est), stride_err, _ptr(accel), stride_accel,
                                                _ptr(cov), _ptr(trajectory), _ptr(status_events), _ptr(status),
                                                _ptr(stream)))

    def run_events_each_dev(self, kinds, dt_events_dev, range_mm=None, stride_ranges=0, err_est=None, stride_err=0,
                            accel=None, stride_accel=0, cov=None, trajectory=None, status_events=None, status=None,
                            stream=None):
        """kfpos_run_events_each_dev: run_events_dev with a timeline per tag. kinds is a host array of one entry per
        slot; dt_events_dev is a DEVICE array [n_events][T] of float64 (a torch tensor or a pointer): each tag's timeLag
        in each slot, < 0 where the tag sits the slot out. The j-th TOA slot reads range_mm / err_est + j * stride, the
        i-th IMU slot accel + i * stride_accel; cov is one [9][T] array for the call. Bit for bit the same slots as
        single step_imu_dev / step_toa_dev calls with dt_dev = dt_events_dev[e]."""
        k = np.ascontiguousarray(kinds, dtype=np.uint8)
        assert k.ndim == 1
        if hasattr(dt_events_dev, "data_ptr"):
            assert tuple(dt_events_dev.shape) == (k.size, self.T) and dt_events_dev.is_contiguous()
            assert dt_events_dev.element_size() == 8
        self._chk(self.lib.kfpos_run_events_each_dev(self._h, k.size, k.ctypes.data, _ptr(dt_events_dev),
                                                     _ptr(range_mm), stride_ranges, _ptr(err_est), stride_err,
                                                     _ptr(accel), stride_accel, _ptr(cov), _ptr(trajectory),
                                                     _ptr(status_events), _ptr(status), _ptr(stream)))

    def run_planar_events_dev(self, kinds, dt_events, range_mm=None, stride_ranges=0, err_est=None, stride_err=0,
                              px4flow=None, stride_px4flow=0, imu=None, stride_imu=0, mag=None, stride_mag=0,
                              compass=None, stride_compass=0, trajectory=None, status_events=None, status=None,
                              stream=None):
        """kfpos_run_planar_events_dev (MODEL_PLANAR): kinds (PLANAR_EVENT_TOA, SENSOR_PX4FLOW .. SENSOR_COMPASS) and
        dt_events are host arrays of one entry per event; the n-th event of a kind reads that kind's array + n * stride
        elements ([A][T] ranges and errorEstimations, [5][T], [24][T], [3][T], [1][T] samples). Bit for bit the same
        events as single step_toa_dev / step_sensor_dev calls."""
        k = np.ascontiguousarray(kinds, dtype=np.uint8)
        d = np.ascontiguousarray(dt_events, dtype=np.float64)
        assert k.ndim == 1 and d.shape == k.shape
        inp = PlanarInputs(_ptr(range_mm), stride_ranges, _ptr(err_est), stride_err, _ptr(px4flow), stride_px4flow,
                           _ptr(imu), stride_imu, _ptr(mag), stride_mag, _ptr(compass), stride_compass)
        self._chk(self.lib.kfpos_run_planar_events_dev(self._h, k.size, k.ctypes.data, d.ctypes.data, C.byref(inp),
                                                       _ptr(trajectory), _ptr(status_events), _ptr(status),
                                                       _ptr(stream)))

    def run_planar_events_each_dev(self, kinds, dt_events_dev, range_mm=None, stride_ranges=0, err_est=None,
                                   stride_err=0, px4flow=None, stride_px4flow=0, imu=None, stride_imu=0, mag=None,
                                   stride_mag=0, compass=None, stride_compass=0, trajectory=None, status_events=None,
                                   status=None, stream=None):
        """kfpos_run_planar_events_each_dev (MODEL_PLANAR): run_planar_events_dev with a timeline per tag. kinds is a
        host array of one entry per slot; dt_events_dev is a DEVICE array [n_events][T] of float64 (a torch tensor or a
        pointer): each tag's timeLag in each slot, < 0 where the tag sits the slot out. The n-th slot of a kind reads
        that kind's array + n * stride elements. Bit for bit the same slots as single step_toa_dev / step_sensor_dev
        calls with dt_dev = dt_events_dev[e]."""
        k = np.ascontiguousarray(kinds, dtype=np.uint8)
        assert k.ndim == 1
        if hasattr(dt_events_dev, "data_ptr"):
            assert tuple(dt_events_dev.shape) == (k.size, self.T) and dt_events_dev.is_contiguous()
            assert dt_events_dev.element_size() == 8
        inp = PlanarInputs(_ptr(range_mm), stride_ranges, _ptr(err_est), stride_err, _ptr(px4flow), stride_px4flow,
                           _ptr(imu), stride_imu, _ptr(mag), stride_mag, _ptr(compass), stride_compass)
        self._chk(self.lib.kfpos_run_planar_events_each_dev(self._h, k.size, k.ctypes.data, _ptr(dt_events_dev),
                                                            C.byref(inp), _ptr(trajectory), _ptr(status_events),
                                                            _ptr(status), _ptr(stream)))

    def run_trace_each_dev(self, dt_steps_dev, range_mm, stride_ranges, err_est, stride_err=0, trajectory=None,
                           status_steps=None, status=None, stream=None):
        """kfpos_run_trace_each_dev (MODEL_TOA): ranging slots with a timeline per tag. dt_steps_dev is a DEVICE array
        [n_steps][T] of float64 (a torch tensor; its first dimension is the number of slots): each tag's timeLag in each
        slot, < 0 where the tag sits the slot out. Slot s reads range_mm / err_est + s * stride. Bit for bit the same
        slots as single step_toa_dev calls with dt_dev = dt_steps_dev[s]."""
        assert dt_steps_dev.dim() == 2 and dt_steps_dev.shape[1] == self.T and dt_steps_dev.is_contiguous()
        assert dt_steps_dev.element_size() == 8
        self._chk(self.lib.kfpos_run_trace_each_dev(self._h, int(dt_steps_dev.shape[0]), _ptr(dt_steps_dev),
                                                    _ptr(range_mm), stride_ranges, _ptr(err_est), stride_err,
                                                    _ptr(trajectory), _ptr(status_steps), _ptr(status), _ptr(stream)))

    def timing_begin(self, stream=None):
        self._chk(self.lib.kfpos_timing_begin(self._h, _ptr(stream)))

    def timing_end(self, stream=None) -> float:
        ms = C.c_float()
        self._chk(self.lib.kfpos_timing_end(self._h, _ptr(stream), C.byref(ms)))
        return float(ms.value)


# ---- multi-GPU: the RCCL pose all-gather behind the C ABI (include/kfpos.h: kfpos_comm_*) ----
def _chk_lib(lib, rc):
    if rc != 0:
        msg = lib.kfpos_strerror(rc).decode()
        detail = lib.kfpos_last_error().decode()
        raise KfposError(msg + (": " + detail if detail else ""))


def shard_range(total_tags: int, world: int, rank: int):
    """kfpos_shard_range: contiguous [lo, hi) of `rank`; host arithmetic only."""
    lo, hi = C.c_int64(), C.c_int64()
    lib = load()
    _chk_lib(lib, lib.kfpos_shard_range(total_tags, world, rank, C.byref(lo), C.byref(hi)))
    return lo.value, hi.value


def comm_unique_id() -> bytes:
    """ncclGetUniqueId through the library: rank 0 makes it, every rank gets the same 128 bytes."""
    lib = load()
    buf = C.create_string_buffer(COMM_ID_BYTES)
    _chk_lib(lib, lib.kfpos_comm_unique_id(buf))
    return buf.raw


def assemble_poses_dev(world, rows, total_tags, staged, out, device=0, stream=None):
    """[world][rows][t_pad] gathered by any collective -> [rows][total] in global tag order (device tensors)."""
    lib = load()
    _chk_lib(lib, lib.kfpos_assemble_poses_dev(world, rows, total_tags, _ptr(staged), _ptr(out), device, _ptr(stream)))


class KfposComm:
    """One rank's end of the pose all-gather (kfpos_comm): RCCL communicator + side stream + two buffer sets."""

    def __init__(self, world, rank, unique_id: bytes, device=0, _handle=None):
        self.lib = load()
        self._c = None
        if _handle is not None:
            self._c = _handle
        else:
            assert len(unique_id) == COMM_ID_BYTES
            c = C.c_void_p()
            _chk_lib(self.lib, self.lib.kfpos_comm_create(world, rank, unique_id, device, C.byref(c)))
            self._c = c
        self.world, self.rank, self.device = self.lib.kfpos_comm_world(self._c), self.lib.kfpos_comm_rank(self._c), device
        self.lo = self.hi = None

    @classmethod
    def create_all(cls, devices):
        """One process, several GPUs (ncclCommInitAll): a list of communicators, one per device."""
        lib = load()
        n = len(devices)
        devs = (C.c_int32 * n)(*devices)
        out = (C.c_void_p * n)()
        _chk_lib(lib, lib.kfpos_comm_create_all(n, devs, out))
        return [cls(n, i, b"", devices[i], _handle=C.c_void_p(out[i])) for i in range(n)]

    def set_total(self, total_tags: int):
        lo, hi = C.c_int64(), C.c_int64()
        _chk_lib(self.lib, self.lib.kfpos_comm_set_total(self._c, total_tags, C.byref(lo), C.byref(hi)))
        self.lo, self.hi, self.total = lo.value, hi.value, total_tags
        return self.lo, self.hi

    def allgather(self, pos_all, pos_local=None, rows=3, bank=None, stream=None):
        """pos_local [rows][t_local] (or the bank's current positions) -> pos_all [rows][total]; asynchronous."""
        _chk_lib(self.lib, self.lib.kfpos_allgather_poses(bank._h if bank is not None else None, self._c,
                                                          _ptr(pos_local), rows, _ptr(pos_all), _ptr(stream)))

    def set_algorithm(self, algorithm: int):
        """GATHER_COLLECTIVE (ncclAllGather) or GATHER_DIRECT (grouped ncclSend / ncclRecv to every peer)."""
        _chk_lib(self.lib, self.lib.kfpos_comm_set_algorithm(self._c, algorithm))

    @property
    def algorithm(self) -> int:
        return self.lib.kfpos_comm_algorithm(self._c)

    def wait(self, stream=None):
        _chk_lib(self.lib, self.lib.kfpos_comm_wait(self._c, _ptr(stream)))

    def sync(self):
        _chk_lib(self.lib, self.lib.kfpos_comm_sync(self._c))

    def close(self):
        if self._c:
            self.lib.kfpos_comm_destroy(self._c)
            self._c = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def allgather_poses_multi(comms, pos_all, pos_local=None, rows=3, banks=None, streams=None):
    """kfpos_allgather_poses_multi: the gathers of all communicators of one process in one RCCL group."""
    lib = load()
    n = len(comms)
    arr = lambda xs: (C.c_void_p * n)(*[_ptr(x) for x in xs]) if xs is not None else None  # noqa: E731
    _chk_lib(lib, lib.kfpos_allgather_poses_multi(
        n, arr([b._h.value for b in banks]) if banks is not None else None, arr([c._c.value for c in comms]),
        arr(pos_local), rows, arr(pos_all), arr(streams)))
