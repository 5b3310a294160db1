"""The row-list step entry points exist in the header, the library and the binding, and refuse a NULL handle before
they touch a device (no GPU needed)."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEPS = ("kfpos_step_toa_rows", "kfpos_step_imu_rows", "kfpos_step_toa_imu_rows", "kfpos_step_sensor_rows")
SLOTS = ("kfpos_slot_acquire_rows", "kfpos_slot_submit_rows")
KFPOS_ERR_ARG = 1


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(capi.LIB_PATH)


def test_header_declares_the_six_entry_points():
    text = open(os.path.join(ROOT, "include", "kfpos.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in STEPS:
        assert re.search(r"\bint\s+%s\s*\(\s*kfpos_handle\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*rows\s*,\s*int32_t\s+n\b" % name,
                         code), name
    assert re.search(r"\bint\s+kfpos_slot_acquire_rows\s*\(\s*kfpos_handle\s*\*\s*h\s*,\s*int32_t\s+slot\s*,\s*kfpos_rows_slot\s*\*", code)
    assert re.search(r"\bint\s+kfpos_slot_submit_rows\s*\(\s*kfpos_handle\s*\*\s*h\s*,\s*int32_t\s+slot\s*,\s*int32_t\s+flags\s*,"
                     r"\s*int32_t\s+n\s*,\s*double\s+dt_shared\s*\)", code)
    assert re.search(r"typedef\s+struct\s+kfpos_rows_slot\s*\{[^}]*\brows\b[^}]*\bcapacity\b[^}]*\}\s*kfpos_rows_slot\s*;", code)
    for name in STEPS + SLOTS:
        assert name in capi.EXPORTS
    assert "#define KFPOS_VERSION 102" in text          # found by symbol, not by version number
    assert not re.search(r"\bkfpos_step_\w+_rows_dev\b", code)  # a device-resident list could not be validated


def test_library_exports_them_and_a_null_handle_is_an_argument_error():
    lib = _lib()
    for name in STEPS + SLOTS:
        assert hasattr(lib, name), name
    vp, i32, f64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_double
    lib.kfpos_step_toa_rows.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp]
    lib.kfpos_step_imu_rows.argtypes = [vp, vp, i32, vp, vp, vp, i32, vp]
    lib.kfpos_step_toa_imu_rows.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp, i32, vp]
    lib.kfpos_step_sensor_rows.argtypes = [vp, vp, i32, i32, vp, vp, i32, vp]
    lib.kfpos_slot_acquire_rows.argtypes = [vp, i32, vp]
    lib.kfpos_slot_submit_rows.argtypes = [vp, i32, i32, i32, f64]
    rows = (ctypes.c_int32 * 2)(0, 1)
    buf = (ctypes.c_double * 64)()
    dt = (ctypes.c_double * 1)(0.1)
    assert lib.kfpos_step_toa_rows(None, rows, 2, buf, buf, dt, 1, None) == KFPOS_ERR_ARG
    assert lib.kfpos_step_imu_rows(None, rows, 2, buf, buf, dt, 1, None) == KFPOS_ERR_ARG
    assert lib.kfpos_step_toa_imu_rows(None, rows, 2, buf, buf, buf, buf, dt, 1, None) == KFPOS_ERR_ARG
    assert lib.kfpos_step_sensor_rows(None, rows, 2, 4, buf, dt, 1, None) == KFPOS_ERR_ARG
    assert lib.kfpos_step_toa_rows(None, None, 0, None, None, None, 1, None) == KFPOS_ERR_ARG
    out = capi._RowsSlot()
    assert lib.kfpos_slot_acquire_rows(None, 0, ctypes.byref(out)) == KFPOS_ERR_ARG
    assert lib.kfpos_slot_submit_rows(None, 0, 0, 2, 0.1) == KFPOS_ERR_ARG


def test_binding_has_the_methods():
    for name in ("step_toa_rows", "step_imu_rows", "step_toa_imu_rows", "step_sensor_rows",
                 "slot_acquire_rows", "slot_submit_rows"):
        assert callable(getattr(capi.KfposBank, name))
    fields = [f for f, _ in capi._RowsSlot._fields_]
    assert fields == ["rows", "range_mm", "err_est", "accel", "cov", "dt", "status", "pos", "capacity"]
