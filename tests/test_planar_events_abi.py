"""kfpos_run_planar_events_dev exists in the header, the library and the binding, and refuses a NULL handle before it
touches a device (no GPU needed)."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KFPOS_ERR_ARG = 1


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(capi.LIB_PATH)


def test_header_declares_the_struct_the_constant_and_the_call():
    text = open(os.path.join(ROOT, "include", "kfpos.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert re.search(r"^#define\s+KFPOS_PLANAR_EVENT_TOA\s+0\s*$", code, flags=re.M)
    ws = r"\s*"
    fields = [r"const\s+int32_t\s*\*\s*range_mm", r"int64_t\s+stride_ranges", r"const\s+void\s*\*\s*err_est",
              r"int64_t\s+stride_err", r"const\s+double\s*\*\s*px4flow", r"int64_t\s+stride_px4flow",
              r"const\s+double\s*\*\s*imu", r"int64_t\s+stride_imu", r"const\s+double\s*\*\s*mag",
              r"int64_t\s+stride_mag", r"const\s+double\s*\*\s*compass", r"int64_t\s+stride_compass"]
    assert re.search(r"typedef\s+struct\s+kfpos_planar_inputs\s*\{" + ws + (ws + ";" + ws).join(fields) + ws + ";" + ws +
                     r"\}\s*kfpos_planar_inputs\s*;", code)
    args = [r"kfpos_handle\s*\*\s*h", r"int32_t\s+n_events", r"const\s+uint8_t\s*\*\s*kinds",
            r"const\s+double\s*\*\s*dt_events", r"const\s+kfpos_planar_inputs\s*\*\s*in", r"double\s*\*\s*trajectory",
            r"uint32_t\s*\*\s*status_events", r"uint32_t\s*\*\s*status", r"void\s*\*\s*stream"]
    assert re.search(r"\bint\s+kfpos_run_planar_events_dev\s*\(" + ws + (ws + "," + ws).join(args) + ws + r"\)\s*;", code)
    assert "#define KFPOS_VERSION 102" in text          # found by symbol, not by version number
    assert "kfpos_run_planar_events_dev" in capi.EXPORTS
    assert capi.PLANAR_EVENT_TOA == 0
    assert (capi.SENSOR_PX4FLOW, capi.SENSOR_IMU, capi.SENSOR_MAG, capi.SENSOR_COMPASS) == (1, 2, 3, 4)
    assert ctypes.sizeof(capi.PlanarInputs) == 12 * 8   # six pointers, six 64-bit strides


def test_library_exports_it_and_a_null_handle_is_an_argument_error():
    lib = _lib()
    assert hasattr(lib, "kfpos_run_planar_events_dev")
    assert lib.kfpos_version() == 102
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.kfpos_run_planar_events_dev.argtypes = [vp, i32, vp, vp, ctypes.POINTER(capi.PlanarInputs), vp, vp, vp, vp]
    kinds = (ctypes.c_uint8 * 2)(2, 0)
    dts = (ctypes.c_double * 2)(0.01, 0.02)
    inp = capi.PlanarInputs()
    call = lib.kfpos_run_planar_events_dev
    assert call(None, 2, kinds, dts, ctypes.byref(inp), None, None, None, None) == KFPOS_ERR_ARG
    assert call(None, 0, None, None, None, None, None, None, None) == KFPOS_ERR_ARG


def test_binding_has_the_method():
    assert callable(getattr(capi.KfposBank, "run_planar_events_dev"))
    capi.load()
    assert len(capi._lib.kfpos_run_planar_events_dev.argtypes) == 9
