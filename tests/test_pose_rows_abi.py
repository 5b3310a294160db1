"""Pose for a row list: kfpos_get_pose_rows / kfpos_get_predicted_rows / kfpos_slot_pose_rows and KFPOS_SLOT_POSE_COV
exist in the header, the library and the binding, and refuse a NULL handle before they touch a device (no GPU needed)."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kfpos_get_pose_rows", "kfpos_get_predicted_rows", "kfpos_slot_pose_rows")
KFPOS_ERR_ARG = 1


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(capi.LIB_PATH)


def test_header_declares_the_entry_points_and_the_flag():
    text = open(os.path.join(ROOT, "include", "kfpos.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    head = r"\bint\s+%s\s*\(\s*kfpos_handle\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*rows\s*,\s*int32_t\s+n\s*,\s*" \
           r"const\s+double\s*\*\s*dt_ahead\s*,\s*int32_t\s+dt_len\s*,\s*"
    assert re.search(head % "kfpos_get_pose_rows" + r"double\s*\*\s*pos\s*,\s*double\s*\*\s*cov3x3\s*,\s*double\s*\*\s*vel\s*,"
                     r"\s*uint32_t\s*\*\s*status\s*\)", code)
    assert re.search(head % "kfpos_get_predicted_rows" + r"double\s*\*\s*x\s*,\s*double\s*\*\s*P\s*,\s*uint32_t\s*\*\s*status\s*\)",
                     code)
    assert re.search(r"\bint\s+kfpos_slot_pose_rows\s*\(\s*kfpos_handle\s*\*\s*h\s*,\s*int32_t\s+slot\s*,\s*double\s*\*\*\s*cov3x3\s*,"
                     r"\s*double\s*\*\*\s*vel\s*\)", code)
    assert re.search(r"#define\s+KFPOS_SLOT_POSE_COV\s+0x1000\b", code)
    assert "#define KFPOS_VERSION 102" in text          # found by symbol, not by version number
    assert not re.search(r"\bkfpos_get_pose_rows_dev\b", code)  # a device-resident list could not be validated
    for name in NAMES:
        assert name in capi.EXPORTS
    assert capi.SLOT_POSE_COV == 0x1000
    # the flag is a bit of its own
    others = capi.SLOT_DT_PER_TAG | capi.SLOT_REUSE_ERR | capi.SLOT_REUSE_COV | capi.SLOT_NO_POSE | 0xff
    assert capi.SLOT_POSE_COV & others == 0


def test_library_exports_them_and_a_null_handle_is_an_argument_error():
    lib = _lib()
    for name in NAMES:
        assert hasattr(lib, name), name
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.kfpos_get_pose_rows.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp, vp]
    lib.kfpos_get_predicted_rows.argtypes = [vp, vp, i32, vp, i32, vp, vp, vp]
    lib.kfpos_slot_pose_rows.argtypes = [vp, i32, ctypes.POINTER(vp), ctypes.POINTER(vp)]
    rows = (ctypes.c_int32 * 2)(0, 1)
    dt = (ctypes.c_double * 1)(0.1)
    buf = (ctypes.c_double * 256)()
    assert lib.kfpos_get_pose_rows(None, rows, 2, dt, 1, buf, buf, buf, None) == KFPOS_ERR_ARG
    assert lib.kfpos_get_pose_rows(None, None, 0, dt, 1, None, None, None, None) == KFPOS_ERR_ARG
    assert lib.kfpos_get_predicted_rows(None, rows, 2, dt, 1, buf, buf, None) == KFPOS_ERR_ARG
    cov, vel = vp(), vp()
    assert lib.kfpos_slot_pose_rows(None, 0, ctypes.byref(cov), ctypes.byref(vel)) == KFPOS_ERR_ARG
    assert cov.value is None and vel.value is None
    assert all(v == 0.0 for v in buf)


def test_binding_has_the_methods():
    for name in ("get_pose_rows", "get_predicted_rows", "slot_pose_rows"):
        assert callable(getattr(capi.KfposBank, name))
