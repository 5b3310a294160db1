"""kfpos_run_trace_each_dev exists in the header, the library and the binding, and refuses a NULL handle before it
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


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "kfpos.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ws = r"\s*"
    args = [r"kfpos_handle\s*\*\s*h", r"int32_t\s+n_steps", r"const\s+double\s*\*\s*dt_steps_dev",
            r"const\s+int32_t\s*\*\s*range_mm", r"int64_t\s+stride_ranges", r"const\s+void\s*\*\s*err_est",
            r"int64_t\s+stride_err", r"double\s*\*\s*trajectory", r"uint32_t\s*\*\s*status_steps",
            r"uint32_t\s*\*\s*status", r"void\s*\*\s*stream"]
    assert re.search(r"\bint\s+kfpos_run_trace_each_dev\s*\(" + ws + (ws + "," + ws).join(args) + ws + r"\)\s*;", code)
    assert "#define KFPOS_VERSION 102" in text          # found by symbol, not by version number
    assert "kfpos_run_trace_each_dev" in capi.EXPORTS
    # the header says what a reader needs to merge timelines: the predicate, and what an absent tag gets
    doc = text[text.index("kfpos_run_trace_dev for a 6-state bank"):text.index("int kfpos_run_trace_each_dev")]
    assert "< 0.0" in doc and "KFPOS_ST_SKIPPED" in doc and "NaN" in doc
    # ... where callers of the other filters go, and which handles are not fused
    assert "kfpos_run_events_each_dev" in doc and "kfpos_run_planar_events_each_dev" in doc and "KFPOS_NO_COOP" in doc


def test_library_exports_it_and_a_null_handle_is_an_argument_error():
    lib = _lib()
    assert hasattr(lib, "kfpos_run_trace_each_dev")
    assert lib.kfpos_version() == 102
    vp, i32, i64 = ctypes.c_void_p, ctypes.c_int32, ctypes.c_int64
    lib.kfpos_run_trace_each_dev.argtypes = [vp, i32, vp, vp, i64, vp, i64, vp, vp, vp, vp]
    buf = (ctypes.c_double * 64)()
    call = lib.kfpos_run_trace_each_dev
    assert call(None, 2, buf, buf, 0, buf, 0, None, None, None, None) == KFPOS_ERR_ARG
    assert call(None, 0, None, None, 0, None, 0, None, None, None, None) == KFPOS_ERR_ARG


def test_binding_has_the_method():
    assert callable(getattr(capi.KfposBank, "run_trace_each_dev"))
    capi.load()
    fn = capi._lib.kfpos_run_trace_each_dev
    assert fn.argtypes is not None and len(fn.argtypes) == 11
