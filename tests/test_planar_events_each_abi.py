"""kfpos_run_planar_events_each_dev exists in the header, the library and the binding, and refuses a NULL handle before
it touches a device (no GPU needed)."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KFPOS_ERR_ARG = 1
NAME = "kfpos_run_planar_events_each_dev"


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(capi.LIB_PATH)


def test_header_declares_the_call():
    text = open(os.path.join(ROOT, "include", "kfpos.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    ws = r"\s*"
    args = [r"kfpos_handle\s*\*\s*h", r"int32_t\s+n_events", r"const\s+uint8_t\s*\*\s*kinds",
            r"const\s+double\s*\*\s*dt_events_dev", r"const\s+kfpos_planar_inputs\s*\*\s*in",
            r"double\s*\*\s*trajectory", r"uint32_t\s*\*\s*status_events", r"uint32_t\s*\*\s*status",
            r"void\s*\*\s*stream"]
    assert re.search(r"\bint\s+" + NAME + r"\s*\(" + ws + (ws + "," + ws).join(args) + ws + r"\)\s*;", code)
    assert "#define KFPOS_VERSION 102" in text          # found by symbol, not by version number
    assert NAME in capi.EXPORTS
    # the header says what a reader needs to merge timelines: the predicate, what an absent tag gets, the latch rule
    # and the PX4Flow drop rule
    doc = text[text.index("kfpos_run_planar_events_dev for a bank whose tags"):text.index("int " + NAME)]
    assert "< 0.0" in doc and "KFPOS_ST_SKIPPED" in doc and "NaN" in doc
    assert "latch" in doc and "quality 0" in doc


def test_library_exports_it_and_a_null_handle_is_an_argument_error():
    lib = _lib()
    assert hasattr(lib, NAME)
    assert lib.kfpos_version() == 102
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    call = getattr(lib, NAME)
    call.argtypes = [vp, i32, vp, vp, ctypes.POINTER(capi.PlanarInputs), vp, vp, vp, vp]
    kinds = (ctypes.c_uint8 * 2)(2, 0)
    dts = (ctypes.c_double * 2)(0.01, 0.02)          # never read: the handle is looked at first
    inp = capi.PlanarInputs()
    assert call(None, 2, kinds, dts, ctypes.byref(inp), None, None, None, None) == KFPOS_ERR_ARG
    assert call(None, 0, None, None, None, None, None, None, None) == KFPOS_ERR_ARG


def test_binding_has_the_method():
    assert callable(getattr(capi.KfposBank, "run_planar_events_each_dev"))
    capi.load()
    fn = getattr(capi._lib, NAME)
    assert fn.argtypes is not None and len(fn.argtypes) == 9
