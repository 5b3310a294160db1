"""The per-tag lifecycle entry points exist in the header, the library and the binding, and refuse a NULL handle before
they touch a device (no GPU needed)."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kfpos_reset_tags", "kfpos_get_tags", "kfpos_set_tags")
KFPOS_ERR_ARG = 1


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(capi.LIB_PATH)


def test_header_declares_the_three_entry_points():
    text = open(os.path.join(ROOT, "include", "kfpos.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NAMES:
        assert re.search(r"\bint\s+%s\s*\(\s*kfpos_handle\s*\*\s*h\s*,\s*const\s+int32_t\s*\*\s*rows\s*,\s*int32_t\s+n\b" % name,
                         code), name
        assert name in capi.EXPORTS
    assert "#define KFPOS_VERSION 102" in text          # found by symbol, not by version number
    assert re.search(r"by symbol", text)


def test_library_exports_them_and_a_null_handle_is_an_argument_error():
    lib = _lib()
    rows = (ctypes.c_int32 * 2)(0, 1)
    for name in NAMES:
        assert hasattr(lib, name), name
    vp, i32 = ctypes.c_void_p, ctypes.c_int32
    lib.kfpos_reset_tags.argtypes = [vp, vp, i32, vp]
    lib.kfpos_get_tags.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    lib.kfpos_set_tags.argtypes = [vp, vp, i32, vp, vp, vp, vp, vp]
    assert lib.kfpos_reset_tags(None, rows, 2, None) == KFPOS_ERR_ARG
    assert lib.kfpos_get_tags(None, rows, 2, None, None, None, None, None) == KFPOS_ERR_ARG
    assert lib.kfpos_set_tags(None, rows, 2, None, None, None, None, None) == KFPOS_ERR_ARG
    assert lib.kfpos_reset_tags(None, None, 0, None) == KFPOS_ERR_ARG


def test_binding_has_the_methods():
    for name in ("reset_tags", "get_tags", "set_tags"):
        assert callable(getattr(capi.KfposBank, name))
