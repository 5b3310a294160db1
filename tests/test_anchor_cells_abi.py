"""kfpos_set_anchor_cells / kfpos_anchor_cells (include/kfpos.h): declared, documented, exported and bound; a NULL handle is
an argument error before anything touches a GPU. What the calls compute: tests/test_anchor_cells_gpu.py."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    return open(os.path.join(ROOT, "include", "kfpos.h")).read()


def _lib():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return ctypes.CDLL(capi.LIB_PATH)


def test_header_declares_the_calls_and_the_block_size():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"#define\s+KFPOS_CELL_TAGS\s+64\b", text)
    assert re.search(r"int\s+kfpos_set_anchor_cells\(kfpos_handle \*h, int32_t n_cells, int32_t n_anchors,\s*"
                     r"const double \*xyz,\s*const int32_t \*cell_of_block\);", text)
    assert re.search(r"int\s+kfpos_anchor_cells\(const kfpos_handle \*h\);", text)
    assert re.search(r"#define\s+KFPOS_VERSION\s+102\b", text), "the feature is detected by symbol, not by version"


def test_header_says_what_refuses_cells_and_why():
    doc = " ".join(_header().split()).replace(" * ", " ")
    for name in ("kfpos_step_*_rows", "kfpos_slot_submit_rows", "kfpos_run_events_dev", "kfpos_run_events_each_dev",
                 "kfpos_run_trace_each_dev"):
        assert name in doc, name
    assert "mixes rows of different cells in one wavefront" in doc
    assert "KFPOS_ERR_MODEL on KFPOS_MODEL_ML and KFPOS_MODEL_PLANAR" in doc
    assert "8-lanes-per-tag kernel" in doc and "KFPOS_NO_COOP=1" in doc
    assert "kfpos_run_trace_dev, which stays FUSED" in doc


def test_library_exports_the_calls_and_refuses_a_null_handle():
    lib = _lib()
    assert hasattr(lib, "kfpos_set_anchor_cells") and hasattr(lib, "kfpos_anchor_cells")
    lib.kfpos_set_anchor_cells.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.c_int32, ctypes.c_void_p, ctypes.c_void_p]
    lib.kfpos_anchor_cells.argtypes = [ctypes.c_void_p]
    xyz = (ctypes.c_double * 24)()
    cells = (ctypes.c_int32 * 4)()
    assert lib.kfpos_set_anchor_cells(None, 1, 8, xyz, cells) == 1   # KFPOS_ERR_ARG
    assert lib.kfpos_anchor_cells(None) == 0


def test_binding_has_the_methods():
    assert "kfpos_set_anchor_cells" in capi.EXPORTS and "kfpos_anchor_cells" in capi.EXPORTS
    assert callable(capi.KfposBank.set_anchor_cells) and callable(capi.KfposBank.set_anchors)
    assert isinstance(capi.KfposBank.anchor_cells, property)
    assert capi.CELL_TAGS == 64
