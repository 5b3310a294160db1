"""KFPOS_SLOT_RANGES_D16 at the ABI (no compute calls here): the library exports kfpos_slot_delta and
kfpos_slot_encode_ranges, the flag and the code constants agree between include/kfpos.h, include/kfpos_d16.h and
roskfpos_amd/capi.py, the struct the binding declares is the header's, and kfpos_d16.h includes <stdint.h> and nothing
else."""
import ctypes
import os
import re

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("kfpos_slot_delta", "kfpos_slot_encode_ranges")


def _text(name):
    return open(os.path.join(ROOT, "include", name)).read()


def _define(text, name):
    m = re.search(r"^#define\s+" + name + r"\s+\(?(-?(?:0x[0-9a-fA-F]+|\d+))\)?", text, flags=re.M)
    assert m, name
    return int(m.group(1), 0)


def test_library_exports_the_entry_points():
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    lib = ctypes.CDLL(capi.LIB_PATH)
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in capi.EXPORTS
    assert lib.kfpos_version() == 102  # unchanged: the feature is detected by symbol


def test_constants_agree():
    h, d = _text("kfpos.h"), _text("kfpos_d16.h")
    assert _define(h, "KFPOS_SLOT_RANGES_D16") == capi.SLOT_RANGES_D16 == 0x2000
    assert _define(d, "KFPOS_D16_ABSENT") == capi.D16_ABSENT == -32768
    assert _define(d, "KFPOS_D16_ESCAPE") == capi.D16_ESCAPE == -32767
    assert _define(d, "KFPOS_D16_DELTA_MIN") == capi.D16_DELTA_MIN == -32766
    assert _define(d, "KFPOS_D16_DELTA_MAX") == capi.D16_DELTA_MAX == 32767
    # no other slot flag shares the bit
    others = [_define(h, "KFPOS_SLOT_" + n) for n in ("DT_PER_TAG", "REUSE_ERR", "REUSE_COV", "NO_POSE", "POSE_COV")]
    assert all(o & capi.SLOT_RANGES_D16 == 0 for o in others)
    import d16
    assert (d16.ABSENT, d16.ESCAPE, d16.DELTA_MIN, d16.DELTA_MAX) == (-32768, -32767, -32766, 32767)


def test_binding_struct_is_the_headers():
    body = re.search(r"typedef struct kfpos_delta_slot \{(.*?)\} kfpos_delta_slot;", _text("kfpos_d16.h"), flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for decl in body.split(";"):
        if not decl.strip():
            continue
        ctype, names = decl.strip().rsplit(None, 1) if "," not in decl else (decl.split()[0], decl.split(None, 1)[1])
        for nm in names.split(","):
            fields.append((nm.strip().lstrip("*"), "*" in ctype or "*" in nm))
    got = [(n, t is ctypes.c_void_p) for n, t in capi._DeltaSlot._fields_]
    assert got == fields
    assert [n for n, _ in fields] == ["code", "esc", "n_esc", "esc_capacity", "base", "n_tags", "max_anchors"]


def test_d16_header_includes_stdint_only():
    assert re.findall(r"^\s*#\s*include\s*(\S+)", _text("kfpos_d16.h"), flags=re.M) == ["<stdint.h>"]
    assert '#include "kfpos_d16.h"' in _text("kfpos.h")
