"""The D16 wire format of include/kfpos_d16.h restated in numpy (whole matrices at a time): what the tests encode with when
they write a slot's codes themselves, and what tests/test_d16_codec.py compares with the header's own C text.

Matrices are (A, T) = [max_anchors][n_tags], flat index e = a * T + t; `skip` is a bool (T,) of the tags whose dt < 0."""
import numpy as np

ABSENT, ESCAPE, DELTA_MIN, DELTA_MAX = -32768, -32767, -32766, 32767


def encode_into(code, base, v, skip=None):
    """kfpos_d16_put over every element of the tags that are not skipped, in ascending order: writes `code` (int16 view)
    and moves `base` (int32 view) in place, the skipped tags' columns of both stay as they are. Returns the escape list,
    int32 (k, 2): flat index, value."""
    v = np.asarray(v, dtype=np.int32)
    live = np.ones(v.shape, dtype=bool) if skip is None else np.broadcast_to(~np.asarray(skip, dtype=bool), v.shape)
    present = live & (v > 0)
    d = v.astype(np.int64) - base.astype(np.int64)
    delta = present & (d >= DELTA_MIN) & (d <= DELTA_MAX)
    esc = present & ~delta
    code[live & (v <= 0)] = ABSENT
    code[delta] = d[delta].astype(np.int16)
    code[esc] = ESCAPE
    base[present] = v[present]
    idx = np.flatnonzero(esc)
    return np.stack([idx, v.reshape(-1)[idx]], axis=1).astype(np.int32).reshape(-1, 2)


def fill(views, v, skip=None):
    """encode_into for the views of KfposBank.slot_delta: codes, escape list and n_esc of the open slot"""
    esc = encode_into(views["code"], views["base"], v, skip)
    views["esc"][:len(esc)] = esc
    views["n_esc"][0] = len(esc)
    return len(esc)


def decode(code, esc, base, out, skip=None):
    """kfpos_d16_decode_ref: moves `base`, writes `out` (an ESCAPE code without an entry keeps what out held)"""
    live = np.ones(code.shape, dtype=bool) if skip is None else np.broadcast_to(~np.asarray(skip, dtype=bool), code.shape)
    c = code.astype(np.int64)
    out[~live | (c == ABSENT)] = 0
    delta = live & (c != ABSENT) & (c != ESCAPE)
    s = ((base.astype(np.int64) + c) & 0xffffffff).astype(np.uint32).view(np.int32)   # the sum wraps as uint32 does
    out[delta] = s[delta]
    base[delta] = s[delta]
    esc = np.asarray(esc, dtype=np.int32).reshape(-1, 2)
    T = code.shape[1]
    keep = np.ones(len(esc), dtype=bool) if skip is None else ~np.asarray(skip, dtype=bool)[esc[:, 0] % T]
    out.reshape(-1)[esc[keep, 0]] = esc[keep, 1]
    base.reshape(-1)[esc[keep, 0]] = esc[keep, 1]
