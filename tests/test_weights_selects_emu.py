"""The working weights and the zero-errorEstimation test as selects (set_weights_ml, ml_covariance_throws,
set_weights_iekf in kfpos_core_ml.h: every reciprocal and every predicate is formed, then selected; no conditional arm
computes anything), on the host build of the headers, one tag at a time with 8 anchors, through iekf9_weights (9-state
step) and through a 6-state step, against the oracle with the tolerances of tests/test_gpu_parity.py (<= 1e-9 m RMS,
<= 1e-8 m at worst over the positions of every epoch) and equal status words.

The cases (tests/weights_selects.py), each asserted to occur: an absent range whose errorEstimation slot holds NaN, 0,
inf and a negative number; a used range with errorEstimation exactly 0 (update skipped); a tag whose errorEstimations lie
on both sides of e_ML in one epoch; fewer than four ranges; e_ML NaN. (CPU only.)"""
import functools

import numpy as np
import pytest

import ml_seed_cases as mc
import weights_selects as ws
from cases import Case, rms_and_max
from impls import EmuImpl, EmuStaticImpl, OracleImpl

T = 32


@functools.lru_cache(maxsize=None)
def _oracle(model):
    return _run(model, OracleImpl)


def _run(model, impl):
    w, _, r, err = mc.inputs(T, **ws.INPUTS)
    f = impl(Case("weights_selects", model, ws.A, T=T, S=ws.S), w, w.init_positions())
    cov = w.accel_cov()
    pos, st = [], []
    for s in range(ws.S):
        if model == 1:
            st.append(np.asarray(f.fused(r[s], err, w.accel(s), cov, w.dt_of(s))).copy())
        else:
            st.append(np.asarray(f.step_toa(r[s], err, w.dt_of(s))).copy())
        pos.append(f.positions().copy())
    return np.stack(pos), np.stack(st).astype(np.uint32), f.state()


@pytest.mark.parametrize("impl", [EmuStaticImpl, EmuImpl], ids=["epoch in registers", "epoch in strided scratch"])
@pytest.mark.parametrize("model", [1, 0], ids=["9-state", "6-state"])
def test_every_side_of_the_selects_against_the_oracle(model, impl):
    pos_o, st_o, (x_o, P_o) = _oracle(model)
    pos, st, (x, P) = _run(model, impl)
    w, _, r, err = mc.inputs(T, **ws.INPUTS)
    ws.assert_inputs_reach_the_branches(model, w, r, err, st)
    rms, mx, same_nan = rms_and_max(pos, pos_o)
    print(f"model {model}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {ws.S} epochs of {T} tags")
    assert same_nan
    assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
    cmp = mc.oracle_status_comparable(model, T, exact_fit=False)
    assert np.array_equal(st[cmp], st_o[cmp]), np.argwhere(st != st_o)
    ok = np.isfinite(x_o).all(1) & np.isfinite(P_o).all((1, 2))
    assert np.array_equal(ok, np.isfinite(x).all(1) & np.isfinite(P).all((1, 2)))
    assert np.abs(P_o[ok] - P[ok]).max() <= 1e-9 * np.abs(P_o[ok]).max()


@pytest.mark.parametrize("model", [1, 0], ids=["9-state", "6-state"])
def test_a_garbage_slot_changes_no_bytes(model):
    """what an absent range's errorEstimation slot holds reaches no result: the run equals, byte for byte, the run in
    which those slots hold the ordinary value -- the tag's own bytes and every other tag's"""
    w, _, r, err = mc.inputs(T, **ws.INPUTS)
    clean = err.copy()
    for lane in ws.GARBAGE:
        clean[lane, 1] = w.err_est()[lane, 1]
    out = []
    for e in (err, clean):
        f = EmuStaticImpl(Case("weights_selects", model, ws.A, T=T, S=ws.S), w, w.init_positions())
        for s in range(ws.S):
            if model == 1:
                f.fused(r[s], e, w.accel(s), w.accel_cov(), w.dt_of(s))
            else:
                f.step_toa(r[s], e, w.dt_of(s))
        out.append(f.state())
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))
