"""ml_estimate's peeled Gauss-Newton loop (kfpos_core_ml.h: the first pass in front of the loop, without cost and SSE and
without a test; the voted convergence test in the loop) on the host build of the headers, one tag at a time with 8
anchors, epoch in registers and in strided scratch, through a 9-state step and through a 6-state step, against the
oracle: the tolerances of tests/test_gpu_parity.py (<= 1e-9 m RMS, <= 1e-8 m at worst over the positions of every epoch)
and EQUAL status words, i.e. equal Gauss-Newton iteration counts.

The cases (tests/ml_seed_cases.py), each asserted to occur on the emulation's own status words: fewer than four ranges
(0 iterations); a slow lane next to a quick one; ranges that fit the seed exactly (cost 0, the quotient form divides 0 by
0); a used range with errorEstimation 0 (NaN position, NaN cost); a used range with errorEstimation NaN; an absent range
with garbage in its slots. (CPU only.)"""
import functools

import numpy as np
import pytest

import ml_seed_cases as mc
from cases import Case, rms_and_max
from impls import EmuImpl, EmuStaticImpl, OracleImpl

T = 64


def _run(model, impl):
    w, init, r, err = mc.inputs(T)
    f = impl(Case("ml_seed_loop", model, mc.A, T=T, S=mc.S), w, init)
    cov = w.accel_cov()
    pos, st = [], []
    for s in range(mc.S):
        if model == 1:
            st.append(np.asarray(f.fused(r[s], err, w.accel(s), cov, mc.DTS[s])).copy())
        else:
            st.append(np.asarray(f.step_toa(r[s], err, mc.DTS[s])).copy())
        pos.append(f.positions().copy())
    return np.stack(pos), np.stack(st).astype(np.uint32), f.state()


@functools.lru_cache(maxsize=None)
def _oracle(model):
    return _run(model, OracleImpl)


@pytest.mark.parametrize("impl", [EmuStaticImpl, EmuImpl], ids=["epoch in registers", "epoch in strided scratch"])
@pytest.mark.parametrize("model", [1, 0], ids=["9-state", "6-state"])
def test_every_case_of_the_peeled_loop_against_the_oracle(model, impl):
    pos_o, st_o, (x_o, P_o) = _oracle(model)
    pos, st, (x, P) = _run(model, impl)
    w, init, r, err = mc.inputs(T)
    mc.assert_cases_occur(model, r, err, init, st)
    rms, mx, same_nan = rms_and_max(pos, pos_o)
    print(f"model {model}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {mc.S} epochs of {T} tags; "
          f"Gauss-Newton iterations {mc.ml_iters(st).min()} .. {mc.ml_iters(st).max()}")
    assert same_nan
    assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
    cmp = mc.oracle_status_comparable(model, T)
    assert np.array_equal(st[cmp], st_o[cmp]), np.argwhere(st != st_o)
    assert np.array_equal(mc.ml_iters(st)[cmp], mc.ml_iters(st_o)[cmp])
    ok = np.isfinite(x_o).all(1) & np.isfinite(P_o).all((1, 2))
    assert np.array_equal(ok, np.isfinite(x).all(1) & np.isfinite(P).all((1, 2)))
    assert np.abs(P_o[ok] - P[ok]).max() <= 1e-9 * np.abs(P_o[ok]).max()


def test_the_exact_fit_is_what_the_status_mask_says_it_is():
    """the one status word left out of the comparison (ml_seed_cases.oracle_status_comparable): the oracle counts 3
    iterations at the exact fit, the headers 2, and the positions agree far inside the bound"""
    for model in (1, 0):
        pos_o, st_o, _ = _oracle(model)
        pos, st, _ = _run(model, EmuStaticImpl)
        assert mc.ml_iters(st_o)[0, mc.EXACT] == 3 and mc.ml_iters(st)[0, mc.EXACT] == 2
        assert np.abs(pos[0, mc.EXACT] - pos_o[0, mc.EXACT]).max() <= 1e-12
