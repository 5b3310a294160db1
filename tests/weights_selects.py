"""Inputs shared by tests/test_weights_selects_emu.py and tests/test_imu9_weights_selects_gpu.py: a short trace in which
chosen tags reach every side of the selects of set_weights_ml, ml_covariance_throws and set_weights_iekf
(kfpos_core_ml.h), next to ordinary tags.

A tag's synthetic trace depends on its index only, so the same lanes serve every bank size. errorEstimation is one row
per tag for the whole trace (the entry points take it with stride 0), so a scenario is a tag."""
import numpy as np

from ml_seed_cases import A, NAN_ERR, S
from roskfpos_amd.capi import (ST_FEW_RANGES, ST_ML_FALLBACK, ST_NONFINITE, ST_UPDATE_SKIPPED, st_flags,
                               st_gain_iters)
from roskfpos_amd.synth import SEED

# lane -> what the errorEstimation slot of its ABSENT range (anchor 1, absent in every epoch) holds
GARBAGE = {3: np.nan, 7: 0.0, 11: np.inf, 13: -3.0}
ZERO_ERR = 17      # a USED range (anchor 3) with errorEstimation exactly 0: the update is skipped, e_ML is NaN
BETWEEN = 19       # errorEstimations from 5e-4 to 1 m^2 around e_ML (about 1e-2): both sides of the select in one tag
FEW = 23           # two ranges in epochs 2 and 5, three in epoch 4
# NAN_ERR (ml_seed_cases.py's lane): a USED range (anchor 5) with errorEstimation NaN: weights and ML position are NaN
# and the zero test does not fire. The 9-state filter goes on with e_ML NaN (and a NaN state: the oracle reports such a
# tag with other status words than the kernels: ml_seed_cases.oracle_status_comparable); the 6-state filter falls back
# to the predicted position, whose e_ML is finite
SPREAD = (5e-4, 0.5, 1e-3, 1.0, 2e-3, 0.25, 2.5e-3, 0.1)
SPECIAL = tuple(GARBAGE) + (ZERO_ERR, BETWEEN, FEW, NAN_ERR)


def cases(init, r, err):
    """ml_seed_cases.inputs(T, real, **INPUTS): this module's special tags, in the synthetic room, on its usual seed"""
    assert len(init) > max(SPECIAL)
    for lane, junk in GARBAGE.items():
        r[:, lane, 1] = -1
        err[lane, 1] = junk
    r[0, 7, 1] = 0                      # (the other spelling of an absent range)
    err[ZERO_ERR, 3] = 0.0
    err[BETWEEN] = SPREAD
    r[2, FEW, 2:] = 0
    r[5, FEW, 2:] = -1
    r[4, FEW, 3:] = 0
    err[NAN_ERR, 5] = np.nan


INPUTS = dict(seed=SEED, cases=cases, anchors=None)


def e_ml_of(model, w, r, err, lane, real=np.float64, dts=None):
    """e_ML of every epoch of one tag, as the numpy oracle's filter forms it (its last ml_error call of a step)"""
    import numpy_oracle
    f = numpy_oracle.NumpyFilter(model, w.anchors, init_pos=w.init_positions()[lane])
    seen, out, orig = [], [], numpy_oracle.ml_error

    def recording(meas, p):
        seen.append(orig(meas, p))
        return seen[-1]

    numpy_oracle.ml_error = recording
    try:
        cov = w.accel_cov(real).astype(np.float64)[lane]
        for s in range(S):
            del seen[:]
            if model == 1:
                f.step_imu(w.accel(s, real).astype(np.float64)[lane], cov, 0.0)
            f.step_toa(r[s, lane], err[lane], w.dt_of(s) if dts is None else dts[s])
            out.append(seen[-1] if seen else np.nan)
    finally:
        numpy_oracle.ml_error = orig
    return np.array(out)


def assert_inputs_reach_the_branches(model, w, r, err, status, real=np.float64, dts=None):
    """status: [S][T] status words of the implementation under test. Fails when an input stopped reaching its case."""
    st = np.asarray(status).astype(np.uint32)
    gains = st_gain_iters(st)
    for lane, junk in GARBAGE.items():   # absent in every epoch, the slot holds the junk, the tag updates all the same
        assert (r[:, lane, 1] <= 0).all() and (np.isnan(junk) and np.isnan(err[lane, 1]) or err[lane, 1] == junk)
        assert (gains[:, lane] > 0).all() and not (st[:, lane] & (ST_UPDATE_SKIPPED | ST_NONFINITE)).any(), lane
    assert (r[:, ZERO_ERR, 3] > 0).all() and err[ZERO_ERR, 3] == 0.0
    assert (st[:, ZERO_ERR] & ST_UPDATE_SKIPPED).all()
    assert np.isnan(e_ml_of(model, w, r, err, ZERO_ERR, real, dts)).all()
    e = e_ml_of(model, w, r, err, BETWEEN, real, dts)
    both = [(e[s] < err[BETWEEN]).any() and not (e[s] < err[BETWEEN]).all() for s in range(S)]
    assert any(both) and (gains[:, BETWEEN] > 0).all(), (e, err[BETWEEN])
    few = (st[:, FEW] & ST_FEW_RANGES) != 0
    assert few.tolist() == [s in (2, 4, 5) for s in range(S)], few
    assert (r[:, NAN_ERR, 5] > 0).all() and np.isnan(err[NAN_ERR, 5])
    if model == 1:
        assert np.isnan(e_ml_of(model, w, r, err, NAN_ERR, real, dts)).all()
    else:
        assert (st[:, NAN_ERR] & ST_ML_FALLBACK).all()
    assert not (st[:, NAN_ERR] & ST_UPDATE_SKIPPED).any()
    ordinary = np.setdiff1d(np.arange(st.shape[1]), SPECIAL)
    assert not st_flags(st[:, ordinary]).any() and (gains[:, ordinary] > 0).all()
