"""Inputs shared by tests/test_ml_seed_loop_emu.py and tests/test_ml_seed_loop_gpu.py: a short trace in which chosen tags
of the first wavefront reach every side of ml_estimate's peeled Gauss-Newton loop (kfpos_core_ml.h), next to ordinary
tags. A tag's synthetic trace depends on its index only, so the same lanes serve every bank size.

The anchors are not the synthetic room's: each of the eight stands at an integer distance from CENTRE (offsets with
integer norms), so that a tag which starts at CENTRE and receives those distances in whole millimetres fits its seed
EXACTLY in the first epoch -- every r - d is 0, the first step moves nothing, the second sweep has cost 0, and the third
convergence test is |0 - 0| / 0: the quotient form divides 0 by 0, says "not above", and the solve ends with 2
iterations. (36 and 49 have exact square roots in every arithmetic the kernels use; 6000 mm / 1000 is exactly 6.)"""
import functools

import numpy as np

import step_checks as sc
from roskfpos_amd.capi import ST_FEW_RANGES, ST_ML_FALLBACK, ST_NONFINITE, ST_UPDATE_SKIPPED, st_flags
from roskfpos_amd.capi import st_ml_iters as ml_iters
from roskfpos_amd.synth import Workload

A, S = 8, 7
DTS = sc.dts(S)   # a dt of its own for every epoch

CENTRE = np.array([5.0, 5.0, 1.0])
OFFSETS = np.array([[4, 4, 2], [-4, -4, 2], [-4, 4, -2], [4, -4, -2],        # norm 6
                    [2, 3, 6], [-3, 2, 6], [6, -2, 3], [-2, -6, -3]], float)  # norm 7
ANCHORS = CENTRE + OFFSETS
EXACT_MM = np.array([6000] * 4 + [7000] * 4, dtype=np.int32)

FEW = 5            # three ranges in every epoch: the seed comes back untouched, 0 iterations
EXACT = 9          # starts at CENTRE and fits it exactly in epoch 0
ZERO_ERR = 17      # a USED range (anchor 3) with errorEstimation exactly 0: weight inf, NaN position, NaN cost
NAN_ERR = 29       # a USED range (anchor 5) with errorEstimation NaN: a NaN wave-mate in every vote
GARBAGE = {3: np.nan, 13: -3.0}   # lane -> what the errorEstimation slot of its ABSENT range (anchor 1) holds
SPECIAL = (FEW, EXACT, ZERO_ERR, NAN_ERR) + tuple(GARBAGE)
LANES = 37         # the lanes of the first wavefront that every bank size of the tests has


def oracle_status_comparable(model, T, exact_fit=True):
    """[S][T]: the status words the oracle and the kernels agree on. The 9-state oracle reports the tag with a NaN
    errorEstimation on a used range (NAN_ERR, here and in weights_selects.py) with other words than the kernels, update
    skipped against iterated to the cap, as it always did. exact_fit: the trace holds this module's exact fit. The fit
    of epoch 0 is exact for the kernels' step p - Hs^-1 g only (g = 0 leaves p where it is: 2 iterations);
    the reference's solve(Hs, Hs p - g) returns p to rounding, its next cost is 1e-30 instead of 0, and it counts a
    third iteration -- at the same position to 1e-15 m, which the position bounds check."""
    ok = np.ones((S, T), dtype=bool)
    if model == 1:
        ok[:, NAN_ERR] = False
    if exact_fit:
        ok[0, EXACT] = False
    return ok


def inputs(T, real=np.float64, seed=None, cases=None, anchors=ANCHORS):
    """(workload, fixed starts [T][3], ranges [S][T][A] int32, errorEstimation [T][A] float64 holding values of `real`).
    What weights_selects.py sets otherwise (its INPUTS): seed, None = the one _seed() chooses with the oracle;
    cases(init, r, err) puts the special tags in, None = this module's; anchors, None = the synthetic room's"""
    w = Workload(T, A, seed=_seed() if seed is None else seed)
    if anchors is not None:
        w.anchors = anchors.copy()
    init = w.init_positions().copy()
    r = np.stack([w.ranges_mm(s) for s in range(S)])
    err = w.err_est().copy()
    (cases or _cases)(init, r, err)
    return w, init, r, err.astype(real).astype(np.float64)


def _cases(init, r, err):
    assert len(init) > max(SPECIAL)
    r[:, FEW, 3:] = -1
    init[EXACT] = CENTRE
    r[0, EXACT] = EXACT_MM
    err[ZERO_ERR, 3] = 0.0
    err[NAN_ERR, 5] = np.nan
    for lane, junk in GARBAGE.items():
        r[:, lane, 1] = -1
        err[lane, 1] = junk


def slow_next_to_quick(iters):
    """iters: [S][T] ml_iters -> the epochs in which, among the first LANES lanes, a lane with 1 or 2 iterations sits next
    to a lane with at least 5"""
    it = np.asarray(iters)[:, :LANES]
    return np.flatnonzero(((it >= 1) & (it <= 2)).any(1) & (it >= 5).any(1))


@functools.lru_cache(maxsize=None)
def _seed():
    """the first workload seed for which the ORACLE (9-state and 6-state, on 8-byte and on 4-byte measurements) sees, in
    the first wavefront, a lane with 1 or 2 Gauss-Newton iterations next to a lane with at least 5"""
    def occurs(seed):
        for model, real in ((1, np.float64), (1, np.float32), (0, np.float64)):
            w, init, r, err = inputs(LANES, real, seed=seed)
            st = sc.oracle_run(w, r, err, DTS, model=model, real=real, init=init)[1]
            if not len(slow_next_to_quick(ml_iters(st))):
                return False
        return True
    return sc.first_seed(range(1, 17), occurs, "a slow lane next to a quick one")


def assert_cases_occur(model, r, err, init, status):
    """status: [S][T] status words of the implementation under test. Fails when an input stopped reaching its case."""
    st = np.asarray(status).astype(np.uint32)
    it = ml_iters(st)
    # fewer than four ranges: flagged, no iteration
    assert ((r[:, FEW] > 0).sum(1) == 3).all()
    assert (st[:, FEW] & ST_FEW_RANGES).all() and (it[:, FEW] == 0).all(), (st[:, FEW], it[:, FEW])
    # the exact fit: distances in whole millimetres from the tag's start, and 2 iterations (step, cost 0, 0 / 0)
    d = np.sqrt(((ANCHORS - init[EXACT]) ** 2).sum(1))
    assert np.array_equal(d * 1000.0, r[0, EXACT].astype(np.float64))
    assert it[0, EXACT] == 2 and not st_flags(st[0, EXACT]), (it[0, EXACT], st[0, EXACT])
    # a slow lane next to a quick one in the first wavefront
    assert len(slow_next_to_quick(it)) > 0, it[:, :LANES]
    # errorEstimation 0 on a used range: the reference throws
    assert (r[:, ZERO_ERR, 3] > 0).all() and err[ZERO_ERR, 3] == 0.0
    assert (st[:, ZERO_ERR] & ST_UPDATE_SKIPPED).all()
    # the NaN wave-mate: ONE iteration (the first step is taken whatever the sums hold, the NaN cost of the second sweep
    # stops), nothing thrown
    assert (r[:, NAN_ERR, 5] > 0).all() and np.isnan(err[NAN_ERR, 5])
    assert not (st[:, NAN_ERR] & ST_UPDATE_SKIPPED).any()
    assert (it[:, NAN_ERR] == 1).all(), it[:, NAN_ERR]
    if model == 0:
        assert (st[:, NAN_ERR] & ST_ML_FALLBACK).all()
    # an absent range with garbage in its slots: the tag updates all the same
    for lane, junk in GARBAGE.items():
        assert (r[:, lane, 1] <= 0).all() and (np.isnan(junk) and np.isnan(err[lane, 1]) or err[lane, 1] == junk)
        assert (it[:, lane] >= 2).all() and not (st[:, lane] & (ST_UPDATE_SKIPPED | ST_NONFINITE)).any(), lane
    ordinary = np.setdiff1d(np.arange(st.shape[1]), SPECIAL)
    assert not st_flags(st[:, ordinary]).any() and (it[:, ordinary] >= 2).all()
