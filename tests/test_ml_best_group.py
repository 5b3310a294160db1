"""MLLocation's third variant, estimatePositionBestGroup (MLLocation.cpp:348-414), where the reference defines it: 4 or
5 ranges. (With 6 and more its erase loop, :377-381, removes by an index into the vector it is shrinking and addresses
end() from the first group on: undefined, refused -- kfpos_set_anchors returns KFPOS_ERR_MODEL.)

Pinned here without the reference (parity unpinned):
  * what the text of :348-414 implies, checked on the oracle with nothing but the NORMAL estimator, which has its own
    tests: one group = NORMAL with 4 ranges; five groups = NORMAL on each 4-subset, smallest covariance trace wins,
    `<=` lets the LATER group win a tie, group order "without range 4, 3, 2, 1, 0";
  * kernel body (host build) and GPU against the oracle: identical status words -- winner, Gauss-Newton passes -- and
    positions to 1e-9 m for every tag whose groups all converged within 15 passes (the regimes of test_ml_estimator).
"""
import numpy as np
import pytest

import oracle_py
from conftest import has_gpu
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload, anchors_xyz

BEST = 2


def _epoch(w, s, n_present=None):
    r = w.ranges_mm(s)
    r[::6, 2] += 600                      # an NLOS-like bias on one anchor of every sixth tag
    if s % 3 == 1:
        r[1::4, 0] = 0                    # 5 anchors -> 4 ranges: one group
    if s % 5 == 4:
        r[2::7, 1:3] = -1                 # 3 ranges: the seed comes back
    return r


def test_oracle_best_group_is_the_argmin_over_four_subsets():
    T, A = 64, 5
    w = Workload(T, A)
    seed = w.init_positions() + 0.3
    best = oracle_py.OracleBank(oracle_py.MODEL_ML, T, w.anchors, init_pos=seed, ml_variant=BEST, n_threads=4)
    for s in range(6):
        r = _epoch(w, s)
        st = best.step_toa(r, w.err_est(), 0.05)
        pb, cb, _, _ = best.get_pose(0.0)
        for t in range(T):
            present = np.flatnonzero(r[t] > 0)
            if len(present) < 4:
                assert st[t] & 4 and np.array_equal(pb[t], seed[t])
                continue
            groups = [present] if len(present) == 4 else [np.delete(present, k) for k in (4, 3, 2, 1, 0)]
            res = []
            for g in groups:   # the NORMAL estimator on exactly those ranges, in anchor order
                p, c, it = oracle_py.ml_estimate(w.anchors[g], r[t, g] / 1000.0, w.err_est()[t, g], seed[t])
                res.append((np.trace(c), p, c, it))
            win = 0
            for i, (tr, _, _, _) in enumerate(res):   # :398-411
                if tr <= res[win][0]:
                    win = i
            assert np.array_equal(pb[t], res[win][1]) and np.allclose(cb[t], res[win][2], rtol=1e-13, atol=0)
            left_out = -1 if len(present) == 4 else (4, 3, 2, 1, 0)[win]
            assert capi.st_ignored(st[t]) == left_out
            assert capi.st_ml_iters(st[t]) == min(res[win][3], 255)
            assert capi.st_gain_iters(st[t]) == min(max(x[3] for x in res), 255)


def test_oracle_tie_goes_to_the_later_group_and_six_ranges_are_refused():
    # Anchors 3 and 4 sit straight above and below the tag, mirror images in z; 0, 1, 2 lie in the tag's plane. The
    # groups "without 4" (enumerated first) and "without 3" (second) are mirror images of each other -- every
    # floating-point operation commutes with the sign flip, so their covariance traces are EQUAL, bit for bit -- and
    # they are the best two (the other groups lose an in-plane anchor). `<=` (:407) hands the win to the second.
    anc = np.array([[0.0, 0, 0], [10, 0, 0], [5, 10, 0], [5, 3, 2.0], [5, 3, -2.0]])
    truth = np.array([5.0, 3.0, 0.0])
    r = np.round(np.sqrt(((anc - truth) ** 2).sum(1)) * 1000).astype(np.int32)[None]
    err = np.full((1, 5), 0.0025)
    seed = np.array([[5.2, 3.1, 0.0]])
    traces = []
    for k in (4, 3, 2, 1, 0):
        g = np.delete(np.arange(5), k)
        _, c, _ = oracle_py.ml_estimate(anc[g], r[0, g] / 1000.0, err[0, g], seed[0])
        traces.append(np.trace(c))
    assert traces[0] == traces[1] == min(traces) and traces[2] > traces[0]
    b = oracle_py.OracleBank(oracle_py.MODEL_ML, 1, anc, init_pos=seed, ml_variant=BEST)
    st = b.step_toa(r, err, 0.05)
    assert capi.st_ignored(st[0]) == 3          # "without range 3": the later of the tied pair
    six = oracle_py.OracleBank(oracle_py.MODEL_ML, 2, anchors_xyz(6), init_pos=np.ones((2, 3)), ml_variant=BEST)
    st = six.step_toa(Workload(2, 6).ranges_mm(0), np.full((2, 6), 0.0025), 0.05)
    assert np.all(st & 1)       # undefined in the reference: reported, nothing estimated


def _judge(sk, so, pk, po, ck, co):
    assert np.array_equal(sk & 0xFF, so & 0xFF)
    passes = capi.st_gain_iters(so).astype(int)          # the most passes any group of the tag took
    few = (so & 4) != 0
    tame = passes <= 15
    assert np.array_equal(sk[tame], so[tame])        # winner, its passes, the most passes: identical
    d = np.abs(pk - po).max(1)
    assert d[tame].max(initial=0.0) < 1e-9
    ok = tame & ~few
    assert np.allclose(ck[ok], co[ok], rtol=1e-5, atol=1e-14)
    assert tame.mean() > 0.9
    return int((~tame).sum())


@pytest.mark.parametrize("static", [False, True])
def test_kernel_body_best_group_matches_oracle(static):
    from impls import emu_lib
    T, A, S = 600, 5, 10
    w = Workload(T, A)
    seed = np.ascontiguousarray(w.init_positions() + 0.3)
    L = emu_lib()
    h = L.kfe_create(2, T, A, np.ascontiguousarray(w.anchors), 0.5, 0.5, 0, 0.5, 0, 1, seed.ctypes.data)
    L.kfe_set_static(h, int(static))
    L.kfe_set_ml_variant(h, BEST)
    orc = oracle_py.OracleBank(oracle_py.MODEL_ML, T, w.anchors, init_pos=seed, ml_variant=BEST, n_threads=8)
    for s in range(S):
        r = _epoch(w, s)
        se = np.zeros(T, dtype=np.uint32)
        L.kfe_step_toa(h, r, w.err_est(), np.array([0.05]), 1, se.ctypes.data)
        so = orc.step_toa(r, w.err_est(), 0.05)
        x, P = np.zeros((T, 3)), np.zeros((T, 3, 3))
        L.kfe_get_state(h, x, P)
        po, co, _, _ = orc.get_pose(0.0)
        _judge(se, so, x, po, P, co)
    L.kfe_destroy(h)


def test_kernel_body_resolves_the_exact_tie_like_the_reference():
    from impls import emu_lib
    anc = np.ascontiguousarray(np.array([[0.0, 0, 0], [10, 0, 0], [5, 10, 0], [5, 3, 2.0], [5, 3, -2.0]]))
    r = np.round(np.sqrt(((anc - np.array([5.0, 3.0, 0.0])) ** 2).sum(1)) * 1000).astype(np.int32)[None]
    seed = np.array([[5.2, 3.1, 0.0]])
    L = emu_lib()
    for static in (0, 1):
        h = L.kfe_create(2, 1, 5, anc, 0.5, 0.5, 0, 0.5, 0, 1, seed.ctypes.data)
        L.kfe_set_static(h, static)
        L.kfe_set_ml_variant(h, BEST)
        se = np.zeros(1, dtype=np.uint32)
        L.kfe_step_toa(h, np.ascontiguousarray(r), np.full((1, 5), 0.0025), np.array([0.05]), 1, se.ctypes.data)
        assert capi.st_ignored(se[0]) == 3
        L.kfe_destroy(h)


@pytest.mark.gpu
@pytest.mark.parametrize("A,storage", [(5, 0), (5, 2), (4, 0)])
def test_gpu_best_group_matches_oracle(A, storage):
    if not has_gpu():
        pytest.skip("no GPU")
    from roskfpos_amd import capi
    T, S = 3000, 10
    w = Workload(T, A)
    if A == 4:   # the first four room corners are coplanar (z = 0.3): take three of them and one at the ceiling
        w.anchors = anchors_xyz(5)[[0, 1, 2, 4]].copy()
    real = np.float32 if storage else np.float64
    seed = w.init_positions() + 0.3
    gpu = capi.KfposBank(capi.MODEL_ML, T, w.anchors, storage=storage, init_pos=seed, ml_variant=capi.ML_BEST)
    orc = oracle_py.OracleBank(oracle_py.MODEL_ML, T, w.anchors, init_pos=seed, ml_variant=BEST, n_threads=8)
    err = w.err_est(real)
    for s in range(S):
        r = _epoch(w, s) if A == 5 else w.ranges_mm(s)
        sg = gpu.step_toa(r, err, 0.05)
        so = orc.step_toa(r, err.astype(np.float64), 0.05)
        pg, cg, _, _ = gpu.get_pose(0.0)
        po, co, _, _ = orc.get_pose(0.0)
        _judge(sg, so, pg, po, cg, co)
    gpu.close()
    # six anchors: no defined result in the reference, refused when the anchor table is set
    with pytest.raises(capi.KfposError, match="estimatePositionBestGroup"):
        capi.KfposBank(capi.MODEL_ML, 8, anchors_xyz(6), init_pos=np.ones(3), ml_variant=capi.ML_BEST)
    with pytest.raises(capi.KfposError, match="ml_variant"):
        capi.KfposBank(capi.MODEL_TOA, 8, anchors_xyz(5), init_pos=np.ones(3), ml_variant=capi.ML_BEST)
