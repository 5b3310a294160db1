"""The weights of a 9-state epoch as selects (set_weights_ml, ml_covariance_throws, set_weights_iekf: every reciprocal
and every predicate is formed for every anchor, then selected) and the pairs' return as selects (iekf9_pairs_held), in
the two headline kernels: T = 37 (one ragged wavefront) and 101 (a full one, which forms pairs, and a ragged one),
8 anchors, mixed and p48 storage, 7 epochs with a dt of their own each.

The cases of tests/weights_selects.py sit on lanes of the first wavefront next to ordinary wave-mates and are asserted to
occur on the kernel's own status words: an absent range whose errorEstimation slot holds NaN, 0, inf and a negative
number; a used range with errorEstimation exactly 0 (update skipped, e_ML NaN); errorEstimations on both sides of e_ML
within one tag; fewer than four ranges; a used range with errorEstimation NaN (e_ML NaN, nothing skipped).

Compared as BIT PATTERNS -- pose of every epoch, x, P, flags, status words, latch -- between one launch of 7 epochs,
launches of 3 + 4 and seven single-epoch calls, each with the pairs' tail (the default) and with KFPOS_PAIR9=0; and
against a run whose garbage slots hold an ordinary value: such a slot changes no byte, the tag's own or anybody else's.
Against the oracle: the tolerances of tests/test_gpu_parity.py (mixed <= 1e-9 m RMS, <= 1e-8 m at worst, equal status
words; p48 <= 1e-7 m / 1e-6 m, equal flags)."""
import numpy as np
import pytest

import weights_selects as ws
from conftest import has_gpu
from test_imu9_epoch_loop_gpu import _dts, _fused
from test_pairs9_tail_gpu import _bank, _fused_split, _same_bits, _single_calls

pytestmark = pytest.mark.gpu

A, S = ws.A, ws.S


def _trace(w, r, err, dev):
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cov = w.accel_cov(np.float32)
    return dict(r=up(r.transpose(0, 2, 1)), e=up(err.astype(np.float32).T), c=up(cov.T),
                a=up(np.stack([w.accel(s, np.float32) for s in range(S)]).transpose(0, 2, 1)), r_host=r, cov_host=cov)


def _runs(w, T, storage, tr, dts, pairs):
    out = {}
    for run in ("single calls", "one launch", "3 + 4"):
        b = _bank(w, T, storage, pairs, chunk=25)
        if run == "single calls":
            out[run] = _single_calls(b, tr, dts, T, n=S)
        elif run == "one launch":
            out[run] = _fused(b, tr, S, dts, T, A)
        else:
            out[run] = _fused_split(b, tr, dts, T, split=(3, 4))
        b.close()
    return out


@pytest.mark.parametrize("storage", [2, 3], ids=["mixed", "p48"])
@pytest.mark.parametrize("T", [37, 101])
def test_every_side_of_the_selects_same_bits_however_launched_and_within_the_oracle_bounds(T, storage):
    if not has_gpu():
        pytest.skip("no GPU")
    import oracle_py
    w, r, err = ws.inputs(T, np.float32)
    dts = _dts(S)
    tr = _trace(w, r, err, "cuda:0")
    with_pairs, without = _runs(w, T, storage, tr, dts, True), _runs(w, T, storage, tr, dts, False)
    single = with_pairs["single calls"]
    ws.assert_inputs_reach_the_branches(1, w, r, err, single[1], np.float32, dts)
    as_fused = (single[0], single[1][-1]) + single[2:]
    for run in ("one launch", "3 + 4"):
        _same_bits(with_pairs[run], as_fused, (T, storage, run, "against single calls"))
        _same_bits(without[run], with_pairs[run], (T, storage, run, "KFPOS_PAIR9=0 against the default"))
    _same_bits(without["single calls"], single, (T, storage, "single calls, KFPOS_PAIR9=0 against the default"))

    # a garbage slot changes nobody's bytes
    clean = err.copy()
    for lane in ws.GARBAGE:
        clean[lane, 1] = np.float32(w.err_est()[lane, 1])
    b = _bank(w, T, storage, True, chunk=25)
    _same_bits(_fused(b, _trace(w, r, clean, "cuda:0"), S, dts, T, A), with_pairs["one launch"],
               (T, storage, "garbage slots against ordinary values"))
    b.close()

    o = oracle_py.OracleBank(1, T, w.anchors, init_pos=w.init_positions(), n_threads=8)
    cov = tr["cov_host"].astype(np.float64)
    poses, stats = [], []
    for s in range(S):
        o.step_imu(w.accel(s, np.float32).astype(np.float64), cov, 0.0)
        stats.append(np.asarray(o.step_toa(r[s], err, dts[s])).astype(np.uint32))
        poses.append(o.get_state()[0][:, :3].T.copy())
    poses, theirs, mine = np.stack(poses), np.stack(stats), single[1].astype(np.uint32)
    ok = np.isfinite(poses).all(1)
    assert np.array_equal(ok, np.isfinite(single[0]).all(1))
    d = np.sqrt((((single[0] - poses) ** 2).sum(1))[ok])
    rms, mx = float(np.sqrt((d ** 2).mean())), float(d.max())
    print(f"T={T} storage={storage}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {S} epochs")
    cmp = ws.oracle_status_comparable(1, T)
    if storage == 2:
        assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
        assert np.array_equal(mine[:, cmp], theirs[:, cmp])
    else:
        assert rms <= 1e-7 and mx <= 1e-6, (rms, mx)
        assert np.array_equal(mine[:, cmp] & 0xFF, theirs[:, cmp] & 0xFF)
