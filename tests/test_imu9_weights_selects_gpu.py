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

import ml_seed_cases as mc
import step_checks as sc
import weights_selects as ws
from conftest import has_gpu
from roskfpos_amd import capi

pytestmark = pytest.mark.gpu

A, S = ws.A, ws.S


def _runs(w, T, storage, tr, dts, pairs):
    """pairs: the default (KFPOS_PAIR9 unset) or KFPOS_PAIR9=0"""
    out = {}
    for run in ("single calls", "one launch", "3 + 4"):
        b = sc.bank(w, T, storage, pairs=sc.UNSET if pairs else 0, chunk=25)
        if run == "single calls":
            out[run] = sc.single_calls(b, tr, dts, S)
        elif run == "one launch":
            out[run] = sc.fused(b, tr, dts, S)
        else:
            out[run] = sc.fused_split(b, tr, dts, S, split=3)
        b.close()
    return out


@pytest.mark.parametrize("storage", [2, 3], ids=["mixed", "p48"])
@pytest.mark.parametrize("T", [37, 101])
def test_every_side_of_the_selects_same_bits_however_launched_and_within_the_oracle_bounds(T, storage):
    if not has_gpu():
        pytest.skip("no GPU")
    w, init, r, err = mc.inputs(T, np.float32, **ws.INPUTS)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, r=r, err=err)
    with_pairs, without = _runs(w, T, storage, tr, dts, True), _runs(w, T, storage, tr, dts, False)
    single = with_pairs["single calls"]
    ws.assert_inputs_reach_the_branches(1, w, r, err, single.status, np.float32, dts)
    for run in ("one launch", "3 + 4"):
        sc.same(with_pairs[run], single.last(), (T, storage, run, "against single calls"))
        sc.same(without[run], with_pairs[run], (T, storage, run, "KFPOS_PAIR9=0 against the default"))
    sc.same(without["single calls"], single, (T, storage, "single calls, KFPOS_PAIR9=0 against the default"))

    # a garbage slot changes nobody's bytes
    clean = err.copy()
    for lane in ws.GARBAGE:
        clean[lane, 1] = np.float32(w.err_est()[lane, 1])
    b = sc.bank(w, T, storage, chunk=25)
    sc.same(sc.fused(b, sc.Trace(w, S, storage, r=r, err=clean), dts, S), with_pairs["one launch"],
            (T, storage, "garbage slots against ordinary values"))
    b.close()

    poses, theirs = sc.oracle_run(w, r, err, dts, real=np.float32, init=init)[:2]
    poses, mine = poses.transpose(0, 2, 1), single.status.astype(np.uint32)
    ok = np.isfinite(poses).all(1)
    assert np.array_equal(ok, np.isfinite(single.poses).all(1))
    d = np.sqrt((((single.poses - poses) ** 2).sum(1))[ok])
    rms, mx = float(np.sqrt((d ** 2).mean())), float(d.max())
    print(f"T={T} storage={storage}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {S} epochs")
    cmp = mc.oracle_status_comparable(1, T, exact_fit=False)
    if storage == 2:
        assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
        assert np.array_equal(mine[cmp], theirs[cmp])
    else:
        assert rms <= 1e-7 and mx <= 1e-6, (rms, mx)
        assert np.array_equal(capi.st_flags(mine[cmp]), capi.st_flags(theirs[cmp]))
