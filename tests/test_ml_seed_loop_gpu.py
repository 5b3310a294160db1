"""ml_estimate's peeled Gauss-Newton loop (kfpos_core_ml.h: the first pass in front of the loop, without cost, SSE or
test; the voted convergence test in the loop) in the kernels that run it: the two 9-state headline kernels (mixed and
p48 storage) and the 6-state step with 8-byte storage, one tag per lane and 8 lanes per tag. T = 37 (one ragged
wavefront) and 101 (a full one and a ragged one), 8 anchors, 7 epochs with a dt of their own each.

The cases of tests/ml_seed_cases.py sit on lanes of the first wavefront next to ordinary wave-mates and are asserted to
occur on the kernel's own status words (ml_iters) before anything is compared: fewer than four ranges (the seed comes
back, 0 iterations); a lane with 1 or 2 iterations next to a lane with at least 5; ranges that fit the seed exactly (a
cost of 0: the quotient form divides 0 by 0); a used range with errorEstimation 0 (NaN position, NaN cost); a NaN
wave-mate, whose vote sends the wavefront to the quotient in every pass; an absent range with garbage in its slots.

Compared as BIT PATTERNS -- pose of every epoch, x, P, flags, status words, latch -- between one launch of 7 epochs and
seven single-epoch calls; and against runs in which the NaN wave-mate, or the garbage slots, hold an ordinary value:
nobody else's bytes change. (No kernel holds both texts, so old against new is compared between builds, on the outputs
bench.py dumps.) Against the oracle: the tolerances of tests/test_gpu_parity.py (8-byte and mixed storage <= 1e-9 m RMS,
<= 1e-8 m at worst, equal status words; p48 <= 1e-7 m / 1e-6 m, equal flags)."""
import numpy as np
import pytest

import ml_seed_cases as mc
import step_checks as sc
from conftest import has_gpu
from roskfpos_amd import capi

pytestmark = pytest.mark.gpu

A, S = mc.A, mc.S
# (model, storage, KFPOS_NO_COOP): the 9-state headline kernels; the 6-state step, one tag per lane and 8 lanes per tag
KERNELS = {"9-state mixed": (1, 2, None), "9-state p48": (1, 3, None),
           "6-state f64": (0, 0, 1), "6-state f64, 8 lanes per tag": (0, 0, None)}


def _bank(w, init, T, model, storage, no_coop):
    return sc.bank(w, T, storage, model=model, init=init, no_coop=no_coop, chunk=25)


@pytest.mark.parametrize("kernel", list(KERNELS), ids=[k.replace(" ", "_").replace(",", "") for k in KERNELS])
@pytest.mark.parametrize("T", [37, 101])
def test_every_case_same_bits_however_launched_and_within_the_oracle_bounds(T, kernel):
    if not has_gpu():
        pytest.skip("no GPU")
    model, storage, _ = KERNELS[kernel]
    real = sc.real_of(storage)
    w, init, r, err = mc.inputs(T, real)
    dts = mc.DTS
    tr = sc.Trace(w, S, storage, r=r, err=err)
    b = _bank(w, init, T, *KERNELS[kernel])
    single = sc.single_calls(b, tr, dts, S, accel=model == 1)
    b.close()
    b = _bank(w, init, T, *KERNELS[kernel])
    fused = sc.fused(b, tr, dts, S, accel=model == 1)
    b.close()
    it = mc.ml_iters(single.status)
    print(f"T={T} {kernel}: Gauss-Newton iterations per epoch, first wavefront: "
          f"min {it[:, :mc.LANES].min(1)}, max {it[:, :mc.LANES].max(1)}")
    mc.assert_cases_occur(model, r, err, init, single.status)
    sc.same(fused, single.last(), (T, kernel, "one launch against single calls"))

    # the NaN wave-mate and the garbage slots change nobody else's bytes
    clean = err.copy()
    clean[mc.NAN_ERR, 5] = w.err_est()[mc.NAN_ERR, 5]
    for lane in mc.GARBAGE:
        clean[lane, 1] = w.err_est()[lane, 1]
    b = _bank(w, init, T, *KERNELS[kernel])
    other = sc.fused(b, sc.Trace(w, S, storage, r=r, err=clean), dts, S, accel=model == 1)
    b.close()
    mates = np.arange(T) != mc.NAN_ERR
    assert np.isfinite(other.poses[:, :, mc.NAN_ERR]).all()       # (with an ordinary value that tag is an ordinary tag)
    sc.same(other.only(mates), fused.only(mates), (T, kernel, "NaN mate / garbage against clean"))

    poses, theirs = sc.oracle_run(w, r, err, dts, model=model, real=real, init=init)[:2]
    poses, mine = poses.transpose(0, 2, 1), single.status.astype(np.uint32)
    ok = np.isfinite(poses).all(1)
    assert np.array_equal(ok, np.isfinite(single.poses).all(1))
    d = np.sqrt((((single.poses - poses) ** 2).sum(1))[ok])
    rms, mx = float(np.sqrt((d ** 2).mean())), float(d.max())
    print(f"T={T} {kernel}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {S} epochs")
    cmp = mc.oracle_status_comparable(model, T)
    if storage == 3:
        assert rms <= 1e-7 and mx <= 1e-6, (rms, mx)
        assert np.array_equal(capi.st_flags(mine[cmp]), capi.st_flags(theirs[cmp]))
    else:
        assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
        assert np.array_equal(mine[cmp], theirs[cmp]), np.argwhere(mine != theirs)
