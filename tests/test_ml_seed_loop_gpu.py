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
from conftest import has_gpu
from replay_checks import env
from test_imu9_epoch_loop_gpu import _fused
from test_pairs9_tail_gpu import _same_bits, _single_calls

pytestmark = pytest.mark.gpu

A, S = mc.A, mc.S
# (model, storage, KFPOS_NO_COOP): the 9-state headline kernels; the 6-state step, one tag per lane and 8 lanes per tag
KERNELS = {"9-state mixed": (1, 2, None), "9-state p48": (1, 3, None),
           "6-state f64": (0, 0, 1), "6-state f64, 8 lanes per tag": (0, 0, None)}


def _trace(w, r, err, real, dev):
    import torch
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    cov = w.accel_cov(real)
    return dict(r=up(r.transpose(0, 2, 1)), e=up(err.astype(real).T), c=up(cov.T),
                a=up(np.stack([w.accel(s, real) for s in range(S)]).transpose(0, 2, 1)), r_host=r, cov_host=cov)


def _bank(w, init, T, model, storage, no_coop):
    from roskfpos_amd import capi
    with env(KFPOS_NO_COOP=no_coop, KFPOS_TRACE_CHUNK_STEPS=25):
        return capi.KfposBank(model, T, w.anchors, storage=storage, init_pos=init)


def _both(w, init, T, kernel, tr, dts):
    model, storage, no_coop = kernel
    b = _bank(w, init, T, model, storage, no_coop)
    single = _single_calls(b, tr, dts, T, accel=model == 1, n=S)
    b.close()
    b = _bank(w, init, T, model, storage, no_coop)
    fused = _fused(b, tr, S, dts, T, A, accel=model == 1)
    b.close()
    return single, fused


@pytest.mark.parametrize("kernel", list(KERNELS), ids=[k.replace(" ", "_").replace(",", "") for k in KERNELS])
@pytest.mark.parametrize("T", [37, 101])
def test_every_case_same_bits_however_launched_and_within_the_oracle_bounds(T, kernel):
    if not has_gpu():
        pytest.skip("no GPU")
    import oracle_py
    model, storage, _ = KERNELS[kernel]
    real = np.float64 if storage == 0 else np.float32
    w, init, r, err = mc.inputs(T, real)
    dts = mc.DTS
    tr = _trace(w, r, err, real, "cuda:0")
    single, fused = _both(w, init, T, KERNELS[kernel], tr, dts)
    it = mc.ml_iters(single[1])
    print(f"T={T} {kernel}: Gauss-Newton iterations per epoch, first wavefront: "
          f"min {it[:, :mc.LANES].min(1)}, max {it[:, :mc.LANES].max(1)}")
    mc.assert_cases_occur(model, r, err, init, single[1])
    _same_bits(fused, (single[0], single[1][-1]) + single[2:], (T, kernel, "one launch against single calls"))

    # the NaN wave-mate and the garbage slots change nobody else's bytes
    clean = err.copy()
    clean[mc.NAN_ERR, 5] = w.err_est()[mc.NAN_ERR, 5]
    for lane in mc.GARBAGE:
        clean[lane, 1] = w.err_est()[lane, 1]
    b = _bank(w, init, T, *KERNELS[kernel])
    other = _fused(b, _trace(w, r, clean, real, "cuda:0"), S, dts, T, A, accel=model == 1)
    b.close()
    mates = np.arange(T) != mc.NAN_ERR
    assert np.isfinite(other[0][:, :, mc.NAN_ERR]).all()       # (with an ordinary value that tag is an ordinary tag)
    for k, name in enumerate(("pose of every epoch", "status", "x", "P", "flags", "latch")):
        a_, b_ = np.ascontiguousarray(other[k]), np.ascontiguousarray(fused[k])
        tags = 2 if k == 0 else 0                               # the axis that counts tags
        a_, b_ = np.compress(mates, a_, axis=tags), np.compress(mates, b_, axis=tags)
        assert np.array_equal(a_.view(np.uint8), b_.view(np.uint8)), (T, kernel, "NaN mate / garbage against clean", name)

    o = oracle_py.OracleBank(model, T, w.anchors, init_pos=init, n_threads=8)
    cov = tr["cov_host"].astype(np.float64)
    poses, stats = [], []
    for s in range(S):
        if model == 1:
            o.step_imu(w.accel(s, real).astype(np.float64), cov, 0.0)
        stats.append(np.asarray(o.step_toa(r[s], err, dts[s])).astype(np.uint32))
        poses.append(o.get_state()[0][:, :3].T.copy())
    poses, theirs, mine = np.stack(poses), np.stack(stats), single[1].astype(np.uint32)
    ok = np.isfinite(poses).all(1)
    assert np.array_equal(ok, np.isfinite(single[0]).all(1))
    d = np.sqrt((((single[0] - poses) ** 2).sum(1))[ok])
    rms, mx = float(np.sqrt((d ** 2).mean())), float(d.max())
    print(f"T={T} {kernel}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {S} epochs")
    cmp = mc.oracle_status_comparable(model, T)
    if storage == 3:
        assert rms <= 1e-7 and mx <= 1e-6, (rms, mx)
        assert np.array_equal(mine[cmp] & 0xFF, theirs[cmp] & 0xFF)
    else:
        assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
        assert np.array_equal(mine[cmp], theirs[cmp]), np.argwhere(mine != theirs)
