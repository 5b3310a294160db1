"""The trip loop of the 9-state gain iteration (iekf9_info / iekf9_pass): what the kernel decides per wavefront must stay
invisible to every tag. A wavefront in which every lane has an accelerometer sample and a diagonal covariance runs the
fast form of the pass (no per-lane look at the sample), any other the full per-lane form; the lanes of a wavefront leave
the loop at different trips; and the convergence test takes its exact-quotient side for the whole wavefront as soon as
one iterating lane asks for it. Every comparison here is bit for bit -- the pose of every epoch, x, P, flags, status
words and latch -- except the last test, which holds the fused launch against the oracle.

T = 37 is one ragged wavefront, T = 128 two full ones; storage 2 = mixed (the bench configuration), 3 = p48."""
import numpy as np
import pytest

from conftest import has_gpu
from roskfpos_amd.synth import Workload
from test_imu9_epoch_loop_gpu import _bank, _dts, _fused, _per_epoch, _same, _trace

pytestmark = pytest.mark.gpu

A = 8
FL_HAS_IMU = np.uint32(2)
ST_NONFINITE = 0x20


def _gain_iters(status):
    return (np.asarray(status).astype(np.uint32) >> 8) & 0xFF


def _only(out, keep):
    """the rows of a (trajectory, status, x, P, flags, latch) tuple that belong to the tags in `keep`"""
    return (out[0][:, :, keep], out[1][keep], out[2][keep], out[3][keep], out[4][keep], out[5][keep])


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [37, 128])
def test_a_wavefront_in_which_only_some_lanes_hold_a_sample(T, storage):
    """ranging-only epochs (MODE_TOA) re-fuse the latched sample of the tags that have one: two of three lanes here"""
    if not has_gpu():
        pytest.skip("no GPU")
    S = 8
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    bare = np.arange(T) % 3 == 1

    def bank(partly, chunk=None, diag=None):
        b = _bank(w, T, storage, chunk=chunk, diag=diag)
        _per_epoch(b, tr, 1, dts, T)      # one fused epoch: every tag latches its sample
        x, P, fl = b.get_state()
        assert (fl & FL_HAS_IMU).all()
        if partly:
            fl[bare] &= ~FL_HAS_IMU
        b.set_state(x, P, fl)             # (both kinds of bank go through the same round trip)
        return b

    b = bank(True)
    ref = _per_epoch(b, tr, S - 1, dts, T, accel=False, s0=1)
    b.close()
    out = {}
    for name, partly, chunk, diag in (("launch per epoch", True, 1, None), ("fused", True, 25, None),
                                      ("fused, full form", True, 25, 0), ("everybody latched", False, 25, None)):
        b = bank(partly, chunk=chunk, diag=diag)
        out[name] = _fused(b, tr, S - 1, dts, T, A, accel=False, s0=1)
        b.close()
    poses = out["launch per epoch"][0]
    for name in ("launch per epoch", "fused", "fused, full form"):
        _same(out[name], (poses, ref[1][-1]) + ref[2:], name)
    assert not (out["fused"][4][bare] & FL_HAS_IMU).any() and (out["fused"][4][~bare] & FL_HAS_IMU).all()
    # the same bank with a sample on every lane takes the fast form: the lanes the two share cannot tell
    _same(_only(out["everybody latched"], ~bare), _only(out["fused"], ~bare), "latched lanes, fast against per-lane form")
    assert not np.array_equal(out["everybody latched"][2][bare], out["fused"][2][bare])   # (the sample does reach the filter)


def _seed_with_mixed_trip_counts(T, S):
    """the first workload seed for which the oracle sees a wavefront and an epoch with a capped step (20 gain iterations)
    next to one that converged within three -> (seed, epoch, wavefront)"""
    import oracle_py
    for seed in range(1, 9):
        w = Workload(T, A, seed=seed)
        tr = _trace(w, S, 2, "cpu")
        o = oracle_py.OracleBank(1, T, w.anchors, init_pos=w.init_positions(), n_threads=8)
        err, cov = w.err_est(np.float32).astype(np.float64), tr["cov_host"].astype(np.float64)
        dts = _dts(S)
        for s in range(S):
            o.step_imu(w.accel(s, np.float32).astype(np.float64), cov, 0.0)
            g = _gain_iters(o.step_toa(tr["r_host"][s], err, dts[s]))
            for wv in range((T + 63) // 64):
                lanes = g[64 * wv:64 * (wv + 1)]
                if (lanes == 20).any() and (lanes <= 3).any():
                    return seed, s, wv
    return None


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [37, 128])
def test_lanes_of_one_wavefront_that_leave_the_loop_at_different_trips(T, storage):
    if not has_gpu():
        pytest.skip("no GPU")
    S = 12
    found = _seed_with_mixed_trip_counts(T, S)
    assert found is not None, "no seed with a capped and a quickly converged step in one wavefront"
    seed = found[0]
    w = Workload(T, A, seed=seed)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    b = _bank(w, T, storage)
    ref = _per_epoch(b, tr, S, dts, T)
    b.close()
    g = _gain_iters(ref[1])
    mixed = [(s, wv) for s in range(S) for wv in range((T + 63) // 64)
             if (g[s, 64 * wv:64 * (wv + 1)] == 20).any() and (g[s, 64 * wv:64 * (wv + 1)] <= 3).any()]
    print(f"T={T} storage={storage}: seed {seed} (oracle: epoch {found[1]}, wavefront {found[2]}); "
          f"the kernel: {len(mixed)} (epoch, wavefront) pairs with gain_iters == 20 next to <= 3")
    assert mixed, "the exit masks were not exercised"
    poses = None
    for chunk in (1, 5, 25):
        b = _bank(w, T, storage, chunk=chunk)
        got = _fused(b, tr, S, dts, T, A)
        b.close()
        poses = got[0] if poses is None else poses
        _same(got, (poses, ref[1][-1]) + ref[2:], f"chunk {chunk}")


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [37, 128])
def test_a_non_finite_wave_mate_changes_nobody_else(T, storage):
    """a tag with a NaN position has a NaN cost: its vote sends the whole wavefront to the exact quotient"""
    if not has_gpu():
        pytest.skip("no GPU")
    S, S0, bad = 12, 6, 5
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    out = {}
    for name in ("plain", "with it"):
        b = _bank(w, T, storage, chunk=25)
        _fused(b, tr, S0, dts, T, A)      # past the fixed start: the covariance is invertible, the information form runs
        x, P, fl = b.get_state()
        if name == "with it":
            x[bad, :3] = np.nan
        b.set_state(x, P, fl)
        out[name] = _fused(b, tr, S - S0, dts, T, A, s0=S0)
        b.close()
    others = np.arange(T) != bad
    assert out["with it"][1][bad] & ST_NONFINITE and np.isnan(out["with it"][0][:, :, bad]).all()
    assert np.isfinite(out["plain"][0]).all() and not (out["plain"][1] & ST_NONFINITE).any()
    assert (_gain_iters(out["plain"][1][:64]) < 20).any()     # (its wave-mates do leave the loop while it iterates)
    _same(_only(out["with it"], others), _only(out["plain"], others), "the other tags")


@pytest.mark.parametrize("T", [37, 128])
def test_fused_launches_match_the_oracle(T):
    """the gate of test_imu9_epoch_loop_gpu.py: <= 1e-6 m RMS over 40 epochs with a dt per epoch (mixed storage: the
    oracle does not round its covariance the way p48 does)"""
    if not has_gpu():
        pytest.skip("no GPU")
    import oracle_py
    from roskfpos_amd import capi
    S, storage = 40, capi.STORE_MIXED
    w = Workload(T, A)
    dts = _dts(S)
    tr = _trace(w, S, storage, "cuda:0")
    b = _bank(w, T, storage)
    got = _fused(b, tr, S, dts, T, A)
    b.close()
    o = oracle_py.OracleBank(1, T, w.anchors, init_pos=w.init_positions(), n_threads=8)
    err, cov = w.err_est(np.float32).astype(np.float64), tr["cov_host"].astype(np.float64)
    for s in range(S):
        o.step_imu(w.accel(s, np.float32).astype(np.float64), cov, 0.0)
        o.step_toa(tr["r_host"][s], err, dts[s])
    xo, _ = o.get_state()
    rms = float(np.sqrt(((got[2][:, :3] - xo[:, :3]) ** 2).sum(1).mean()))
    print(f"T={T}: RMS position difference vs oracle over {S} epochs with a dt per epoch: {rms:.3e} m")
    assert rms <= 1e-6, rms
