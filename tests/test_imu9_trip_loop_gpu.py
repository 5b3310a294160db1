"""The trip loop of the 9-state gain iteration (iekf9_info / iekf9_pass): what the kernel decides per wavefront must stay
invisible to every tag. A wavefront in which every lane has an accelerometer sample and a diagonal covariance runs the
fast form of the pass (no per-lane look at the sample), any other the full per-lane form; the lanes of a wavefront leave
the loop at different trips; and the convergence test takes its exact-quotient side for the whole wavefront as soon as
one iterating lane asks for it. Every comparison here is bit for bit -- the pose of every epoch, x, P, flags, status
words and latch -- except the last test, which holds the fused launch against the oracle.

T = 37 is one ragged wavefront, T = 128 two full ones; storage 2 = mixed (the bench configuration), 3 = p48."""
import functools

import numpy as np
import pytest

import step_checks as sc
from conftest import has_gpu
from roskfpos_amd import capi
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

A = 8


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [37, 128])
def test_a_wavefront_in_which_only_some_lanes_hold_a_sample(T, storage):
    """ranging-only epochs (MODE_TOA) re-fuse the latched sample of the tags that have one: two of three lanes here"""
    if not has_gpu():
        pytest.skip("no GPU")
    S = 8
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    bare = np.arange(T) % 3 == 1

    def bank(partly, chunk=None, diag=None):
        b = sc.bank(w, T, storage, chunk=chunk, diag=diag)
        sc.single_calls(b, tr, dts, 1, poses=False)      # one fused epoch: every tag latches its sample
        x, P, fl = b.get_state()
        assert (fl & sc.FL_HAS_IMU).all()
        if partly:
            fl[bare] &= ~sc.FL_HAS_IMU
        b.set_state(x, P, fl)             # (both kinds of bank go through the same round trip)
        return b

    b = bank(True)
    ref = sc.single_calls(b, tr, dts, S - 1, s0=1, accel=False, poses=False)
    b.close()
    out = {}
    for name, partly, chunk, diag in (("launch per epoch", True, 1, None), ("fused", True, 25, None),
                                      ("fused, full form", True, 25, 0), ("everybody latched", False, 25, None)):
        b = bank(partly, chunk=chunk, diag=diag)
        out[name] = sc.fused(b, tr, dts, S - 1, s0=1, accel=False)
        b.close()
    poses = out["launch per epoch"].poses
    for name in ("launch per epoch", "fused", "fused, full form"):
        sc.same(out[name], ref.last(poses), name)
    fl = out["fused"].flags
    assert not (fl[bare] & sc.FL_HAS_IMU).any() and (fl[~bare] & sc.FL_HAS_IMU).all()
    # the same bank with a sample on every lane takes the fast form: the lanes the two share cannot tell
    sc.same(out["everybody latched"].only(~bare), out["fused"].only(~bare), "latched lanes, fast against per-lane form")
    assert not np.array_equal(out["everybody latched"].x[bare], out["fused"].x[bare])   # (the sample does reach the filter)


def _mixed(g, T):
    """g: [S][T] gain iterations -> the (epoch, wavefront) pairs with a capped step (20) next to one that converged within 3"""
    return [(s, wv) for s in range(len(g)) for wv in range((T + 63) // 64)
            if (g[s, 64 * wv:64 * (wv + 1)] == 20).any() and (g[s, 64 * wv:64 * (wv + 1)] <= 3).any()]


@functools.lru_cache(maxsize=None)
def _oracle_mixed(T, S, seed):
    w = Workload(T, A, seed=seed)
    r = sc.Trace(w, S, 2, "cpu", gaps=True).r_host
    return _mixed(capi.st_gain_iters(sc.oracle_run(w, r, w.err_est(), sc.dts(S), real=np.float32,
                                                   init=w.init_positions())[1]), T)


def _seed_with_mixed_trip_counts(T, S):
    """the first workload seed for which the oracle sees a wavefront and an epoch with a capped step (20 gain iterations)
    next to one that converged within three -> (seed, epoch, wavefront)"""
    seed = sc.first_seed(range(1, 9), lambda sd: _oracle_mixed(T, S, sd),
                         "a capped and a quickly converged step in one wavefront")
    return (seed,) + _oracle_mixed(T, S, seed)[0]


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [37, 128])
def test_lanes_of_one_wavefront_that_leave_the_loop_at_different_trips(T, storage):
    if not has_gpu():
        pytest.skip("no GPU")
    S = 12
    seed, epoch, wavefront = _seed_with_mixed_trip_counts(T, S)
    w = Workload(T, A, seed=seed)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    b = sc.bank(w, T, storage)
    ref = sc.single_calls(b, tr, dts, S, poses=False)
    b.close()
    mixed = _mixed(capi.st_gain_iters(ref.status), T)
    print(f"T={T} storage={storage}: seed {seed} (oracle: epoch {epoch}, wavefront {wavefront}); "
          f"the kernel: {len(mixed)} (epoch, wavefront) pairs with gain_iters == 20 next to <= 3")
    assert mixed, "the exit masks were not exercised"
    poses = None
    for chunk in (1, 5, 25):
        b = sc.bank(w, T, storage, chunk=chunk)
        got = sc.fused(b, tr, dts, S)
        b.close()
        poses = got.poses if poses is None else poses
        sc.same(got, ref.last(poses), f"chunk {chunk}")


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [37, 128])
def test_a_non_finite_wave_mate_changes_nobody_else(T, storage):
    """a tag with a NaN position has a NaN cost: its vote sends the whole wavefront to the exact quotient"""
    if not has_gpu():
        pytest.skip("no GPU")
    S, S0, bad = 12, 6, 5
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    out = {}
    for name in ("plain", "with it"):
        b = sc.bank(w, T, storage, chunk=25)
        sc.fused(b, tr, dts, S0)      # past the fixed start: the covariance is invertible, the information form runs
        x, P, fl = b.get_state()
        if name == "with it":
            x[bad, :3] = np.nan
        b.set_state(x, P, fl)
        out[name] = sc.fused(b, tr, dts, S - S0, s0=S0)
        b.close()
    others = np.arange(T) != bad
    plain, with_it = out["plain"], out["with it"]
    assert with_it.status[bad] & capi.ST_NONFINITE and np.isnan(with_it.poses[:, :, bad]).all()
    assert np.isfinite(plain.poses).all() and not (plain.status & capi.ST_NONFINITE).any()
    assert (capi.st_gain_iters(plain.status[:64]) < 20).any()     # (its wave-mates do leave the loop while it iterates)
    sc.same(with_it.only(others), plain.only(others), "the other tags")


@pytest.mark.parametrize("T", [37, 128])
def test_fused_launches_match_the_oracle(T):
    """the gate of test_imu9_epoch_loop_gpu.py: <= 1e-6 m RMS over 40 epochs with a dt per epoch (mixed storage: the
    oracle does not round its covariance the way p48 does)"""
    if not has_gpu():
        pytest.skip("no GPU")
    S, storage = 40, capi.STORE_MIXED
    w = Workload(T, A)
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    b = sc.bank(w, T, storage)
    got = sc.fused(b, tr, dts, S)
    b.close()
    xo = sc.oracle_run(w, tr.r_host, w.err_est(), dts, real=np.float32, init=w.init_positions())[2]
    rms = float(np.sqrt(((got.x[:, :3] - xo[:, :3]) ** 2).sum(1).mean()))
    print(f"T={T}: RMS position difference vs oracle over {S} epochs with a dt per epoch: {rms:.3e} m")
    assert rms <= 1e-6, rms
