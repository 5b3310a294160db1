"""The pairs' tail of the 9-state gain iteration in the two headline kernels (iekf9_pairs_held: what a pair trip reads is
held in registers in front of its loop; a hand-over that moves only what is needed; the pair pass in the form its
wavefront runs) against the same kernel without the hand-over. The tail is the default in these two storage modes, so
every comparison is between a bank created with KFPOS_PAIR9 unset and one created with KFPOS_PAIR9=0 (read at
kfpos_create), and every comparison is made on BIT PATTERNS: the pose of every epoch, state, covariance, flags, status
words and latch.

Shapes: T = 64 is one wavefront, T = 128 two, T = 101 one full wavefront and a ragged one, which never forms pairs.
Storage 2 = mixed (the bench configuration), 3 = p48. Runs: 30 epochs as single-epoch calls, and as fused launches of
7 + 23 epochs.

The scenarios are asserted on the kernel's own status words ((s >> 8) & 0xFF = the solve count): the lanes of a
wavefront meet after 8 solves, so the lanes with a final count >= 8 are exactly those still iterating there -- more than
32 of them: they meet again at 12; at most 32: the hand-over happens at 8; a final count of exactly 8 among them: that
survivor converged in the pair's first pass and its owner's wl / mrlast / dlast must be its own untouched values. The
workload's seed is chosen with the oracle on the CPU so that all of them occur in the first wavefront; a test fails if
its scenario does not occur in the kernel's run."""
import functools

import numpy as np
import pytest

import step_checks as sc
from conftest import has_gpu
from roskfpos_amd import capi
from roskfpos_amd.capi import st_gain_iters as _gain_iters
from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

A, S = 8, 30
SPLIT = 7          # fused launches of 7 epochs and the rest


def _scenarios(g):
    """g: [epoch][64] solve counts of one full wavefront -> which scenarios it holds, as {name: [epochs]}. A wavefront
    forms pairs only when every lane runs the iteration (count > 0 on every lane here: a lane without an update leaves
    the step early)."""
    n8 = (g >= 8).sum(1)
    all_in = (g > 0).all(1)
    formed = all_in & (n8 >= 1)
    return {
        "more than 32 at 8": np.flatnonzero(all_in & (n8 > 32)),
        "at most 32 at 8": np.flatnonzero(formed & (n8 <= 32) & (g > 8).any(1)),
        "count of exactly 8": np.flatnonzero(formed & (n8 <= 32) & (g == 8).any(1) & (g > 8).any(1)),
        "cap next to <= 3": np.flatnonzero(formed & (g == 20).any(1) & (g <= 3).any(1)),
    }


@functools.lru_cache(maxsize=None)
def _seed():
    """the first workload seed for which the ORACLE sees every scenario in the first wavefront (tags 0 .. 63: a tag's
    trace does not depend on how many tags the workload has, so the seed serves every shape)"""
    def occurs(seed):
        w = Workload(64, A, seed=seed)
        r = sc.Trace(w, S, 2, "cpu", gaps=True).r_host
        st = sc.oracle_run(w, r, w.err_est(), sc.dts(S), real=np.float32, init=w.init_positions())[1]
        return all(len(v) for v in _scenarios(_gain_iters(st)).values())
    return sc.first_seed(range(1, 9), occurs, "every pair scenario in one wavefront")


def _bank(w, T, storage, pairs, **kw):
    """pairs: the default (KFPOS_PAIR9 unset) or KFPOS_PAIR9=0"""
    return sc.bank(w, T, storage, pairs=sc.UNSET if pairs else 0, **kw)


def _both_ways(w, T, storage, tr, dts, prepare=None, accel=True, s0=0, n=S, diag=None):
    """{(pairs, run): result}: the four banks of a comparison. prepare(bank) brings a fresh bank to its starting state."""
    out = {}
    for pairs in (False, True):
        for run in ("single calls", "fused"):
            b = _bank(w, T, storage, pairs, chunk=25, diag=diag)
            if prepare:
                prepare(b)
            out[pairs, run] = (sc.single_calls(b, tr, dts, n, s0, accel) if run == "single calls"
                               else sc.fused_split(b, tr, dts, n, s0, accel, split=SPLIT))
            b.close()
    return out


def _check_invisible(out, what):
    sc.same(out[True, "single calls"], out[False, "single calls"], (what, "single calls, pairs against none"))
    sc.same(out[True, "fused"], out[False, "fused"], (what, "fused launches, pairs against none"))
    sc.same(out[True, "fused"], out[True, "single calls"].last(), (what, "pairs: fused against single calls"))


def _full_wavefronts(T):
    return range(T // 64)


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [64, 128, 101])
def test_the_tail_is_invisible_and_every_hand_over_scenario_occurs(T, storage):
    """both meeting points, a survivor that converges in the pair's first pass, a capped tag next to quick ones, absent
    ranges and tags with fewer than four ranges (the trace's epochs 2 and 4: such a tag iterates on what it has)"""
    if not has_gpu():
        pytest.skip("no GPU")
    w = Workload(T, A, seed=_seed())
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    out = _both_ways(w, T, storage, tr, dts)
    st = out[True, "single calls"].status
    g = _gain_iters(st)
    seen = {}
    for wv in _full_wavefronts(T):
        for name, epochs in _scenarios(g[:, 64 * wv:64 * wv + 64]).items():
            seen[name] = seen.get(name, 0) + len(epochs)
    print(f"T={T} storage={storage} seed={_seed()}: wavefront-epochs per scenario: {seen}")
    assert all(seen.values()), seen
    assert (tr.r_host[2, ::7, 1] == -1).all() and (g[2, ::7] > 0).all()      # an absent range: the tag still updates
    # fewer than four ranges: flagged, and the tag still iterates on what it has (next to wave-mates with all eight)
    few = st[4] & capi.ST_FEW_RANGES
    assert few[1::9].all() and not few[0::9].any() and (g[4] > 0).all()
    if T == 101:   # the ragged wavefront iterates too (and never forms pairs: nothing to assert but its bits)
        assert (g[:, 64:] >= 8).any()
    _check_invisible(out, f"T={T} storage={storage}")


@pytest.mark.parametrize("storage", [2, 3])
@pytest.mark.parametrize("T", [64, 128])
def test_a_partly_latched_wavefront_runs_the_per_lane_form_in_pairs(T, storage):
    """ranging-only epochs (MODE_TOA) re-fuse the latched sample of the tags that have one, two of three lanes here: the
    wavefront runs the per-lane form of the pass, and so do its pairs"""
    if not has_gpu():
        pytest.skip("no GPU")
    w = Workload(T, A, seed=_seed())
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    bare = np.arange(T) % 3 == 1

    def prepare(b):
        sc.single_calls(b, tr, dts, 1, poses=False)      # one fused epoch: every tag latches its sample
        x, P, fl = b.get_state()
        assert (fl & sc.FL_HAS_IMU).all()
        fl[bare] &= ~sc.FL_HAS_IMU
        b.set_state(x, P, fl)

    out = _both_ways(w, T, storage, tr, dts, prepare=prepare, accel=False, s0=1, n=S - 1)
    g = _gain_iters(out[True, "single calls"].status)
    formed = sum(len(_scenarios(g[:, 64 * wv:64 * wv + 64])["at most 32 at 8"]) for wv in _full_wavefronts(T))
    print(f"T={T} storage={storage}: {formed} wavefront-epochs handed over at 8")
    assert formed > 0
    fl = out[True, "fused"].flags
    assert not (fl[bare] & sc.FL_HAS_IMU).any() and (fl[~bare] & sc.FL_HAS_IMU).all()
    _check_invisible(out, f"partly latched, T={T} storage={storage}")


@pytest.mark.parametrize("storage", [2, 3])
def test_a_lane_with_a_full_accelerometer_covariance_sends_its_wavefront_to_the_full_form(storage):
    if not has_gpu():
        pytest.skip("no GPU")
    T = 128
    w = Workload(T, A, seed=_seed())
    dts = sc.dts(S)
    cov = w.accel_cov().copy()
    cov[5, 1] = cov[5, 3] = 1e-3          # lane 5 of the first wavefront: an off-diagonal of 1e-3 m^2/s^4
    tr = sc.Trace(w, S, storage, cov=cov, gaps=True)
    out = _both_ways(w, T, storage, tr, dts)
    g = _gain_iters(out[True, "single calls"].status)
    assert len(_scenarios(g[:, :64])["at most 32 at 8"]) > 0 and len(_scenarios(g[:, 64:])["at most 32 at 8"]) > 0
    _check_invisible(out, f"one lane not diagonal, storage={storage}")
    # ... and the full form on every wavefront (KFPOS_IMU9_DIAG=0) computes the same as the default's choice
    forced = _both_ways(w, T, storage, tr, dts, diag=0)
    sc.same(forced[True, "fused"], out[True, "fused"], "pairs: KFPOS_IMU9_DIAG=0 against the default")


@pytest.mark.parametrize("storage", [2, 3])
def test_a_nan_state_among_finite_wave_mates(storage):
    """a tag with a NaN position has a NaN cost and iterates to the cap: it is a survivor at every hand-over. Its bytes
    and everybody else's equal the run without pairs."""
    if not has_gpu():
        pytest.skip("no GPU")
    T, S0, bad = 64, 8, 5
    w = Workload(T, A, seed=_seed())
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)

    def prepare(b):
        sc.fused(b, tr, dts, S0)      # past the fixed start: the information form runs
        x, P, fl = b.get_state()
        x[bad, :3] = np.nan
        b.set_state(x, P, fl)

    out = _both_ways(w, T, storage, tr, dts, prepare=prepare, s0=S0, n=S - S0)
    single = out[True, "single calls"]
    g = _gain_iters(single.status)
    assert (single.status[:, bad] & capi.ST_NONFINITE).all() and np.isnan(single.poses[:, :, bad]).all()
    others = np.arange(T) != bad
    assert np.isfinite(single.poses[:, :, others]).all()
    handed = [s for s in range(S - S0) if (g[s] > 0).all() and (g[s] >= 8).sum() <= 32 and g[s, bad] == 20]
    print(f"storage={storage}: {len(handed)} epochs in which the NaN tag went through a hand-over at 8")
    assert handed
    _check_invisible(out, f"NaN wave-mate, storage={storage}")


@pytest.mark.parametrize("storage", [2, 3])
def test_the_tail_matches_the_oracle(storage):
    """the tolerances of tests/test_gpu_parity.py: mixed storage <= 1e-9 m RMS and <= 1e-8 m at worst over the poses of
    every epoch, with equal status words; p48 <= 1e-7 m / 1e-6 m with equal flags (iteration counts may differ by one
    where a stop decision sits on its threshold)"""
    if not has_gpu():
        pytest.skip("no GPU")
    T = 128
    w = Workload(T, A, seed=_seed())
    dts = sc.dts(S)
    tr = sc.Trace(w, S, storage, gaps=True)
    b = _bank(w, T, storage, True)
    got = sc.single_calls(b, tr, dts, S)
    b.close()
    poses, theirs = sc.oracle_run(w, tr.r_host, w.err_est(), dts, real=np.float32, init=w.init_positions())[:2]
    d = np.sqrt(((got.poses - poses.transpose(0, 2, 1)) ** 2).sum(1))
    rms, mx = float(np.sqrt((d ** 2).mean())), float(d.max())
    print(f"storage={storage}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {S} epochs")
    mine = got.status.astype(np.uint32)
    if storage == 2:
        assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
        assert np.array_equal(mine, theirs)
    else:
        assert rms <= 1e-7 and mx <= 1e-6, (rms, mx)
        assert np.array_equal(capi.st_flags(mine), capi.st_flags(theirs))
