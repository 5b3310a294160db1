"""Where the lanes of a 9-state wavefront meet to hand the tail of the gain iteration to pairs (KFPOS_PAIR9_MEET =
first,dense_until, read at kfpos_create: iekf9_next_meet) changes no byte: the default (8,10), 7,10, the old schedule 8,8, a
meeting after every solve (1,20) and no pairs at all (KFPOS_PAIR9=0) leave the same pose of every epoch, state, covariance,
flags, status words and latch, compared as BIT PATTERNS.

Each setting runs in a fresh child process (tests/pairs9_meet_cases.py as a program: the five start together, once for
the module) that replays the trace for every shape: T = 64 (one wavefront), 128 (two), 101 (a full wavefront and a ragged
one, which never forms pairs), 8 anchors, storage 2 = mixed and 3 = p48; the 12 epochs as one launch, as 5 + 7, and as
single calls, whose status words carry every epoch's solve counts.

The six ways a wavefront can meet (pairs9_meet_cases.scenarios) are asserted on the kernel's own status words before
anything is compared; the seed is chosen with the oracle on the CPU so that the first wavefront shows all six, and a
scenario that does not occur in the kernel's run is a failure. Measured on MI355X, seed 22: the first wavefront's epochs
0-3 find nobody at 7, 4-7 at most 32 lanes by 6, epoch 8 hands over first at 7, epoch 10 at 8, epoch 9 at 9 or 10, and
epoch 11 keeps more than 32 lanes beyond 11."""
import functools
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

import pairs9_meet_cases as pm
import step_checks as sc
from conftest import has_gpu
from roskfpos_amd import capi
from roskfpos_amd.capi import ST_FEW_RANGES, ST_NONFINITE

pytestmark = pytest.mark.gpu

CHILD_LIMIT = 240   # seconds for the five children together; they take about ten


@functools.lru_cache(maxsize=None)
def _results():
    """{setting: {name: array}}: one child process per setting, all started at once"""
    sd = pm.seed()
    script = os.path.abspath(pm.__file__)
    with tempfile.TemporaryDirectory(prefix="kfpos_meet_") as tmp:
        procs = {}
        for k, (name, extra) in enumerate(pm.SETTINGS.items()):
            env = {key: v for key, v in os.environ.items() if key not in ("KFPOS_PAIR9_MEET", "KFPOS_PAIR9")}
            env.update(extra)
            out = os.path.join(tmp, f"{k}.npz")
            procs[name] = (subprocess.Popen([sys.executable, script, out, str(sd)], env=env, stdout=subprocess.PIPE,
                                            stderr=subprocess.STDOUT, text=True), out)
        res = {}
        try:
            for name, (p, out) in procs.items():
                text, _ = p.communicate(timeout=CHILD_LIMIT)
                assert p.returncode == 0, (name, p.returncode, text[-2000:])
                with np.load(out) as z:
                    res[name] = {key: z[key] for key in z.files}
        finally:
            for p, _ in procs.values():
                if p.poll() is None:
                    p.kill()
        return res


def _run(setting, T, storage, run):
    res = _results()[setting]
    return sc.Run(*(res[f"{T}/{storage}/{run}/{part}"] for part in sc.Run._fields))


def _same_bytes(T, storage, run):
    for setting in pm.SETTINGS:
        sc.same(_run(setting, T, storage, run), _run("no pairs", T, storage, run), (setting, T, storage, run))


@pytest.mark.parametrize("T,storage", pm.SHAPES)
def test_every_schedule_leaves_the_same_bytes_and_every_meeting_scenario_occurs(T, storage):
    if not has_gpu():
        pytest.skip("no GPU")
    res = _results()
    assert int(res["default"]["seed"]) == pm.seed()
    st = res["default"][f"{T}/{storage}/single calls/status"]
    g = pm.gain_iters(st)
    seen = {name: 0 for name in pm.SCENARIOS}
    for wv in range(T // 64):
        for name, epochs in pm.scenarios(g[:, 64 * wv:64 * wv + 64]).items():
            seen[name] += len(epochs)
    print(f"T={T} storage={storage} seed={pm.seed()}: wavefront-epochs per scenario: {seen}")
    assert all(seen.values()), seen
    # fewer than four ranges (the trace's epoch 4, every ninth tag from the second): flagged, iterating on what it has
    # next to wave-mates with all eight, in an epoch whose first wavefront hands over at the first meeting
    assert (st[4, 1::9] & ST_FEW_RANGES).all() and not (st[4, 0::9] & ST_FEW_RANGES).any() and (g[4] > 0).all()
    assert 4 in pm.scenarios(g[:, :64])["at most 32 by 6"]
    if T == 101:   # the ragged wavefront iterates too (and never forms pairs: nothing to assert but its bits)
        assert (g[:, 64:] >= 7).any()
    for run in ("one launch", "5 + 7", "single calls"):
        _same_bytes(T, storage, run)
    # ... and the three ways of running the epochs agree with each other (status: a launch reports its last epoch's)
    one = _run("default", T, storage, "one launch")
    sc.same(one, _run("default", T, storage, "5 + 7"), "one launch against 5 + 7")
    sc.same(one, _run("default", T, storage, "single calls").last(), "one launch against single calls")


@pytest.mark.parametrize("storage", [2, 3])
def test_a_nan_wave_mate_changes_nobodys_bytes(storage):
    """a tag whose position is NaN has a NaN cost and iterates to the cap: it is among the lanes every meeting finds. Its
    bytes and everybody else's are the same under every schedule and without pairs."""
    if not has_gpu():
        pytest.skip("no GPU")
    T, bad = pm.NAN_T, pm.NAN_TAG
    res = _results()["default"]
    st = res[f"{T}/{storage}/nan, single calls/status"]
    poses = res[f"{T}/{storage}/nan, single calls/poses"]
    g = pm.gain_iters(st)
    others = np.arange(T) != bad
    assert (st[:, bad] & ST_NONFINITE).all() and np.isnan(poses[:, :, bad]).all() and (g[:, bad] == 20).all()
    assert np.isfinite(poses[:, :, others]).all()
    met = pm.scenarios(g)
    handed = sum(len(met[k]) for k in ("first at 7", "first at 8", "first at 9 or 10", "at most 32 by 6"))
    print(f"storage={storage}: the NaN tag went through {handed} hand-overs; {({k: len(v) for k, v in met.items()})}")
    assert handed >= 1
    for run in ("nan, one launch", "nan, single calls"):
        _same_bytes(T, storage, run)


@pytest.mark.parametrize("storage", [2, 3])
def test_the_default_schedule_matches_the_oracle(storage):
    """the tolerances of tests/test_gpu_parity.py: mixed storage <= 1e-9 m RMS and <= 1e-8 m at worst over the poses of
    every epoch, with equal status words; p48 <= 1e-7 m / 1e-6 m with equal flags (iteration counts may differ by one
    where a stop decision sits on its threshold)"""
    if not has_gpu():
        pytest.skip("no GPU")
    T = 128
    res = _results()["default"]
    poses, mine = res[f"{T}/{storage}/single calls/poses"], res[f"{T}/{storage}/single calls/status"].astype(np.uint32)
    want, theirs = pm.oracle_run(T, pm.seed())
    d = np.sqrt(((poses - want) ** 2).sum(1))
    rms, mx = float(np.sqrt((d ** 2).mean())), float(d.max())
    print(f"storage={storage}: RMS {rms:.3e} m, max {mx:.3e} m against the oracle over {pm.S} epochs")
    if storage == 2:
        assert rms <= 1e-9 and mx <= 1e-8, (rms, mx)
        assert np.array_equal(mine, theirs)
    else:
        assert rms <= 1e-7 and mx <= 1e-6, (rms, mx)
        assert np.array_equal(capi.st_flags(mine), capi.st_flags(theirs))
