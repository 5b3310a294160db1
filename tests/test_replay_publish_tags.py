"""kfpos_replay in batched mode with publishTags:=<hex,...>: a P tick asks the GPU for the named tags' rows only
(BatchedRangingNode::getPoseRows -> kfpos_get_pose_rows) and prints, character for character, the lines the run without
the parameter prints for those tags. The three-tag trace of tests/test_ingest_batched.py, 40 epochs of it."""
import os
import subprocess

import pytest

from roskfpos_amd.synth import Workload

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "roskfpos_amd", "csrc", "kfpos_replay")
A = 8
TAGS = [0x10, 0x2A, 0x3]
N_EPOCHS = 40


def _trace(path):
    """Interleaved tags, an anchor that drops out now and then, a tag that misses two epochs (its 50 ms timer fires), an
    errorEstimation of 0 on a same-sequence message; a P line every five epochs, the first one before tag 0x3 started."""
    w = Workload(len(TAGS), A)
    ev = [(10.0 - 0.001, f"P {10.0 - 0.001:.9f}")]
    for k in range(N_EPOCHS):
        t0 = 10.0 + 0.05 * k
        r = w.ranges_mm(k)
        for ti, tag in enumerate(TAGS):
            if tag == TAGS[1] and k in (20, 21):
                continue
            if tag == TAGS[2] and k < 3:
                continue
            for a in range(A):
                if a == 1 and k % 7 == 3:
                    continue
                err = 0.0 if (tag == TAGS[0] and a == 3 and k % 5 == 2) else 0.0025
                t = t0 + 0.0007 * a + 0.0001 * ti
                ev.append((t, f"R {t:.9f} {100 + a} {tag} {float(r[ti, a]) + 0.6:.3f} {k % 256} {err:.17g}"))
        if k % 5 == 2:
            ev.append((t0 + 0.03, f"P {t0 + 0.03:.9f}"))
    ev.sort(key=lambda e: e[0])
    lines = [f"A {100 + a} {x:.17g} {y:.17g} {z:.17g}" for a, (x, y, z) in enumerate(w.anchors)]
    open(path, "w").write("\n".join(lines + [e[1] for e in ev]) + "\n")
    p0 = w.init_positions()[0]
    return ["algorithm:=ALGORITHM_KF_TOA", "useStartPosition:=0", f"initPositionX:={p0[0]:.17g}",
            f"initPositionY:={p0[1]:.17g}", f"initPositionZ:={p0[2]:.17g}", "tagIds:=" + ",".join(f"{t:x}" for t in TAGS)]


def _run(args):
    return subprocess.run([REPLAY] + args, capture_output=True, text=True)


def test_publish_tags_prints_the_same_lines_for_the_named_tags(tmp_path):
    trace = str(tmp_path / "multi.txt")
    params = _trace(trace)
    full = _run(params + [trace])
    assert full.returncode == 0, full.stderr
    all_lines = full.stdout.splitlines()
    ticks = 1 + len([k for k in range(N_EPOCHS) if k % 5 == 2])
    assert len(all_lines) == ticks * len(TAGS)
    assert any(ln.split()[3] == "0" for ln in all_lines) and any(ln.split()[3] == "1" for ln in all_lines)
    for subset in (["2a"], ["3", "10"]):
        part = _run(params + ["publishTags:=" + ",".join(subset), trace])
        assert part.returncode == 0, part.stderr
        # per tick the named tags in the order given; per tag the lines of the full run in time order
        for tag in subset:
            want = [ln for ln in all_lines if ln.split()[2] == tag]
            got = [ln for ln in part.stdout.splitlines() if ln.split()[2] == tag]
            assert len(want) == ticks and got == want, tag
        assert len(part.stdout.splitlines()) == ticks * len(subset)


def test_an_unknown_publish_tag_is_an_error(tmp_path):
    trace = str(tmp_path / "multi.txt")
    params = _trace(trace)
    res = _run(params + ["publishTags:=2a,77", trace])
    assert res.returncode == 1
    assert "publishTags" in res.stderr and "77" in res.stderr
    assert res.stdout == ""
