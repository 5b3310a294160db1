"""roskfpos_amd/csrc/kfpos_replay_plan.h: how a replay entry point cuts a schedule into launches, and how `kinds` travels in
a kernel-argument block (one bit per event for the 9-state kernels, four for the planar ones).

The checks live in a C++ driver, tests/replay/plan_driver.cpp, built here with g++ and the address and undefined-behaviour
sanitizers (into tmp_path; nothing built is kept): the header includes no HIP header, so no GPU, no library and no Python
extension is involved. Cut: for every n_events in 0..300, launches of 1, 7, 64, 127 and 128 events, 2 and 5 kinds, seeded
schedules (all ranging, no ranging, the first other event at 0, 1 and n_events - 1 among them) the launches tile
[first, n_events) in order, none is longer than the chunk, and every per-kind ordinal equals a brute-force count plus the
lead for ranging. Formats: for every n in 1..128 decode(pack(kinds), k) == kinds[k] below n and every bit beyond n is 0."""
import os
import subprocess

import numpy as np
import pytest

import planar_events

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "replay", "plan_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("replay_plan") / "plan_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def test_the_header_stands_alone():
    text = open(os.path.join(CSRC, "kfpos_replay_plan.h")).read()
    assert "#include <hip" not in text and '#include "' not in text


def test_cut_and_formats(driver):
    out = subprocess.run([driver], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "OK", out.stdout[-3000:] + out.stderr[-3000:]


@pytest.mark.parametrize("chunk", [1, 7, 64, 128])
def test_launches_start_where_the_planar_tests_expect_them(driver, chunk):
    """planar_events.launch_starts is what the GPU tests of the planar schedules assert their boundaries with"""
    for end_on_sensor in (True, False):
        for waiting in (False, True):
            kinds = planar_events.kinds_of(end_on_sensor, waiting)
            for reps in (1, 4):   # 4: longer than one launch of 128 events
                k = np.tile(kinds, reps)
                out = subprocess.run([driver, "starts", str(chunk), "5", "".join(str(int(v)) for v in k)],
                                     capture_output=True, text=True, check=True)
                assert [int(v) for v in out.stdout.split()] == planar_events.launch_starts(k, chunk)
