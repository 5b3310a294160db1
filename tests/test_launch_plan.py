"""roskfpos_amd/csrc/kfpos_launch_plan.h: which kernel form a handle runs for a launch, over how many workgroups, with how
many bytes of dynamic LDS -- the one place that decides it.

The checks live in a C++ driver, tests/launch/launch_driver.cpp, built here with g++ and the address and
undefined-behaviour sanitizers (into tmp_path; nothing built is kept): the header includes no HIP header, so no GPU, no
library and no Python extension is involved. Four models x four storage modes x max_anchors in {1, 7, 8, 9, 16, 17, 30, 31,
42, 43, 64} x fixed / ML start x leave-one-out x top-N x force_generic x two_waves x coop x planar_sensors x every kind of
launch, less what kfpos_create refuses or never produces: selector arguments, epoch and park doubles equal a table written
out in the driver per kernel form; the park starts where the epoch ends; no plan exceeds a CU's 160 KB; the plans over 64 KB
are exactly the run-time-loop forms from 17 (9-state), 31 (a 36-per-lane park behind the epoch) and 43 anchors on."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "launch", "launch_driver.cpp")
HOST_UNITS = ("kfpos_hip.hip", "kfpos_hip_state.hip", "kfpos_hip_slots.hip", "kfpos_hip_replay.hip")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def test_the_header_stands_alone():
    text = open(os.path.join(CSRC, "kfpos_launch_plan.h")).read()
    assert "#include <hip" not in text
    assert [ln for ln in text.splitlines() if ln.startswith('#include "')] == ['#include "../../include/kfpos.h"']


def test_every_plan_matches_what_the_kernels_address(driver):
    out = subprocess.run([driver], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout[-3000:] + out.stderr[-3000:]
    # per storage mode and anchor count, (configurations kfpos_create can produce) x (launches they can make).
    # 6-state without coop: start x leave-one-out x top-N x force_generic x two_waves = 32 (the 48-bit covariance: 28, its ML
    # start with leave-one-out exists as force_generic only), step and per-tag trace; with coop, up to 8 anchors: two_waves
    # = 2, step only. 9-state: force_generic x two_waves = 4, step, IMU-only step, event replay. ML estimator: top-N x
    # force_generic x two_waves = 8, step. Planar: force_generic x two_waves x planar_sensors = 8, step, sensor call, replay.
    toa = 3 * (11 * 32 * 2 + 3 * 2) + (11 * 28 * 2 + 3 * 2)
    assert int(out.stdout.split()[1]) == toa + 4 * 11 * (4 * 3 + 8 + 8 * 3)


def test_one_place_computes_lds_bytes():
    """no host unit multiplies lanes into an LDS size any more"""
    for name in HOST_UNITS:
        assert "* WAVE * sizeof(double)" not in open(os.path.join(CSRC, name)).read(), name
