"""BatchedRangingNode::setDeltaRanges (kfpos_ingest.h): whole-bank ranging rounds assembled as int16 codes
(KFPOS_SLOT_RANGES_D16) compute what rounds with int32 ranges do.

The checks live in a C++ driver, tests/d16/ingest_d16_driver.cpp, built here with g++ against libkfpos_hip.so the way
roskfpos_amd/csrc/Makefile builds kfpos_replay (into tmp_path; nothing built is kept). One seeded message stream --
asynchronous tags, a tag that stays silent for twenty epochs, ranges that jump by 40 m for an epoch, epochs without a
poll() so that calls wait in the overflow arena, IMU samples for the 9-state bank, a bindRows admission of a third of the
bank in the middle and rows that change hands -- feeds a node in each mode. After every poll() both banks hold the same
bytes; the status words delivered to the sink for every estimator call are the same sequence."""
import os
import subprocess

import pytest

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "d16", "ingest_d16_driver.cpp")


def _driver(tmp_path):
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exe = str(tmp_path / "ingest_d16_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", exe, SRC,
                    "-L", CSRC, "-lkfpos_hip", "-Wl,-rpath," + CSRC], check=True)
    return exe


def test_driver_builds_and_the_ingest_has_the_switch(tmp_path):
    """no GPU: the header compiles with the D16 entry points, and the driver explains itself"""
    out = subprocess.run([_driver(tmp_path)], capture_output=True, text=True)
    assert out.returncode == 1 and "usage" in out.stdout
    text = open(os.path.join(CSRC, "kfpos_ingest.h")).read()
    assert "void setDeltaRanges(bool on)" in text and "bool delta_ = false" in text  # opt-in


@pytest.mark.gpu
@pytest.mark.parametrize("model,seed", [("toa6", 1), ("imu9", 1), ("imu9", 7)])
def test_delta_rounds_equal_int32_rounds(tmp_path, model, seed):
    out = subprocess.run([_driver(tmp_path), model, str(seed)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr
