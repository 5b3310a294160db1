"""roskfpos_amd/csrc/kfpos_host_layout.h: the byte layouts of the small bank's mapped block, of a streaming slot and of the
row-list block -- offsets the copy stream runs ahead of the compute stream on.

The checks live in a C++ driver, tests/layout/layout_driver.cpp, built here with g++ and the address and
undefined-behaviour sanitizers (into tmp_path; nothing built is kept): the header includes no HIP header, so no GPU, no
library and no Python extension is involved. For n_tags in {1, 63, 64, 65, 4096}, max_anchors in {1, 8, 16, 64}, 4- and
8-byte measurements, every state dimension with its covariance sizes and, for the row-list block, lists of 1, cap / 2 and cap
tags: every region starts on a 256-byte boundary, no two overlap, each ends inside the total; a slot keeps ranges | err |
accel | cov | dt and status | pos as neighbours in this order; the KFPOS_N_SLOTS input areas of the row-list block overlap
neither each other nor the work bank."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "layout", "layout_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    slots = re.search(r"#define KFPOS_N_SLOTS (\d+)", open(os.path.join(CSRC, "kfpos_internal.h")).read()).group(1)
    exe = str(tmp_path_factory.mktemp("host_layout") / "layout_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    f"-DKFPOS_N_SLOTS={slots}", "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def test_the_header_stands_alone():
    text = open(os.path.join(CSRC, "kfpos_host_layout.h")).read()
    assert "#include <hip" not in text and '#include "' not in text


def test_regions_are_aligned_disjoint_and_inside(driver):
    out = subprocess.run([driver], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout[-3000:] + out.stderr[-3000:]
    assert int(out.stdout.split()[1]) == 5 * 4 * (3 + 1) * 5  # every configuration ran


def test_one_region_bump():
    """the 256-byte bump exists once: no other host unit rounds a region up on its own"""
    for name in ("kfpos_hip.hip", "kfpos_hip_state.hip", "kfpos_hip_slots.hip", "kfpos_hip_replay.hip"):
        assert "auto region" not in open(os.path.join(CSRC, name)).read(), name
