"""roskfpos_amd/csrc/kfpos_state_record.h: the one place that writes down where the components of a tag's record -- x | P |
latch | height, the formats of kfpos_get_state / kfpos_get_latch / kfpos_get_height -- live in the bank's component-major
arrays. The per-tag kernels are handed its tables, the whole-bank accessors walk them on the CPU.

The checks live in a C++ driver, tests/record/record_driver.cpp, built here with g++ and the address and
undefined-behaviour sanitizers (into tmp_path; nothing built is kept): the header includes no HIP header, so no GPU, no
library and no Python extension is involved. For the ML estimator, the 6-state filter (packed and full covariance), the
9-state and the planar filter, (covariance, measurement) element sizes (8, 8), (4, 4), (8, 4), (6, 4) and 1, 3 and 65 tags:
the walkers against the formats include/kfpos.h documents, worked out independently in the driver; asymmetric records in
(packed P takes j >= i, the latch covariance i >= j, nothing else is written); the record table against the fresh table."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "record", "record_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("state_record") / "record_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def test_the_header_stands_alone():
    text = open(os.path.join(CSRC, "kfpos_state_record.h")).read()
    assert "#include <hip" not in text
    assert set(re.findall(r'#include "([^"]+)"', text)) <= {"kfpos_host_layout.h", "kfpos_p48.h"}


def test_the_record_of_every_model_in_every_storage(driver):
    out = subprocess.run([driver], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout[-3000:] + out.stderr[-3000:]
    assert int(out.stdout.split()[1]) == 5 * 4 * 3  # models x element sizes x bank sizes: every configuration ran
