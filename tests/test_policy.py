"""roskfpos_amd/csrc/kfpos_policy.h: what kfpos_create refuses and what it decides from the configuration, the device's
wavefront slots and the KFPOS_* environment -- the one place that says it; and roskfpos_amd/csrc/kfpos_owned.h: the owner
of everything the handle and the communicator free.

The checks live in a C++ driver, tests/policy/policy_driver.cpp, built here with g++ and the address and
undefined-behaviour sanitizers (into tmp_path; nothing built is kept): neither header includes a HIP header, so no GPU, no
library and no Python extension is involved. The sweep: four models x four storage modes x max_anchors in {7, 8, 9, 16} x
fixed / ML start x leave-one-out x top-N x ml_variant x wavefront slots S in {0, 4, 1024} x n_tags in {1, 8192, 8193, 64 S,
64 S + 1} x (each of the nine variables unset, empty, 0, 1 with the others unset, then all at once): every field of Policy
equals a table written out in the driver in the words of kfpos_create's rules, every variable is read once, and every
accepted combination is producible() -- the filter tests/launch/launch_driver.cpp sweeps by."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "policy", "policy_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("policy") / "policy_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", CSRC, "-o", exe, SRC], check=True)

    def run(section):
        out = subprocess.run([exe, section], capture_output=True, text=True)
        assert out.returncode == 0 and out.stdout.startswith("OK " + section), out.stdout[-3000:] + out.stderr[-3000:]
        return [int(w) for w in out.stdout.split()[2:]]
    return run


def _own_includes(name):
    text = open(os.path.join(CSRC, name)).read()
    assert "#include <hip" not in text and "hipError_t" not in text, name
    return [ln for ln in text.splitlines() if ln.startswith('#include "')]


def test_the_headers_stand_alone():
    assert _own_includes("kfpos_policy.h") == ['#include "../../include/kfpos.h"', '#include "kfpos_launch_plan.h"']
    assert _own_includes("kfpos_owned.h") == []


def test_every_policy_matches_the_rules_in_words(driver):
    accepted, calls = driver("sweep")
    # per storage mode and anchor count: 6-state start x leave-one-out x top-N = 8, 9-state and planar start = 2 each, the ML
    # estimator start x top-N x its three variants = 12; slots and tags: S = 0 has n_tags = 0 refused, 4 + 5 + 5 = 14
    assert accepted == 4 * 4 * (8 + 2 + 12 + 2) * 14
    assert calls == accepted * (1 + 9 * 3 + 3)  # all unset; each variable empty, 0, 1; all of them empty, 0, 1


def test_pair9_meet_as_sscanf_reads_it(driver):
    assert driver("meet") == [12]


def test_trace_chunk_steps_is_clamped(driver):
    assert driver("chunk") == [6]


def test_a_refusal_per_rule_and_the_earlier_of_two(driver):
    assert driver("refusal") == [12]


def test_an_owner_releases_what_it_holds_once(driver):
    assert driver("owned") == [9]


def test_the_environment_is_read_in_one_place():
    """kfpos_create hands getenv to the policy; no other function of the handle's units reads a variable, nothing but the
    owners' aliases frees, and kfpos_create has one failure exit"""
    units = ("kfpos_hip.hip", "kfpos_hip_state.hip", "kfpos_hip_slots.hip", "kfpos_hip_replay.hip")
    text = {n: open(os.path.join(CSRC, n)).read() for n in units + ("kfpos_comm.hip", "kfpos_host.h")}
    assert sum(text[n].count("getenv(") for n in units) == 1 and text["kfpos_hip.hip"].count("getenv(") == 1
    for n, t in text.items():
        for call in ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy("):
            assert call not in t, (n, call)
    create = text["kfpos_hip.hip"].split("int kfpos_create(")[1].split("\nint kfpos_destroy(")[0]
    assert create.count("kfpos_destroy(h);") == 1
