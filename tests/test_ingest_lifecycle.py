"""Rows of a BatchedRangingNode become reusable (kfpos_ingest.h: releaseRows / bindRows / rowOf, FlatIdMap::erase).

The checks live in a small C++ driver, tests/lifecycle/lifecycle_driver.cpp, built here with g++ against
libkfpos_hip.so the way roskfpos_amd/csrc/Makefile builds kfpos_replay (into tmp_path; nothing built is kept):
  idmap  FlatIdMap with erase against std::map over a seeded random sequence of build / erase / insert / find,
         ids that collide and re-insertion of erased ids included (no GPU)
  node   a node with 6 rows: tags a-d stream 40 epochs; b's row is released and bound to a new tag e, which must come
         out bit for bit like e on a fresh handle that had it from the start; the other rows like a run in which nothing
         was released; both calls throw std::logic_error while a call is pending (GPU)
"""
import os
import subprocess

import pytest

from roskfpos_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "lifecycle", "lifecycle_driver.cpp")


def _driver(tmp_path):
    if not os.path.exists(capi.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    exe = str(tmp_path / "lifecycle_driver")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", exe, SRC,
                    "-L", CSRC, "-lkfpos_hip", "-Wl,-rpath," + CSRC], check=True)
    return exe


def _run(exe, *args):
    out = subprocess.run([exe, *args], capture_output=True, text=True)
    print(out.stdout)
    assert out.returncode == 0 and out.stdout.strip().endswith("OK"), out.stdout + out.stderr


@pytest.mark.parametrize("seed", [1, 2, 20240])
def test_flat_id_map_with_erase_agrees_with_std_map(tmp_path, seed):
    _run(_driver(tmp_path), "idmap", str(seed))


@pytest.mark.gpu
def test_released_row_serves_a_new_tag_like_a_fresh_handle(tmp_path):
    _run(_driver(tmp_path), "node")
