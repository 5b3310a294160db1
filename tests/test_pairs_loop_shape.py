"""tools/pairs_loop_shape.py, the build rule that keeps a trip of the PAIRS' loop of the 9-state gain iteration down to
arithmetic: it holds for the library as built, and on hand-written disassembly fragments it passes a clean pair loop and
fires once for each of its rules -- an LDS read in the trip, a vector-memory access, a wait for memory, one branch too
many, no loop of the fast form. (CPU only: the rule reads text.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import pairs_loop_shape as pls  # noqa: E402
from test_trip_loop_shape import KERNEL, PER_LANE, fragment  # noqa: E402  (the same synthetic kernel, with an exchange)

DPP = "v_mov_b32_dpp v5, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"


def pair_fragment(in_trip=(), **kw):
    """the trip loop of test_trip_loop_shape.fragment with the exchange of a pair in its sweep; a pair's solve is the
    per-lane one, its sweep half of it: 160 + 220 fp64 instructions"""
    kw.setdefault("solve", 220)
    return fragment(in_trip=(DPP, DPP) + tuple(in_trip), **kw)


def _check(text, **kw):
    report = []
    return pls.check(text, kernels=KERNEL, report=report, **kw), report


def test_the_rule_holds_for_the_library_as_built():
    if not os.path.exists(os.path.join(CSRC, "libkfpos_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pairs_loop_shape.py"),
                          os.path.join(CSRC, "libkfpos_hip.so")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    # both headline kernels, each with the fast and the per-lane form of the pairs' loop
    loops = [l for l in res.stdout.splitlines() if " blocks, " in l]
    assert len(loops) == 4 and sum("IdfLi8ELb1E" in l for l in loops) == 2, res.stdout
    assert sum("(fast form)" in l for l in loops) == 2 and sum("(per-lane form)" in l for l in loops) == 2, res.stdout
    assert all(" ds 0, vmem 0, mem_waits 0," in l for l in loops), res.stdout
    paths = [l for l in res.stdout.splitlines() if "usual path" in l]
    assert len(paths) == 4 and sum(" branches 4," in l for l in paths) == 2, res.stdout


def test_a_pair_trip_of_arithmetic_and_four_branches_passes():
    problems, report = _check(pair_fragment())
    assert problems == [], problems
    assert len(report) == 2 and "(fast form)" in report[0] and "fp64 382" in report[0] and "branches 4" in report[0], report
    assert "usual path" in report[1] and "fp64 380" in report[1] and "branches 4" in report[1], report


def test_an_lds_read_in_the_pair_trip_fails():
    problems, _ = _check(pair_fragment(in_trip=("ds_read2st64_b64 v[198:201], v240 offset1:2",)))
    assert len(problems) == 1 and "ds_read2st64_b64" in problems[0] and "a pair trip reads or writes memory" in problems[0]


def test_a_vector_memory_access_in_the_pair_trip_fails():
    problems, _ = _check(pair_fragment(in_trip=("global_load_dwordx2 v[14:15], v2, s[0:1]",)))
    assert len(problems) == 1 and "global_load_dwordx2" in problems[0], problems


def test_a_wait_for_memory_in_the_pair_trip_fails():
    for wait in ("s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(0) lgkmcnt(1)"):
        problems, _ = _check(pair_fragment(in_trip=(wait,)))
        assert len(problems) == 1 and "a pair trip waits for memory" in problems[0], (wait, problems)
    assert _check(pair_fragment(in_trip=("s_waitcnt expcnt(0)", "s_nop 1")))[0] == []   # (not a wait for memory)


def test_a_fifth_branch_fails():
    problems, _ = _check(pair_fragment(extra_branches=1))
    assert len(problems) == 1 and "5 branch instructions on the usual path of a pair trip" in problems[0], problems
    assert "maximum 4" in problems[0]


def test_the_per_lane_form_may_branch_once_more_but_a_fast_form_must_exist():
    problems, report = _check(pair_fragment(in_trip=PER_LANE))
    assert "(per-lane form)" in report[0] and "saveexec 2" in report[0] and "branches 5" in report[1], report
    assert len(problems) == 1 and "no fast form" in problems[0], problems
    problems, _ = _check(pair_fragment(in_trip=PER_LANE, extra_branches=1))
    assert len(problems) == 2 and "6 branch instructions" in problems[1] and "maximum 5" in problems[1], problems


def test_only_loops_with_an_exchange_are_pairs_loops():
    # the one-tag-per-lane trip loop is none of this rule's business, whatever it holds; without any pairs' loop the
    # rule says so
    problems, report = _check(fragment(in_trip=("ds_read_b64 v[198:199], v240",)))
    assert report == [] and len(problems) == 1 and "where are the pairs" in problems[0], problems
    assert pls.check(pair_fragment(), kernels=(r"k_step_imu9I\w*p48\w*fLi8ELb1E",)) != []   # no kernel of that name
