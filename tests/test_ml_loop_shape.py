"""tools/ml_loop_shape.py, the build rule that keeps a pass of the Gauss-Newton seed loop (ml_estimate's peeled loop) of
the 9-state bench kernels down to arithmetic: it holds for the library as built, and on hand-written disassembly
fragments it passes a clean loop and fires once for each of its rules -- an LDS read in the pass, a vector-memory access,
a wait for memory, one branch too many, a loop that went missing. (CPU only: the rule reads text.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ml_loop_shape as mls  # noqa: E402
from test_trip_loop_shape import KERNEL, PER_LANE, fragment  # noqa: E402  (the same synthetic kernel, a smaller loop)

DPP = "v_mov_b32_dpp v5, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"


def ml_fragment(**kw):
    """the loop of test_trip_loop_shape.fragment at the size of a Gauss-Newton pass: 160 fp64 instructions of sweep, the
    vote around the cold block with the division, the skip of the step, 180 of step = 4 branches a pass"""
    kw.setdefault("solve", 180)
    return fragment(**kw)


def _check(text, copies=1, **kw):
    report = []
    return mls.check(text, kernels=KERNEL, copies=copies, report=report, **kw), report


def test_the_rule_holds_for_the_library_as_built():
    if not os.path.exists(os.path.join(CSRC, "libkfpos_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ml_loop_shape.py"),
                          os.path.join(CSRC, "libkfpos_hip.so")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    # both headline kernels, each with the ML start's loop and the loop that seeds every step
    loops = [l for l in res.stdout.splitlines() if " blocks, " in l]
    assert len(loops) == 4 and sum("IdfLi8ELb1E" in l for l in loops) == 2, res.stdout
    assert all(" ds 0, vmem 0, mem_waits 0," in l for l in loops), res.stdout
    paths = [l for l in res.stdout.splitlines() if "usual path" in l]
    assert len(paths) == 4 and all(" branches 4," in l for l in paths), res.stdout


def test_a_pass_of_arithmetic_and_four_branches_passes():
    problems, report = _check(ml_fragment())
    assert problems == [], problems
    assert len(report) == 2 and "fp64 342" in report[0] and "branches 4" in report[0], report
    assert "usual path" in report[1] and "fp64 340" in report[1] and "branches 4" in report[1], report


def test_a_memory_access_in_the_pass_fails():
    problems, _ = _check(ml_fragment(in_trip=("ds_read_b64 v[198:199], v240 offset:39424",)))
    assert len(problems) == 1 and "ds_read_b64" in problems[0] and "a pass reads or writes memory" in problems[0], problems
    problems, _ = _check(ml_fragment(in_trip=("global_load_dwordx2 v[14:15], v2, s[0:1]",)))
    assert len(problems) == 1 and "global_load_dwordx2" in problems[0], problems


def test_a_wait_for_memory_in_the_pass_fails():
    for wait in ("s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(0) lgkmcnt(1)"):
        problems, _ = _check(ml_fragment(in_trip=(wait,)))
        assert len(problems) == 1 and "a pass waits for memory" in problems[0], (wait, problems)
    assert _check(ml_fragment(in_trip=("s_waitcnt expcnt(0)", "s_nop 1")))[0] == []   # (not a wait for memory)


def test_a_fifth_branch_fails():
    """the unpeeled loop: the first-pass test and the masked region of `iter > 0` are branches of every pass"""
    problems, _ = _check(ml_fragment(extra_branches=1))
    assert len(problems) == 1 and "5 branch instructions on the usual path of a pass" in problems[0], problems
    assert "maximum 4" in problems[0]
    problems, _ = _check(ml_fragment(in_trip=PER_LANE, extra_branches=1))
    assert len(problems) == 1 and "6 branch instructions" in problems[0], problems
    assert _check(ml_fragment(extra_branches=1), max_branches=5)[0] == []


def test_the_loops_of_the_gain_iteration_are_not_this_rules_business_and_a_missing_loop_is_an_error():
    # a trip loop of the gain iteration (460 fp64) and a pairs' loop (an exchange), whatever they hold: not looked at,
    # and then the Gauss-Newton loop is missing
    for text in (fragment(in_trip=("ds_read_b64 v[198:199], v240",)), ml_fragment(in_trip=("s_waitcnt lgkmcnt(0)", DPP))):
        problems, report = _check(text)
        assert report == [] and len(problems) == 1 and "where is the Gauss-Newton loop" in problems[0], problems
    # the kernels hold two copies of the loop; one is not enough
    problems, _ = _check(ml_fragment(), copies=2)
    assert len(problems) == 1 and "1 loop(s)" in problems[0] and "2 expected" in problems[0], problems
    assert mls.check(ml_fragment(), kernels=(r"k_step_imu9I\w*p48\w*fLi8ELb1E",), copies=1) != []   # no kernel of that name
