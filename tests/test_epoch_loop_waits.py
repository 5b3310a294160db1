"""tools/epoch_loop_waits.py, the build rule that keeps vector-memory waits out of the 9-state kernel's epoch loop, on two
hand-written disassembly fragments: a loop whose `s_waitcnt vmcnt(0)` sits ten instructions behind a load fails, the same
loop with the wait 400 instructions behind passes. (CPU only: the rule reads text.)"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epoch_loop_waits as elw  # noqa: E402
from disasm_fragment import NAME, Fragment  # noqa: E402


def fragment(gap):
    """A kernel in llvm-objdump's format: a prologue with a load and its wait (outside the loop: not the rule's
    business), then one loop = load, `gap` - 1 arithmetic instructions, s_waitcnt vmcnt(0), a store, 350 more
    arithmetic instructions (so that the store is far from the wait around the back-edge), backward branch."""
    k = Fragment()
    k.emit("global_load_dwordx2 v[0:1], v2, s[0:1]", "s_waitcnt vmcnt(0)", "v_mov_b32_e32 v9, 0")
    k.label("LOOP")
    k.emit("global_load_dword v3, v2, s[4:5]")
    k.emit(*["v_fma_f64 v[4:5], v[0:1], v[0:1], v[4:5]"] * (gap - 1))
    k.emit("s_waitcnt vmcnt(0)", "v_cvt_f64_f32_e32 v[6:7], v3", "global_store_dwordx2 v2, v[4:5], s[6:7]")
    k.emit(*["v_add_f64 v[4:5], v[4:5], v[6:7]"] * 350)
    k.emit("s_add_i32 s8, s8, 1", "s_cmp_lt_i32 s8, s9")
    k.branch("s_cbranch_scc1", "LOOP")
    k.emit("s_endpgm")
    return k.text()


def test_wait_ten_instructions_behind_its_load_fails():
    report = []
    problems = elw.check(fragment(10), kernels=(r"k_step_imu9IdfLi8ELb1E",), report=report)
    assert len(report) == 1 and "vmcnt(0)" in report[0] and "10 instructions" in report[0], report
    assert len(problems) == 1 and "minimum 300" in problems[0], problems


def test_wait_400_instructions_behind_its_load_passes():
    report = []
    problems = elw.check(fragment(400), kernels=(r"k_step_imu9IdfLi8ELb1E",), report=report)
    assert len(report) == 1 and "400 instructions" in report[0], report
    assert problems == []


def test_the_store_counts_and_the_wait_may_leave_younger_operations_alone():
    """vmcnt(1) behind load + store waits for the load (the store may stay outstanding); vmcnt(0) waits for the store"""
    text = fragment(400)
    ins = elw.parse(text)[NAME]
    body = elw.outermost_loop(ins)
    assert ins[body[0]][1] == "global_load_dword" and ins[body[-1]][1] == "s_cbranch_scc1"  # the prologue is not in it
    # a second wait near the branch: 351 behind the store with vmcnt(0), all the way back to the load with vmcnt(1)
    for cnt, want in ((0, 351), (1, 351 + 402)):
        lines = text.splitlines()
        k = next(i for i, l in enumerate(lines) if "s_add_i32" in l)
        lines[k] = lines[k].replace("s_add_i32 s8, s8, 1", f"s_waitcnt vmcnt({cnt})")
        waits = elw.waits_in_loop(elw.parse("\n".join(lines))[NAME])
        assert [w[1:] for w in waits] == [(0, 400), (cnt, want)], waits


def test_a_kernel_that_is_not_there_is_a_problem():
    assert elw.check(fragment(400), kernels=(r"k_step_imu9I\w*p48\w*fLi8ELb1E",)) != []
