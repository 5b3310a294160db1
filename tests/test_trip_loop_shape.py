"""tools/trip_loop_shape.py, the build rule that keeps a trip of the 9-state gain iteration down to arithmetic: it holds
for the library as built, and on hand-written disassembly fragments it passes a clean trip loop and fires once for each
of its rules -- an LDS read in the trip, a vector-memory access, a wait for memory, one branch too many. (CPU only: the
rule reads text.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trip_loop_shape as tls  # noqa: E402
from disasm_fragment import FMA, KERNEL, NAME, Fragment  # noqa: E402

PER_LANE = ("s_and_saveexec_b64 s[90:91], s[6:7]", "s_cbranch_execz 0 <NEXT>", FMA, FMA, "s_or_b64 exec, exec, s[90:91]")


def fragment(in_trip=(), extra_branches=0, solve=300):
    """A kernel in llvm-objdump's format. An epoch loop (with a load and its wait, which are none of this rule's
    business) around a trip loop shaped like the real one: exit test at the top, 160 fp64 instructions of sweep, the
    vote of the convergence test around a cold block with the division, the skip of the solve, `solve` fp64
    instructions, the back-edge = 4 branches a trip. in_trip: instructions put into the sweep (PER_LANE: the masked
    block of the per-lane form, whose branch goes to the next instruction); extra_branches: that many more conditional
    branches (to the next instruction) in the sweep."""
    kernel = Fragment()
    emit, label, branch = kernel.emit, kernel.label, kernel.branch

    emit("global_load_dwordx2 v[0:1], v2, s[0:1]", "s_waitcnt vmcnt(0)")
    label("EPOCH")
    emit("global_load_dword v3, v2, s[4:5]", *[FMA] * 20, "s_waitcnt vmcnt(0)")
    label("TRIP")
    emit("s_andn2_b64 exec, exec, s[30:31]")
    branch("s_cbranch_execz", "DONE")
    emit(*[FMA] * 160)
    for ins in in_trip:
        if ins.endswith(" 0 <NEXT>"):
            branch(ins[:-len(" 0 <NEXT>")], f"N{len(kernel.body)}")
            label(f"N{len(kernel.body) - 1}")
        else:
            emit(ins)
    for k in range(extra_branches):
        branch("s_cbranch_scc1", f"X{k}")
        label(f"X{k}")
    emit("v_cmp_lt_f64_e64 s[10:11], |v[6:7]|, v[8:9]")
    branch("s_cbranch_vccz", "VOTED")
    emit("v_div_scale_f64 v[10:11], s[12:13], v[4:5], v[4:5], v[6:7]", "v_rcp_f64_e32 v[12:13], v[10:11]")
    label("VOTED")
    emit("s_and_saveexec_b64 vcc, s[10:11]")
    branch("s_cbranch_execz", "TRIP")
    emit(*[FMA] * solve, "v_add_u32_e32 v96, 1, v96")
    branch("s_branch", "TRIP")
    label("DONE")
    emit("s_or_b64 exec, exec, s[30:31]", *[FMA] * 20, "s_add_i32 s8, s8, 1", "s_cmp_lt_i32 s8, s9")
    branch("s_cbranch_scc1", "EPOCH")
    emit("s_endpgm")
    return kernel.text()


def _check(text, **kw):
    report = []
    return tls.check(text, kernels=KERNEL, report=report, **kw), report


def test_the_rule_holds_for_the_library_as_built():
    if not os.path.exists(os.path.join(CSRC, "libkfpos_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "trip_loop_shape.py"),
                          os.path.join(CSRC, "libkfpos_hip.so")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    # both headline kernels, each with the fast and the full form of the trip loop, and the loops set aside are named
    judged = [l for l in res.stdout.splitlines() if " blocks, " in l and "listed only" not in l]
    assert len(judged) == 4 and sum("IdfLi8ELb1E" in l for l in judged) == 2, res.stdout
    assert "the pairs' loop: listed only" in res.stdout and "the (I + M B) form: listed only" in res.stdout
    assert all(" ds 0, vmem 0, mem_waits 0," in l for l in judged), res.stdout


def test_a_trip_of_arithmetic_and_four_branches_passes():
    problems, report = _check(fragment())
    assert problems == [], problems
    assert len(report) == 2 and "fp64 462" in report[0] and "branches 4" in report[0], report   # the trip loop alone
    assert "usual path" in report[1] and "fp64 460" in report[1] and "branches 4" in report[1], report


def test_an_lds_read_in_the_trip_fails():
    problems, _ = _check(fragment(in_trip=("ds_read_b64 v[198:199], v240 offset:39424",)))
    assert len(problems) == 1 and "ds_read_b64" in problems[0] and "reads or writes memory" in problems[0], problems


def test_a_vector_memory_access_in_the_trip_fails():
    problems, _ = _check(fragment(in_trip=("global_load_dwordx2 v[14:15], v2, s[0:1]",)))
    assert len(problems) == 1 and "global_load_dwordx2" in problems[0], problems


def test_a_wait_for_memory_in_the_trip_fails():
    for wait in ("s_waitcnt lgkmcnt(0)", "s_waitcnt vmcnt(2)", "s_waitcnt vmcnt(0) lgkmcnt(1)"):
        problems, _ = _check(fragment(in_trip=(wait,)))
        assert len(problems) == 1 and "waits for memory" in problems[0], (wait, problems)
    assert _check(fragment(in_trip=("s_waitcnt expcnt(0)", "s_nop 1")))[0] == []   # (not a wait for memory)


def test_one_branch_too_many_fails():
    problems, _ = _check(fragment(extra_branches=1))
    assert len(problems) == 1 and "5 branch instructions on the usual path" in problems[0] and "maximum 4" in problems[0]
    assert _check(fragment(extra_branches=1), max_branches=5)[0] == []


def test_the_per_lane_form_is_known_by_its_second_masked_region_and_may_branch_once_more():
    # a kernel with a fast form only: fine; a kernel with nothing but the per-lane form: the fast form is missing
    assert tls.check(fragment(), kernels=KERNEL) == []
    problems, report = _check(fragment(in_trip=PER_LANE))
    assert "saveexec 2" in report[0] and "branches 5" in report[1], report
    assert len(problems) == 1 and "no fast form" in problems[0], problems
    # ... and there its fifth branch is allowed, a sixth is not
    problems, _ = _check(fragment(in_trip=PER_LANE, extra_branches=1))
    assert len(problems) == 2 and "6 branch instructions" in problems[1] and "maximum 5" in problems[1], problems


def test_the_usual_path_is_the_cycle_that_carries_the_trip():
    """the cycle that skips the solve is shorter, but it is not a trip: it does not count"""
    ins = tls.parse(fragment())[NAME]
    loops, cfg = tls.trip_loops(ins)
    assert len(loops) == 1
    comp, entries = loops[0]
    starts, ends, _ = cfg
    path = tls.usual_path(ins, comp, entries, cfg)
    n = sum(ends[b] - starts[b] for b in path)
    assert n == 160 + 300 + 8 and sum(tls.is_branch(ins[i][1]) for b in path for i in range(starts[b], ends[b])) == 4


def test_loops_that_are_not_the_trip_are_set_aside_or_missed_loudly():
    # the (I + M B) form: too much arithmetic for one solve -> listed, not judged; and then no trip loop is left
    problems, report = _check(fragment(in_trip=("ds_read_b64 v[198:199], v240",), solve=700))
    assert any("the (I + M B) form: listed only" in l for l in report), report
    assert len(problems) == 1 and "no trip loop of the information form" in problems[0], problems
    # the pairs' loop: a DPP exchange in it
    dpp = "v_mov_b32_dpp v5, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf"
    problems, report = _check(fragment(in_trip=("ds_read_b64 v[198:199], v240", dpp)))
    assert any("the pairs' loop: listed only" in l for l in report), report
    assert len(problems) == 1 and "no trip loop of the information form" in problems[0], problems
    # no loop with that much arithmetic, no kernel of that name
    assert any("where is the trip" in p for p in _check(fragment(solve=100))[0])
    assert tls.check(fragment(), kernels=(r"k_step_imu9I\w*p48\w*fLi8ELb1E",)) != []
