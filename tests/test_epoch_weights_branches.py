"""tools/epoch_weights_branches.py, the build rule that keeps the weights of a 9-state epoch -- between the unpack and
the first trip loop of the gain iteration -- selects instead of one masked region per anchor: it holds for the library
as built, and on hand-written disassembly fragments it passes a stretch with a few masked regions, fires for one with a
region per anchor and a nested short-circuit, and counts neither the regions inside nested loops nor those behind the
first trip loop. (CPU only: the rule reads text.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epoch_weights_branches as ewb  # noqa: E402
from disasm_fragment import FMA, KERNEL, NAME, Fragment  # noqa: E402

LOAD = "global_load_dword v9, v[2:3], off"
SELECT = "v_cndmask_b32_e32 v7, 0, v7, vcc"


def fragment(regions=0, regions_in_solve=0, regions_behind=0, loads=16):
    """A kernel in llvm-objdump's format: a prologue; an epoch loop whose header unpacks (`loads` loads); `regions`
    masked regions of a reciprocal each (saveexec, execz, five fp64, restore); a Gauss-Newton loop of 60 fp64 with
    `regions_in_solve` regions inside; eight selects; a trip loop of 420 fp64; `regions_behind` regions; the latch."""
    kernel = Fragment()
    emit, label, branch = kernel.emit, kernel.label, kernel.branch

    def region(tag):
        emit("v_cmp_lt_f64_e32 vcc, 0, v[10:11]", "s_and_saveexec_b64 s[10:11], vcc")
        branch("s_cbranch_execz", tag)
        emit(*[FMA] * 5)
        label(tag)
        emit("s_or_b64 exec, exec, s[10:11]")

    emit("global_load_dwordx2 v[0:1], v2, s[0:1]", "s_waitcnt vmcnt(0)", *[FMA] * 10)
    label("EPOCH")
    emit(*[LOAD] * loads, "v_cvt_f64_f32_e32 v[10:11], v58")
    for k in range(regions):
        region(f"W{k}")
    label("SOLVE")
    emit(*[FMA] * 60)
    for k in range(regions_in_solve):
        region(f"S{k}")
    emit("s_cmp_lt_i32 s14, s15")
    branch("s_cbranch_scc1", "SOLVE")
    emit(*[SELECT] * 8)
    label("TRIP")
    emit(*[FMA] * 420, "s_cmp_lt_i32 s12, s13")
    branch("s_cbranch_scc1", "TRIP")
    for k in range(regions_behind):
        region(f"B{k}")
    emit("ds_write_b64 v240, v[20:21]", "s_add_i32 s8, s8, 1", "s_cmp_lt_i32 s8, s9")
    branch("s_cbranch_scc1", "EPOCH")
    emit("global_store_dwordx2 v2, v[4:5], s[0:1]", "s_endpgm")
    return kernel.text()


def _check(text, **kw):
    report = []
    return ewb.check(text, kernels=KERNEL, report=report, **kw), report


def test_the_rule_holds_for_the_library_as_built():
    if not os.path.exists(os.path.join(CSRC, "libkfpos_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "epoch_weights_branches.py"),
                          os.path.join(CSRC, "libkfpos_hip.so")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    verdicts = [l for l in res.stdout.splitlines() if "s_cbranch_execz between the unpack and" in l]
    assert len(verdicts) == 2 and sum("IdfLi8ELb1E" in l for l in verdicts) == 1, res.stdout   # both headline kernels


def test_selects_and_a_few_regions_pass():
    problems, report = _check(fragment(regions=3))
    assert problems == [], problems
    assert any(l.endswith(": 3 s_cbranch_execz between the unpack and the first trip loop") for l in report), report
    # the mix of the stretch: the regions and the selects, without the Gauss-Newton loop (60 fp64) and the trip loop
    # (the first region opens in the unpack block: its saveexec and its branch are there, the branch is counted)
    mix = [l for l in report if "blocks outside nested loops between them" in l][0]
    assert "fp64 15," in mix and "saveexec 2," in mix and "branches 2," in mix, mix


def test_a_region_per_anchor_and_a_nested_short_circuit_fail():
    problems, _ = _check(fragment(regions=8 + 7 + 8))
    assert len(problems) == 1 and "23 s_cbranch_execz" in problems[0] and "(maximum 12)" in problems[0], problems
    assert _check(fragment(regions=12))[0] == [] and len(_check(fragment(regions=13))[0]) == 1
    assert _check(fragment(regions=23), max_execz=23)[0] == []


def test_regions_inside_nested_loops_and_behind_the_first_trip_loop_do_not_count():
    problems, report = _check(fragment(regions=2, regions_in_solve=20, regions_behind=20))
    assert problems == [], problems
    assert any(l.endswith(": 2 s_cbranch_execz between the unpack and the first trip loop") for l in report), report


def test_a_kernel_without_unpack_or_trip_loop_is_said_so():
    problems, _ = _check(fragment(loads=2))
    assert len(problems) == 1 and "where is the unpack" in problems[0], problems
    assert ewb.check(fragment(), kernels=(r"k_step_imu9I\w*p48\w*fLi8ELb1E",)) != []
    text = f"{0x1000:016x} <{NAME}>:\n\t{FMA}  // 000000001000: BF800000\n\ts_endpgm  // 000000001004: BF810000\n"
    problems, _ = _check(text)
    assert len(problems) == 1 and "no loop" in problems[0], problems
