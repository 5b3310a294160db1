"""tools/epoch_turnaround_shape.py, the build rule that keeps the covariance out of the registers a lane carries across
the back-edge of the 9-state epoch loop: it holds for the library as built, and on hand-written disassembly fragments it
passes a latch that copies a position, a velocity and a few words, and fires for one that copies a covariance as well.
(CPU only: the rule reads text.)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import epoch_turnaround_shape as ets  # noqa: E402
from disasm_fragment import FMA, KERNEL, NAME, Fragment  # noqa: E402



def fragment(latch_copies=(), body_copies=()):
    """A kernel in llvm-objdump's format: a prologue, an epoch loop whose header unpacks (two AGPR reads, a conversion),
    a nested trip loop of 40 fp64 instructions, a divergent early exit that reloads from LDS, a covariance update, and a
    latch block of its own -- entered by a branch, so that it holds nothing but what the back-edge costs -- with
    `latch_copies`. body_copies go into the covariance update (none of the rule's business)."""
    kernel = Fragment()
    emit, label, branch = kernel.emit, kernel.label, kernel.branch

    emit("global_load_dwordx2 v[0:1], v2, s[0:1]", "s_waitcnt vmcnt(0)", *[FMA] * 10)
    label("EPOCH")
    emit("v_accvgpr_read_b32 v58, a18", "v_accvgpr_read_b32 v59, a19", "v_cvt_f64_f32_e32 v[10:11], v58",
         "global_load_dword a18, v[2:3], off", "v_cmp_u_f64_e32 vcc, v[4:5], v[4:5]", "s_and_saveexec_b64 s[10:11], vcc")
    branch("s_cbranch_execz", "EARLY")
    emit(*[FMA] * 12)
    label("TRIP")
    emit(*[FMA] * 40, "s_cmp_lt_i32 s12, s13")
    branch("s_cbranch_scc1", "TRIP")
    emit("ds_read_b64 v[20:21], v240", *[FMA] * 30, *body_copies, "v_readlane_b32 s2, v254, 3", "v_writelane_b32 v254, s2, 4")
    label("EARLY")
    emit("s_or_b64 exec, exec, s[10:11]", "ds_write_b64 v240, v[20:21]", "s_add_i32 s8, s8, 1", "s_cmp_lt_i32 s8, s9")
    branch("s_cbranch_scc0", "DONE")
    label("LATCH")
    emit(*latch_copies)
    branch("s_branch", "EPOCH")
    label("DONE")
    emit("global_store_dwordx2 v2, v[4:5], s[0:1]", "s_endpgm")
    return kernel.text()


# position and velocity to where the header expects them, three words: what a lane legitimately carries
STATE = tuple(f"v_accvgpr_write_b32 a{k}, v{156 + k}" for k in range(12)) + (
    "v_mov_b32_e32 v98, v190", "v_accvgpr_mov_b32 a39, a100", "v_mov_b64_e32 v[240:241], v[208:209]")
# ... and a covariance: 45 doubles
COVARIANCE = tuple(f"v_accvgpr_write_b32 a{100 + k}, v{100 + k}" for k in range(46)) + tuple(
    f"v_mov_b64_e32 v[{2 * k}:{2 * k + 1}], v[{60 + 2 * k}:{61 + 2 * k}]" for k in range(22))


def _check(text, **kw):
    report = []
    return ets.check(text, kernels=KERNEL, report=report, **kw), report


def test_the_rule_holds_for_the_library_as_built():
    if not os.path.exists(os.path.join(CSRC, "libkfpos_hip.so")):
        import __graft_entry__
        __graft_entry__.build()
    res = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "epoch_turnaround_shape.py"),
                          os.path.join(CSRC, "libkfpos_hip.so")], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    verdicts = [l for l in res.stdout.splitlines() if "latch block(s) at" in l]
    assert len(verdicts) == 2 and sum("IdfLi8ELb1E" in l for l in verdicts) == 1, res.stdout   # both headline kernels
    assert sum(l.lstrip().startswith("total") for l in res.stdout.splitlines()) == 2, res.stdout


def test_a_latch_that_carries_state_and_words_passes():
    problems, report = _check(fragment(latch_copies=STATE))
    assert problems == [], problems
    assert any("15 register copies" in l for l in report), report
    # the listing: header, latch and the blocks between them, without the trip loop; the totals
    rows = [l.split() for l in report if l.startswith("  ") and l.split()[0].startswith("0x")]
    assert sum(r[-1] == "header" for r in rows) == 1 and sum(r[-1] == "latch" for r in rows) == 1, report
    total = dict(zip(ets.COLUMNS, map(int, [l for l in report if l.lstrip().startswith("total")][0].split()[1:])))
    assert total["fp64"] == 12 + 30 and total["agpr_read"] == 2 and total["agpr_write"] == 12, total   # (no trip: 40)
    assert total["lane_read"] == 1 and total["lane_write"] == 1 and total["ds"] == 2 and total["vmem"] == 1, total
    assert total["v_mov"] == 2 and total["branches"] == 3, total   # (the trip's own branch is nested)


def test_a_latch_that_carries_a_covariance_fails():
    problems, report = _check(fragment(latch_copies=STATE + COVARIANCE))
    assert len(problems) == 1 and "83 register copies (maximum 32)" in problems[0], problems
    assert _check(fragment(latch_copies=STATE + COVARIANCE), max_copies=83)[0] == []
    # 32 pass, 33 do not
    assert _check(fragment(latch_copies=COVARIANCE[:32]))[0] == []
    assert len(_check(fragment(latch_copies=COVARIANCE[:33]))[0]) == 1


def test_copies_elsewhere_are_listed_not_judged():
    problems, report = _check(fragment(latch_copies=STATE, body_copies=COVARIANCE))
    assert problems == [], problems
    total = [l for l in report if l.lstrip().startswith("total")][0].split()
    assert int(total[1 + ets.COLUMNS.index("agpr_write")]) == 12 + 46, report


def test_a_kernel_that_is_missing_or_has_no_loop_is_said_so():
    assert ets.check(fragment(), kernels=(r"k_step_imu9I\w*p48\w*fLi8ELb1E",)) != []
    text = f"{0x1000:016x} <{NAME}>:\n\t{FMA}  // 000000001000: BF800000\n\ts_endpgm  // 000000001004: BF810000\n"
    problems, _ = _check(text)
    assert len(problems) == 1 and "no loop" in problems[0], problems
