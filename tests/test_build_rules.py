"""The build-time performance rules of roskfpos_amd/csrc (make check = tools/check_kernels.py, which runs every rule on
one disassembly), and the first of them, tools/check_scratch.py: no scratch access inside a loop, and the kernels written
to share a SIMD two at a time still fit twice. Neither can be seen by a parity test -- a kernel that lost its second
wavefront computes the same bits 25-40 % slower -- so the rules themselves are tested: they hold for the library as
built, and they do fire."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
TOOL = os.path.join(ROOT, "tools", "check_scratch.py")
DRIVER = os.path.join(ROOT, "tools", "check_kernels.py")
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import check_scratch  # noqa: E402
from disasm_fragment import FMA, NAME, NAME_P48, Fragment  # noqa: E402


def _built():
    if not (os.path.exists(os.path.join(CSRC, "libkfpos_hip.so")) and os.path.exists(os.path.join(CSRC, "build.log"))):
        import __graft_entry__
        __graft_entry__.build()


def _run(*rules):
    cmd = [sys.executable, TOOL, os.path.join(CSRC, "libkfpos_hip.so"), "--resource-log", os.path.join(CSRC, "build.log")]
    for r in rules:
        cmd += ["--min-occupancy", r]
    return subprocess.run(cmd, capture_output=True, text=True)


def test_make_check_holds_for_the_library_as_built():
    _built()
    res = subprocess.run(["make", "-s", "-C", CSRC, "check"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "3 occupancy rule(s) hold" in res.stdout


def test_occupancy_rule_fires():
    _built()
    ok = _run("k_step_toa6_w2=2")
    assert ok.returncode == 0 and "1 occupancy rule(s) hold" in ok.stdout
    # the 9-state kernel holds its state in 256 VGPRs + AGPRs: one wavefront per SIMD, and the rule says so
    bad = _run(r"k_step_imu9I\w*5KArgsE=2")  # (around KArgs: the twelve kernels this rule has always named)
    assert bad.returncode == 1 and "1 wavefront(s) per SIMD, 2 required" in bad.stdout
    # a rule that matches nothing is an error too (a renamed kernel must not switch its rule off)
    gone = _run("k_no_such_kernel=2")
    assert gone.returncode == 1 and "no kernel of that name" in gone.stdout


def test_scratch_inside_a_loop_fires_and_scratch_in_the_prologue_passes():
    """on hand-written text: the rule stands on the control-flow graph it shares with the other rules"""
    def kernel(in_prologue=(), in_loop=()):
        k = Fragment()
        k.emit("s_load_dwordx2 s[0:1], s[4:5], 0x0", *in_prologue, "v_mov_b32_e32 v9, 0")
        k.label("LOOP")
        k.emit(FMA, *in_loop, FMA, "s_add_i32 s8, s8, 1", "s_cmp_lt_i32 s8, s9")
        k.branch("s_cbranch_scc1", "LOOP")
        k.emit("s_endpgm")
        return k.text()

    reload = "scratch_load_dword v3, off, off offset:4"
    assert check_scratch.check(kernel(in_prologue=(reload,))) == []
    problems = check_scratch.check(kernel(in_loop=(reload,)))
    assert problems == [f"{NAME}: 1 scratch access(es) inside a loop"], problems
    # two in the loop, one outside: the two are counted
    problems = check_scratch.check(kernel(in_prologue=(reload,), in_loop=(reload, "scratch_store_dword off, v3, off")))
    assert problems == [f"{NAME}: 2 scratch access(es) inside a loop"], problems


def headline_kernel(name, base, latch_copies):
    """A kernel that every rule of make check finds its loops in and lets pass: an epoch loop whose header unpacks 16
    loads and waits for them 320 instructions later, a Gauss-Newton loop, a trip loop, a pairs' loop (each with its
    vote, its skip, its exit and its back-edge), a second Gauss-Newton loop in front (the ML start), and a latch block
    of `latch_copies` register copies."""
    k = Fragment(name, base)

    def loop(tag, fp64, in_sweep=()):
        k.label(tag)
        k.emit("s_andn2_b64 exec, exec, s[30:31]")
        k.branch("s_cbranch_execz", tag + "_DONE")
        k.emit(*[FMA] * 160, *in_sweep, "v_cmp_lt_f64_e64 s[10:11], |v[6:7]|, v[8:9]")
        k.branch("s_cbranch_vccz", tag + "_VOTED")
        k.emit("v_rcp_f64_e32 v[12:13], v[10:11]")
        k.label(tag + "_VOTED")
        k.emit("s_and_saveexec_b64 vcc, s[10:11]")
        k.branch("s_cbranch_execz", tag)
        k.emit(*[FMA] * (fp64 - 160))
        k.branch("s_branch", tag)
        k.label(tag + "_DONE")
        k.emit("s_or_b64 exec, exec, s[30:31]")

    k.emit("s_load_dwordx2 s[0:1], s[4:5], 0x0", "scratch_load_dword v3, off, off offset:4")
    k.label("EPOCH")
    k.emit(*["global_load_dword v9, v[2:3], off"] * 16, *[FMA] * 320, "s_waitcnt vmcnt(0)", "s_cmp_eq_u32 s20, 0")
    k.branch("s_cbranch_scc1", "SEED")
    loop("START", 340)
    k.label("SEED")
    loop("ML", 340)
    k.emit(*["v_cndmask_b32_e32 v7, 0, v7, vcc"] * 8)
    loop("TRIP", 460)
    loop("PAIRS", 380, in_sweep=("v_mov_b32_dpp v5, v4 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf",))
    k.emit("ds_write_b64 v240, v[20:21]", "s_add_i32 s8, s8, 1", "s_cmp_lt_i32 s8, s9")
    k.branch("s_cbranch_scc0", "OUT")
    k.emit(*[f"v_accvgpr_write_b32 a{i}, v{100 + i}" for i in range(latch_copies)])
    k.branch("s_branch", "EPOCH")
    k.label("OUT")
    k.emit("s_endpgm")
    return k.text()


def test_check_kernels_names_the_one_broken_rule_and_still_judges_the_others(tmp_path):
    """on hand-written text: both headline kernels pass all seven rules; with a covariance in one latch, the turnaround
    rule breaks, its heading and problem are printed, the other six verdicts too, and the exit status is 1"""
    log = tmp_path / "build.log"
    log.write_text(f"remark: Function Name: {NAME}\nremark:     ScratchSize [bytes/lane]: 8\n"
                   "remark:     Occupancy [waves/SIMD]: 1\n")

    def run(copies_p48):
        src = tmp_path / "kernels.s"
        src.write_text(headline_kernel(NAME, 0x1000, 15) + "\n" + headline_kernel(NAME_P48, 0x100000, copies_p48))
        return subprocess.run([sys.executable, DRIVER, str(src), "--resource-log", str(log), "--min-occupancy",
                               "k_step_imu9IdfLi8ELb1E=1"], capture_output=True, text=True)

    verdicts = ["no kernel touches scratch inside a loop (2 scratch instructions in the library, all outside loops); "
                "1 occupancy rule(s) hold",
                "no epoch loop waits for a vector-memory operation issued fewer than 300 instructions before",
                "the trip loops of the 9-state gain iteration hold no memory access or wait and at most 4 branches a trip",
                "the pairs' loops of the 9-state gain iteration hold no memory access or wait and at most 4 branches a trip",
                "the Gauss-Newton loops of the 9-state kernels hold no memory access or wait and at most 4 branches a pass",
                "the latch of the 9-state epoch loop holds at most 32 register copies",
                "at most 12 s_cbranch_execz between the unpack of a 9-state epoch and its first trip loop"]
    ok = run(15)
    assert ok.returncode == 0 and ok.stdout.splitlines() == verdicts, ok.stdout + ok.stderr
    bad = run(60)
    lines = bad.stdout.splitlines()
    assert bad.returncode == 1, bad.stdout + bad.stderr
    assert lines[:5] == verdicts[:5] and lines[-1] == verdicts[6], bad.stdout
    assert lines[5] == "the 9-state epoch loop carries too much across its back-edge in registers:", bad.stdout
    assert len(lines) == 8 and lines[6].startswith(NAME_P48) and "60 register copies (maximum 32)" in lines[6], bad.stdout
