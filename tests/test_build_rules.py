"""The build-time performance rules of roskfpos_amd/csrc (make check = tools/check_kernels.py, which runs every rule on
one disassembly), and the first of them, tools/check_scratch.py: no scratch access inside a loop, and the kernels written
to share a SIMD two at a time still fit twice. Neither can be seen by a parity test -- a kernel that lost its second
wavefront computes the same bits 25-40 % slower -- so the rules themselves are tested: they hold for the library as
built, and they do fire."""
import os
import re
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


def _units():
    """the translation units of the library, as the Makefile lists them"""
    line = next(l for l in open(os.path.join(CSRC, "Makefile")) if l.startswith("UNITS"))
    return line.split(":=")[1].split()


def _built():
    have = ["libkfpos_hip.so", "build.log"] + [u + ".d" for u in _units()]
    if not all(os.path.exists(os.path.join(CSRC, f)) for f in have):
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


def _headers_seen(unit):
    """the project files unit.hip includes, as the compiler lists them (its own headers carry absolute paths)"""
    res = subprocess.run(["hipcc", "-MM", "--offload-arch=gfx950", "-std=c++17", unit + ".hip"], cwd=CSRC,
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    words = res.stdout.replace("\\\n", " ").split()
    seen = {w for w in words if not w.startswith(("/", "#")) and not w.endswith((":", ".hip"))
            and (w.endswith((".h", ".inc")))}
    assert seen, res.stdout
    return seen


def test_a_kernel_unit_sees_no_host_header_and_a_host_unit_no_device_header():
    """what the split of kfpos_kernels.h promises: the handle and the host glue are out of every kernel unit's sight, the
    two kernel units that run no filter see none of the per-tag arithmetic, and the host units see no device helper"""
    units = _units()
    kernels = [u for u in units if u.startswith("kfpos_k_")]
    hosts = [u for u in units if u.startswith("kfpos_hip")]
    assert len(kernels) == 16 and len(hosts) == 4, units
    for u in kernels + hosts:
        seen = _headers_seen(u)
        for h in seen:
            assert os.path.exists(os.path.join(CSRC, h)), (u, h)
        names = {os.path.basename(h) for h in seen}
        if u in kernels:
            assert not names & {"kfpos_internal.h", "kfpos_host.h", "kfpos_policy.h", "kfpos_owned.h"}, (u, sorted(names))
            assert "kfpos_kargs.h" in names, (u, sorted(names))
        if u in ("kfpos_k_d16", "kfpos_k_tags"):
            assert not [h for h in names if h.startswith("kfpos_core")], (u, sorted(names))
        if u in hosts:
            assert "kfpos_kernels.h" not in names, (u, sorted(names))
            assert {"kfpos_host.h", "kfpos_internal.h", "kfpos_policy.h", "kfpos_owned.h"} <= names, (u, sorted(names))


def _would_rebuild(*touched):
    """the units `make` would compile again if these headers were newer than everything (a dry run: nothing is built)"""
    cmd = ["make", "-n", "-C", CSRC]
    for h in touched:
        cmd += ["-W", h]
    res = subprocess.run(cmd + ["libkfpos_hip.so"], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    return set(re.findall(r"-c -o (\w+)\.o ", res.stdout))


def test_a_touched_header_rebuilds_its_side_only():
    """the Makefile takes each unit's headers from the compiler (%.d): a host-side edit reaches no kernel unit, an edit to
    the device helpers no host unit"""
    _built()
    assert _would_rebuild() == set(), "the library as built is up to date"
    host = _would_rebuild("kfpos_internal.h", "kfpos_host.h")
    assert host == _would_rebuild("kfpos_policy.h") == _would_rebuild("kfpos_owned.h")
    assert host == {"kfpos_hip", "kfpos_hip_state", "kfpos_hip_slots", "kfpos_hip_replay", "kfpos_comm"}, sorted(host)
    device = _would_rebuild("kfpos_kernels.h")
    assert device and all(u.startswith("kfpos_k_") for u in device), sorted(device)
    assert {"kfpos_k_imu9", "kfpos_k_toa6s", "kfpos_k_misc", "kfpos_k_coop"} <= device, sorted(device)
    assert not device & {"kfpos_k_d16", "kfpos_k_tags"}, sorted(device)
