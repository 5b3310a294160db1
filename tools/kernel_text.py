"""What the build-time performance rules of libkfpos_hip.so share (tools/check_kernels.py lists the rules): the
disassembly of the gfx950 code objects and its parser, the control-flow graph of a kernel with its loops, the opcode
predicates and counters, the headline kernels, the judgement of a loop that should pay for arithmetic only, and the
command line of a rule. Nothing in here knows a rule's threshold or its wording.

A rule is a module with check(text or parsed kernels, ..., report=None) -> problems, OPTIONS = ((flag, type, default),
...) named like check()'s keyword arguments, HEADING (what its problems are listed under) and verdict(kernels, opts)
(the line it prints when it holds); run() judges by one, main() is its command line.
"""
import argparse
import os
import re
import shutil
import subprocess
import tempfile

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
# k_step_imu9<double,float,8,true,KArgs> (the bench kernel) and k_step_imu9<p48,float,8,true,KArgs>, mangled. The
# argument block is part of the pattern: the same template around CellArgs (anchor cells) keeps the plain epoch order,
# has no pairs' loop to find, and is not held to the headline kernels' rules. \w* in front of it: KArgs is mangled as a
# template argument in the library and as the parameter's type in names written before the block was a parameter.
ARGS = r"\w*5KArgsE"
KERNELS = (r"k_step_imu9IdfLi8ELb1E" + ARGS, r"k_step_imu9I\w*p48\w*fLi8ELb1E" + ARGS)
VMEM = ("global_", "flat_", "buffer_", "scratch_", "tbuffer_")
LINE = re.compile(r"^\s+(\S+)\s*(.*?)\s*//\s*([0-9A-Fa-f]+):\s*[0-9A-Fa-f ]*(?:<\S+?(?:\+0x([0-9a-fA-F]+))?>)?\s*$")
FP64 = re.compile(r"^v_(mul|fmac|fma|add|rsq|rcp|sqrt|min|max|ldexp|div_\w+|trig_preop|frexp_mant|fract|floor|ceil|rndne|trunc)_f64")


def disassemble(lib):
    tmp = tempfile.mkdtemp(prefix="kfpos_co_")
    try:
        local = os.path.join(tmp, "lib.so")
        shutil.copy(lib, local)
        subprocess.run([OBJDUMP, "--offloading", local], check=True, capture_output=True, cwd=tmp)
        cos = sorted(f for f in os.listdir(tmp) if "gfx950" in f)  # one code object per translation unit
        if not cos:
            raise SystemExit("no gfx950 code object in " + lib)
        return "\n".join(subprocess.run([OBJDUMP, "-d", "--no-show-raw-insn", os.path.join(tmp, co)], check=True,
                                        capture_output=True, text=True).stdout for co in cos)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def read(path):
    """the disassembly of a library, or the text of one kept as .s / .txt"""
    if path.endswith((".s", ".txt")):
        with open(path) as f:
            return f.read()
    return disassemble(path)


def parse(text):
    """{function: [(address, opcode, operands, branch target offset from the function start or None)]}"""
    func, insns = None, {}
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            func = m.group(1)
            insns[func] = []
            continue
        m = LINE.match(line)
        if m and func:
            off = None
            if m.group(1).startswith(("s_cbranch", "s_branch")) and "<" in line:
                off = int(m.group(4), 16) if m.group(4) else 0
            insns[func].append((int(m.group(3), 16), m.group(1), m.group(2), off))
    return insns


def parsed(text):
    """what every check() starts with: disassembly text or what parse() made of it -> the latter"""
    return parse(text) if isinstance(text, str) else text


def kernels_matching(insns, patterns, problems):
    """(name, instructions) of the kernels that match, pattern by pattern; a pattern without a kernel is a problem (a
    renamed kernel must not switch its rule off)"""
    for pattern in patterns:
        names = [f for f in insns if re.search(pattern, f) and insns[f]]
        if not names:
            problems.append(f"{pattern}: no kernel of that name")
        for f in names:
            yield f, insns[f]


# ---- opcodes

def is_fp64(op):
    return bool(FP64.match(op))


def is_branch(op):
    return op.startswith(("s_cbranch", "s_branch"))


def is_mem(op):
    return op.startswith("ds_") or op.startswith(VMEM)


def is_mem_wait(op, args):
    return op == "s_waitcnt" and ("lgkmcnt" in args or "vmcnt" in args)


def is_copy(op):
    return op.startswith(("v_mov_b", "v_accvgpr_"))


COUNTERS = {
    "instructions": lambda op, args: True,
    "fp64": lambda op, args: is_fp64(op),
    "valu_other": lambda op, args: op.startswith("v_") and not is_fp64(op),
    "agpr_read": lambda op, args: op.startswith("v_accvgpr_read"),
    "agpr_write": lambda op, args: op.startswith("v_accvgpr_write"),
    "accvgpr": lambda op, args: op.startswith("v_accvgpr"),
    "v_mov": lambda op, args: op.startswith("v_mov_b"),
    "lane_read": lambda op, args: op.startswith(("v_readlane", "v_readfirstlane")),
    "lane_write": lambda op, args: op.startswith("v_writelane"),
    "ds": lambda op, args: op.startswith("ds_"),
    "vmem": lambda op, args: op.startswith(VMEM),
    "mem_waits": is_mem_wait,
    "salu": lambda op, args: op.startswith("s_") and not is_branch(op) and op not in ("s_waitcnt", "s_nop"),
    "branches": lambda op, args: is_branch(op),
    "saveexec": lambda op, args: "saveexec" in op,
}
# fp64 instructions that make a cycle a trip loop of the gain iteration (two rules look for it)
TRIP_FP64 = 400
# what the rules about a trip loop list, in their order
LOOP_COLUMNS = ("instructions", "fp64", "ds", "vmem", "mem_waits", "branches", "salu", "v_mov", "accvgpr", "saveexec")


def mix(ins, idx, columns):
    """{column: how many of the instructions idx it counts}, in the order of `columns` (names of COUNTERS)"""
    ops = [ins[i][1:3] for i in idx]
    return {c: sum(bool(COUNTERS[c](op, args)) for op, args in ops) for c in columns}


# ---- control-flow graph

def blocks_of(ins):
    """(starts, ends, succ): basic blocks as instruction index ranges and their successor lists"""
    base = ins[0][0]
    index = {a: i for i, (a, _, _, _) in enumerate(ins)}
    target = [index.get(base + off) if off is not None else None for _, _, _, off in ins]
    leaders = {0}
    for i, (_, op, _, _) in enumerate(ins):
        if target[i] is not None:
            leaders.add(target[i])
        if (target[i] is not None or op == "s_endpgm") and i + 1 < len(ins):
            leaders.add(i + 1)
    starts = sorted(leaders)
    ends = starts[1:] + [len(ins)]
    block_at = {st: b for b, st in enumerate(starts)}
    succ = []
    for st, en in zip(starts, ends):
        out, op = [], ins[en - 1][1]
        if target[en - 1] is not None:
            out.append(block_at[target[en - 1]])
        if op not in ("s_branch", "s_endpgm") and en < len(ins) and block_at[en] not in out:
            out.append(block_at[en])
        succ.append(out)
    return starts, ends, succ


def predecessors(succ):
    pred = [[] for _ in succ]
    for b, out in enumerate(succ):
        for w in out:
            pred[w].append(b)
    return pred


def indices(cfg, blocks):
    """the instructions of these blocks, block by block"""
    starts, ends, _ = cfg
    return [i for b in blocks for i in range(starts[b], ends[b])]


def components(nodes, succ):
    """strongly connected components with a cycle, of the graph restricted to `nodes` (Tarjan, iterative)"""
    nodes = set(nodes)
    num, low, on, stack, comps, counter = {}, {}, set(), [], [], 0
    for root in sorted(nodes):
        if root in num:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                num[v] = low[v] = counter
                counter += 1
                stack.append(v)
                on.add(v)
            out = [w for w in succ[v] if w in nodes]
            if k < len(out):
                w = out[k]
                work.append((v, k + 1))
                if w not in num:
                    work.append((w, 0))
                elif w in on:
                    low[v] = min(low[v], num[w])
                continue
            if low[v] == num[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(sorted(comp))
            if work:
                low[work[-1][0]] = min(low[work[-1][0]], low[v])
    return comps


def largest_loop(ins):
    """(blocks of the largest cycle -- in the 9-state kernels the epoch loop with everything nested in it --, its header
    blocks, its latch blocks, its blocks outside nested loops, cfg) or None when the function has no loop"""
    cfg = blocks_of(ins)
    starts, ends, succ = cfg
    comps = components(range(len(starts)), succ)
    if not comps:
        return None
    loop = max(comps, key=lambda comp: sum(ends[b] - starts[b] for b in comp))
    inside, pred = set(loop), predecessors(succ)
    headers = [b for b in loop if any(p not in inside for p in pred[b])] or [loop[0]]
    latches = [b for b in loop if any(w in headers for w in succ[b])]
    nested = {b for c in components(inside - set(headers), succ) for b in c}
    return loop, headers, latches, [b for b in loop if b not in nested], cfg


def trip_loops(ins, min_fp64=TRIP_FP64):
    """[(blocks of the loop, its entry blocks)] for the innermost cycles that hold at least min_fp64 fp64 instructions:
    a component is split again, without its entry blocks, as long as a part of it still holds that many; with
    (starts, ends, succ) as a second result"""
    cfg = blocks_of(ins)
    succ = cfg[2]
    n, pred = len(succ), predecessors(succ)
    fp = [sum(is_fp64(ins[i][1]) for i in indices(cfg, [b])) for b in range(n)]
    found = []
    todo = [c for c in components(range(n), succ) if sum(fp[b] for b in c) >= min_fp64]
    while todo:
        comp = todo.pop()
        inside = set(comp)
        entries = [b for b in comp if any(p not in inside for p in pred[b])] or [comp[0]]
        inner = [c for c in components(inside - set(entries), succ) if sum(fp[b] for b in c) >= min_fp64]
        if inner:
            todo += inner
        else:
            found.append((comp, entries))
    return sorted(found), cfg


def usual_path(ins, comp, entries, cfg, min_fp64=TRIP_FP64):
    """blocks of the cycle through the loop's entry that carries the trip with the fewest instructions, or None"""
    starts, ends, succ = cfg
    inside = set(comp)
    size = {b: ends[b] - starts[b] for b in comp}
    fp = {b: sum(is_fp64(ins[i][1]) for i in range(starts[b], ends[b])) for b in comp}
    best = None
    for head in entries:
        work = [(head, [head])]
        while work:  # every simple path from the entry back to it (these loops have a handful of blocks)
            v, path = work.pop()
            for w in succ[v]:
                if w == head:
                    if sum(fp[b] for b in path) >= min_fp64:
                        cost = sum(size[b] for b in path)
                        if best is None or cost < best[0]:
                            best = (cost, path)
                elif w in inside and w not in path:
                    work.append((w, path + [w]))
    return None if best is None else best[1]


def arithmetic_only(ins, cfg, loop, min_fp64, where, noun, allowed, report=None, note=""):
    """What three rules ask of a loop (blocks, entry blocks) run by a lone wavefront: no DS or vector-memory
    instruction, no wait for memory, at most `allowed` branch instructions on the usual path of `noun` ("a trip", "a
    pass"). Lists the loop's instruction mix and that of its usual path in `report`; returns the problems."""
    comp, entries = loop
    idx = indices(cfg, comp)
    path = usual_path(ins, comp, entries, cfg, min_fp64)
    on_path = mix(ins, indices(cfg, path), LOOP_COLUMNS) if path else None
    if report is not None:
        report.append(where + note + f": {len(comp)} blocks, "
                      + ", ".join(f"{k} {v}" for k, v in mix(ins, idx, LOOP_COLUMNS).items()))
        if on_path:
            report.append(where + ": usual path: " + ", ".join(f"{k} {v}" for k, v in on_path.items()))
    problems = []
    for i in idx:
        a, op, args, _ = ins[i]
        if is_mem(op):
            problems.append(f"{where}: {op} at {a:#x}: {noun} reads or writes memory")
        elif is_mem_wait(op, args):
            problems.append(f"{where}: s_waitcnt {args} at {a:#x}: {noun} waits for memory")
    if on_path is None:
        problems.append(f"{where}: no cycle through its entry carries {min_fp64} fp64 instructions")
    elif on_path["branches"] > allowed:
        problems.append(f"{where}: {on_path['branches']} branch instructions on the usual path of {noun} "
                        f"(maximum {allowed})")
    return problems


# ---- a rule's command line

def defaults(options):
    return {flag[2:].replace("-", "_"): default for flag, _, default in options}


def run(rule, insns, opts, quiet=False):
    """Judge the parsed kernels by one rule and print what its script prints: its listing unless quiet, then its
    heading and problems, or its verdict. True when the rule holds."""
    report = []
    problems = rule.check(insns, report=report, **opts)
    if report and not quiet:
        print("\n".join(report))
    if problems:
        print("\n".join(([rule.HEADING + ":"] if rule.HEADING else []) + problems))
        return False
    print(rule.verdict(insns, opts))
    return True


def main(rule, kernels=True):
    """The command line of a rule: LIB (the library, or a disassembly as .s / .txt) and the rule's OPTIONS, of which one
    whose default is a tuple may be given several times; kernels: with --kernel REGEX ... and --quiet"""
    p = argparse.ArgumentParser(description=rule.__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("lib", metavar="LIB")
    for flag, kind, default in rule.OPTIONS:
        many = isinstance(default, tuple)
        p.add_argument(flag, type=kind, action="append" if many else "store", default=[] if many else default)
    if kernels:
        p.add_argument("--kernel", dest="kernels", action="append", default=[])
        p.add_argument("--quiet", action="store_true")
    opts = vars(p.parse_args())
    for key, value in opts.items():
        if isinstance(value, list):
            opts[key] = tuple(value) or (KERNELS if key == "kernels" else ())
    lib, quiet = opts.pop("lib"), opts.pop("quiet", False)
    raise SystemExit(0 if run(rule, parse(read(lib)), opts, quiet) else 1)
