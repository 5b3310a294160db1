#!/usr/bin/env python3
"""What can the three vector-memory waits of the 9-state kernel's epoch loop cost at most? Timing variants of
kfpos_k_imu9.hip AS IT STOOD BEFORE those waits were removed (--src: a checkout of that revision's roskfpos_amd/csrc;
the edits below match its text and nothing newer). Results are WRONG by construction, only the duration is of interest;
nothing here ships:
  libkfpos_dtshared.so  the dt of a multi-epoch launch is a.dt_shared: no load, no wait for it in the loop
  libkfpos_noimu.so     no accelerometer fetch inside the loop: every epoch reuses the sample of epoch 0
  libkfpos_notraj.so    no pose store in the loop
(T_parent - T_variant) per epoch is an upper bound for the wait in question (the variant also sheds the instructions).
Only kfpos_k_imu9 is recompiled, with the Makefile's flags; the other objects are those of --src (build it first).
Output: tools/exp/_build/ (git-ignored); select a library with KFPOS_LIB_PATH.
"""
import argparse
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
OUT = os.path.join(ROOT, "tools", "exp", "_build")
UNITS = "kfpos_k_toa6f kfpos_k_toa6s kfpos_k_misc kfpos_k_coop kfpos_k_tags kfpos_hip kfpos_hip_state kfpos_hip_slots kfpos_hip_replay kfpos_comm".split()
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=on", "-Rpass-analysis=kernel-resource-usage"]

EDITS = {
    "dtshared": ("const double dt = epoch_dt(a, t, e);",
                 "const double dt = a.n_steps > 1 ? a.dt_shared : epoch_dt(a, t, e);"),
    "noimu": ("if constexpr (AHEAD) fetch_imu<MREAL>(a, opaque_lane(t), opaque_uniform(e + 1), rawi);",
              "(void)0; /* EXPERIMENT: the sample of epoch 0 again */"),
    "notraj": ("if (a.traj) { /* the pose a per-epoch caller", "if (false) { /* EXPERIMENT: no pose; a per-epoch caller"),
}


def variant(src, name):
    old, new = EDITS[name]
    text = open(os.path.join(src, "kfpos_k_imu9.hip")).read()
    if text.count(old) != 1:
        raise SystemExit(f"{name}: the text to edit is not in {src}/kfpos_k_imu9.hip (a newer revision?)")
    hip = os.path.join(src, f"_exp_{name}.hip")  # next to the headers it includes
    obj = os.path.join(OUT, f"kfpos_k_imu9_{name}.o")
    lib = os.path.join(OUT, f"libkfpos_{name}.so")
    open(hip, "w").write(text.replace(old, new))
    try:
        res = subprocess.run(["hipcc"] + FLAGS + ["-c", "-o", obj, hip], capture_output=True, text=True)
    finally:
        os.remove(hip)
    if res.returncode:
        sys.stderr.write(res.stderr[-3000:])
        raise SystemExit(1)
    cur = None
    for line in res.stderr.splitlines():
        if "Function Name:" in line:
            cur = line.split("Function Name:")[1].split()[0]
        if cur and "k_step_imu9IdfLi8ELb1" in cur and ("ScratchSize" in line or "VGPRs:" in line or "AGPRs:" in line):
            print(name, line.split("remark:")[1].split("[-R")[0].strip())
    objs = [os.path.join(src, u + ".o") for u in UNITS]
    subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, obj] + objs + ["-ldl"])
    os.remove(obj)
    print("built", lib)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "roskfpos_amd", "csrc"))
    ap.add_argument("names", nargs="*", default=sorted(EDITS))
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    for n in args.names:
        variant(os.path.abspath(args.src), n)
