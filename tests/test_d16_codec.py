"""include/kfpos_d16.h: the wire format of KFPOS_SLOT_RANGES_D16 -- one int16 code per range element against a base the
encoder and the decoder both move, exceptions in an escape list -- and the layout of the block that carries it
(kfpos_layout::delta_layout of roskfpos_amd/csrc/kfpos_host_layout.h).

The checks live in a stand-alone C++ driver, tests/d16/d16_driver.cpp, built here with g++ and the address and
undefined-behaviour sanitizers (into tmp_path; nothing built is kept); no GPU, no library. kfpos_d16_put followed by
kfpos_d16_decode_ref returns v > 0 ? v : 0, and the encoder's base equals the decoder's after every round, over rounds that
hold: deltas of -32766, -32767, -32768, 32767 and 32768 (the inner two are codes, the others escape); v of 0, -1 and
INT32_MIN; a base of INT32_MAX with a small v (the difference is taken in 64 bits: the undefined-behaviour sanitizer would
say otherwise); absent -> present; skipped tags with stale codes and a forged escape entry; an escape list exactly full
and one put beyond it. The numpy restatement the GPU tests encode with (tests/d16.py) agrees with the driver, code for
code, on seeded matrices."""
import os
import subprocess

import numpy as np
import pytest

import d16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "roskfpos_amd", "csrc")
SRC = os.path.join(ROOT, "tests", "d16", "d16_driver.cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("d16") / "d16_driver")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", os.path.join(ROOT, "include"), "-I", CSRC, "-o", exe, SRC], check=True)
    return exe


def test_put_then_decode_and_the_layout(driver):
    out = subprocess.run([driver], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.startswith("OK "), out.stdout[-3000:] + out.stderr[-3000:]
    assert int(out.stdout.split()[1]) > 1000  # the checks ran


@pytest.mark.parametrize("lang", ["c", "c++"])
def test_the_header_compiles_alone(tmp_path, lang):
    src = tmp_path / ("alone.c" if lang == "c" else "alone.cpp")
    src.write_text('#include "kfpos_d16.h"\nint main(void) { return KFPOS_D16_ESCAPE - KFPOS_D16_ABSENT - 1; }\n')
    cc = ["gcc", "-std=c99"] if lang == "c" else ["g++", "-std=c++17"]
    subprocess.run(cc + ["-Wall", "-Wextra", "-Werror", "-pedantic", "-I", os.path.join(ROOT, "include"),
                         "-o", str(tmp_path / "alone"), str(src)], check=True)
    assert subprocess.run([str(tmp_path / "alone")]).returncode == 0


@pytest.mark.parametrize("A,T,seed", [(1, 1, 1), (5, 65, 2), (8, 4099, 3)])
def test_numpy_codec_agrees_with_the_header(driver, tmp_path, A, T, seed):
    rng = np.random.default_rng(seed)
    R = 8
    v = rng.integers(20000, 60000, size=(A, T)).astype(np.int32)
    rounds = []
    for r in range(R):
        v = v + rng.integers(-80, 81, size=(A, T)).astype(np.int32)
        cur = v.copy()
        cur[rng.random((A, T)) < 0.1] = 0                       # absences
        cur[rng.random((A, T)) < 0.02] = -7
        jump = rng.random((A, T)) < 0.05
        cur[jump] += 40000                                       # escapes up, and back down in the next round
        if r == 3:
            cur.reshape(-1)[0] = np.iinfo(np.int32).max
        skip = (rng.random(T) < 0.3) if r % 3 == 2 else np.zeros(T, dtype=bool)
        rounds.append((cur, skip))
    fin, fout = tmp_path / "in.bin", tmp_path / "out.bin"
    with open(fin, "wb") as f:
        f.write(np.array([A, T, R], dtype=np.int32).tobytes())
        for cur, skip in rounds:
            f.write(cur.tobytes())
            f.write(skip.astype(np.uint8).tobytes())
    res = subprocess.run([driver, str(fin), str(fout)], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-3000:]
    raw = open(fout, "rb").read()
    pos = 0

    def take(dtype, count, shape):
        nonlocal pos
        a = np.frombuffer(raw, dtype=dtype, count=count, offset=pos).reshape(shape)
        pos += a.nbytes
        return a

    code = np.zeros((A, T), dtype=np.int16)
    mirror = np.zeros((A, T), dtype=np.int32)
    base = np.zeros((A, T), dtype=np.int32)
    out = np.full((A, T), 12345, dtype=np.int32)
    escapes = 0
    for r, (cur, skip) in enumerate(rounds):
        esc = d16.encode_into(code, mirror, cur, skip)
        d16.decode(code, esc, base, out, skip)
        c_code = take(np.int16, A * T, (A, T))
        n_esc = int(take(np.int32, 1, (1,))[0])
        c_esc = take(np.int32, 2 * n_esc, (n_esc, 2))
        c_out, c_base = take(np.int32, A * T, (A, T)), take(np.int32, A * T, (A, T))
        assert np.array_equal(code, c_code), f"codes, round {r}"
        assert np.array_equal(esc, c_esc), f"escape list, round {r}"
        assert np.array_equal(out, c_out) and np.array_equal(base, c_base) and np.array_equal(base, mirror), f"round {r}"
        assert np.array_equal(out, np.where(skip[None, :], 0, np.maximum(cur, 0))), f"round {r}"
        escapes += n_esc
    assert pos == len(raw) and escapes > 0
