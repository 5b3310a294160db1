"""kfpos_core_imu9.h has the 9-state step in two texts: step_imu9_state (covariance in registers from epoch to epoch) and
the phase functions step_imu9_head + step_imu9_state_parked (covariance in the park between two epochs: the epoch loop of
the bench kernel). tests/emu/imu9_phases.cpp runs one tag through sequences of epochs both ways on the host and compares
position, velocity, covariance and status word of every epoch as bytes, over every way a step can end; it also fails when
one of those ways was not taken. (CPU only.)"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_phase_functions_leave_the_bytes_of_step_imu9_state(tmp_path):
    exe = str(tmp_path / "imu9_phases")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe,
                           os.path.join(ROOT, "tests", "emu", "imu9_phases.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stdout + res.stderr
    assert "the same bytes" in res.stdout, res.stdout
