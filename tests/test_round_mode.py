"""The mode resolution of the round engine (simgrid_amd/csrc/lmm_round_mode.hpp), checked on the CPU.

A round-engine solve runs in one of nine vote modes (what a re-vote reads its row from, the ready queue, the sat-key
filter) and one of four update modes; round_plan (lmm_hip_maxmin.hip) resolves them from the knobs' values and indexes
the kernel tables, which are built by enumerating the mode indices, with the mode's own index.
tests/c/round_mode_check.cpp keeps the resolution round_plan had before — loose bools and positions in two hand-written
tables — literally, and replays it next to the header's functions over group sizes, knob values, CU counts and
constraint counts around every boundary; which kernels then run on the device is pinned by
tests/test_gpu_engine_scripts.py::test_every_round_mode_matches_the_default.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_round_mode_matches_the_former_resolution(tmp_path):
    exe = tmp_path / "round_mode_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "c", "round_mode_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000, out.stdout
