"""The chunk policy of the round-chain engines (simgrid_amd/csrc/lmm_chunk.hpp), checked on the CPU.

The round engine and the frontier engine queue a chunk of rounds per termination poll; both take the chunk lengths from
one policy (first chunk, doubling up to a maximum, the cut at the previous solve's round count, the round engine's
short tail chunks), driven by run_chunks (lmm_hip_maxmin.hip).  tests/c/chunk_policy_check.cpp keeps the arithmetic of
the two loops the engines had before, literally, and replays it next to the shared one over hints that are exact, short,
long and absent, on a model of the one-chunk-late polls; the device side is pinned by the launch counts of
tests/test_gpu_engine_scripts.py::test_round_chain_launch_sequence.
"""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_chunk_policy_matches_the_two_former_loops(tmp_path):
    exe = tmp_path / "chunk_policy_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "c", "chunk_policy_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 10000, out.stdout
