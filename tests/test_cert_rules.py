"""The rules of the max-min certificate (simgrid_amd/csrc/lmm_cert.hpp), checked on the CPU.

System::check_certificate (the host walk) and cert_cnst / cert_var (the device pass, lmmhip_certificate) decide from one
set of inline predicates.  tests/c/cert_rules_check.cpp keeps the comparisons check_certificate wrote out before the
header existed, literally, and replays them next to the header's functions over inputs on both sides of every
threshold; what the device then computes with them is pinned by tests/test_gpu_certificate.py.  Also here: the calls'
answers where there is nothing to certify, which need no device.
"""
import ctypes as ct
import os
import subprocess

import pytest

from simgrid_amd import lmm as L
from tests import lmm_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "c", "cert_rules_check.cpp")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def test_rules_match_the_former_comparisons(tmp_path):
    exe = tmp_path / "cert_rules_check"
    base = ["g++", "-O2", "-std=c++17", "-Wall", "-o", str(exe), SRC]
    # under the address and undefined-behaviour sanitizers where this g++ links them, else plain
    if subprocess.run(base + SAN, capture_output=True).returncode != 0:
        subprocess.check_call(base)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    assert int(out.stdout.split()[1]) > 1000, out.stdout


def test_null_context_is_a_state_error():
    cert = L.LmmhipCert()
    assert L.lib().lmmhip_certificate(None, 1e-5, ct.byref(cert), None) == -4  # LMMHIP_E_STATE
    assert b"no solved system" in L.lib().lmmhip_last_error()


def test_before_any_solve():
    s, _, _ = K.replay(L, K.random_script(0, frees=3, penalty_updates=4, bound_updates=4))
    ex, ni, nu = L.D(), L.I64(), L.I64()
    assert L.lib().lmm_device_certificate(s.h, 1e-5, ct.byref(ex), ct.byref(ni), ct.byref(nu)) == -1
    assert b"no device solve" in L.lib().lmm_last_error()
    assert L.lib().lmm_device_bottlenecks(s.h, None, None, 0) == -1
    assert b"no device solve" in L.lib().lmm_last_error()
    with pytest.raises(L.LmmError, match="no device solve"):
        s.device_certificate()
    with pytest.raises(L.LmmError, match="no device solve"):
        s.device_bottlenecks()
