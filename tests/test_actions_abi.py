"""The resident action table's ABI (CPU only): declared in the header and in lmm.SIGNATURES, exported, refusing a
missing context with a message instead of crashing, and usable from a C99 client."""
import ctypes as ct
import os
import re
import subprocess

import pytest

from simgrid_amd import lmm as L
from simgrid_amd import step as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("lmmhip_actions_bind", "lmmhip_actions_patch", "lmmhip_actions_lazy_update_solved", "lmmhip_actions_events",
       "lmmhip_actions_var_index")
E_ARG = -3


def header():
    return open(os.path.join(ROOT, "include", "lmm", "lmm_hip.h")).read()


@pytest.mark.parametrize("name", NEW)
def test_declared_bound_and_exported(name):
    code = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    assert name in L.SIGNATURES
    n_args = len(re.search(r"\b%s\s*\(([^)]*)\)" % name, code).group(1).split(","))
    assert n_args == len(L.SIGNATURES[name][1]), name  # the binding passes what the header declares
    assert hasattr(ct.CDLL(L.LIB_PATH), name)


def test_patch_field_bits_match_the_header():
    code = header()
    for field, (bit, _) in D.PATCH_FIELDS.items():
        m = re.search(r"#define LMMHIP_ACT_F_%s (\d+)" % field.upper(), code)
        assert m and int(m.group(1)) == bit, field
    assert len({bit for bit, _ in D.PATCH_FIELDS.values()}) == 12


@pytest.mark.parametrize("name", NEW)
def test_missing_context_is_refused_with_a_message(name):
    """What a caller without a device ends up doing: lmmhip_ctx_create gave it no context."""
    lib = L.lib()
    args = [None if a is L.P or hasattr(a, "contents") else 0 for a in L.SIGNATURES[name][1]]
    assert getattr(lib, name)(*args) == E_ARG
    assert b"null" in lib.lmmhip_last_error()


def test_python_wrappers_report_the_library_error():
    class NoCtx(D.DeviceActions):
        def __init__(self):
            self.ctx, self.n, self.L = None, 2, L.lib()

    acts = NoCtx()
    for call in (lambda: acts.bind([0, 1]), lambda: acts.patch([0], remains=1.0), lambda: acts.events(),
                 lambda: acts.var_index(), lambda: acts.lazy_update_solved(D.MODEL_CPU, 0.0, [1])):
        with pytest.raises(L.LmmError, match="null"):
            call()
    with pytest.raises(TypeError, match="unknown field"):
        acts.patch([0], remain=1.0)


def test_c_client_compiles_and_is_refused_cleanly():
    """The C99 client of the new calls compiles against the header with -Werror, links the library and runs (no
    device needed: it has no context to pass); the existing client (tests/c/abi_drive.c) still compiles."""
    from tests import test_abi

    lib_dir = os.path.dirname(L.LIB_PATH)
    exe = os.path.join(ROOT, "tests", "c", "actions_abi_drive")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "include"),
                           exe + ".c", "-o", exe, "-L", lib_dir, "-llmm_amd", "-Wl,-rpath," + lib_dir, "-lm"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and out.stdout.strip() == "ok", (out.returncode, out.stdout, out.stderr)
    assert os.path.exists(test_abi.build_c_drive())
