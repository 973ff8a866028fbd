"""The key window of the max-min round kernels (simgrid_amd/csrc/lmm_keywin.hpp), checked on the CPU.

The round kernels compare constraints by 16-bit keys first and by exact fp64 ratios only where the keys tie.  A key is
the code of the ratio's f32 bits in a window {base, shift} that the round engine chooses on the device from each
solve's initial ratios; the persistent and batch engines keep the window {0, 16}, the f32's upper 16 bits.  Results do
not depend on the window as long as the map is monotone, which tests/c/keywin_check.cpp checks over denormals, values
below, inside and above the window, FLT_MAX and +inf, together with the bound on the codes (below kSatKey), the
identity of {0, 16} with the former key, the window's resolution on the C2 range and the shift selection on
degenerate ranges.  The device side is pinned by tests/test_gpu_keywin.py.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan-ubsan"])
def test_key_window_map_and_choice(tmp_path, flags):
    exe = tmp_path / "keywin_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall"] + flags +
                          ["-o", str(exe), os.path.join(ROOT, "tests", "c", "keywin_check.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert out.stdout.startswith("ok "), out.stdout
    _, checks, width, legacy = out.stdout.split()
    print(f"relative code width on [1e-4, 0.4]: window {float(width):.3g}, legacy {float(legacy):.3g}")
    assert int(checks) > 100000, out.stdout
    # 16 bits over the C2 range's 12 binades: at least 4 more mantissa bits than the legacy key's 7
    assert float(width) <= float(legacy) / 16, out.stdout
