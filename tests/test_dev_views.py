"""Which engine's kernels can name which device fields (simgrid_amd/csrc/lmm_dev.hpp), checked on the CPU.

Every kernel takes the system by value: as a Dev (the flattened system and the max-min state the engines share), or as
its engine's view, FrDev (Dev + the frontier engine's eight fields) or FbDev (Dev + FairBottleneck's nineteen).
tests/c/dev_views_check.hip is static_asserts only — Dev has none of the 27 fields, each view has its own and none of
the other's, both are trivially copyable, sizeof(Dev) shrank — compiled here with the Makefile's flags and
-fsyntax-only; that the driver keeps nothing of the former conventions is a search of its sources.
"""
import os
import re
import subprocess

from tests.test_kernel_resources import CSRC, ROOT, makefile_units


def test_dev_views_static_asserts():
    _, flags = makefile_units()
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-fsyntax-only",
                                                           os.path.join(ROOT, "tests", "c", "dev_views_check.hip")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    sizes = set(re.findall(r"DevViewSizes<(\d+), (\d+), (\d+)>", out.stderr))
    assert len(sizes) == 1, out.stderr
    dev, fr, fb = map(int, sizes.pop())
    print(f"sizeof: Dev {dev}, FrDev {fr}, FbDev {fb} (Dev with every engine's fields: 720)")
    assert (dev, fr, fb) == (504, 568, 656)  # (the figures DESIGN.md quotes)


def test_no_engine_field_goes_through_the_context_dev():
    """No guard or hand-written nulling of another engine's pointer is left, and the 32-bit keys are named by frontier
    code alone (mm_init_cnsts takes them as an argument)."""
    found = []
    for f in sorted(os.listdir(CSRC)):
        if not f.endswith((".hip", ".hpp", ".cpp")):
            continue
        for n, line in enumerate(open(os.path.join(CSRC, f)), 1):
            for pat in ("HprogOff", "c->d.mu_p", "c->d.xnb", "c->d.xmin", "c->d.hprog"):
                if pat in line:
                    found.append((f, n, pat))
            if "s.key32" in line and f != "lmm_frontier_kernels.hpp":
                found.append((f, n, "s.key32"))
    assert not found, found
