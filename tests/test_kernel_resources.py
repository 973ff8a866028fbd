"""Register budget of the hot kernels (CPU only: hipcc cross-compiles gfx950 here).

The persistent max-min kernel runs one 1024-thread workgroup per CU, so it has 128 VGPRs per lane; a
change that pushes a round phase over that budget spills to scratch and costs the C4 solve ~45 %
(observed: 4.3 -> 6.3 ms when the re-vote kept 12 row elements in registers).  This test compiles the
solver with the compiler's resource report and requires zero VGPR spills / scratch for every round
kernel of both engines and the batch kernel.
"""
import os
import re
import subprocess
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "simgrid_amd", "csrc")
HOT = ("mm_persist", "mm_vote_lane", "mm_vote", "mm_ready", "mm_saturate", "mm_update", "mm_batch_lds",
       "mm_init_cnsts", "cmp_write", "fbk_", "fb_var_inc", "fr_")


def makefile_units():
    """The .hip translation units the Makefile builds and its HIPFLAGS (default ARCH, no EXTRA_HIPFLAGS)."""
    mk = open(os.path.join(CSRC, "Makefile")).read().replace("\\\n", " ")
    var = {k: v.strip() for k, v in re.findall(r"^(\w+) [:?]?= (.*)$", mk, re.M)}
    flags = var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"]).replace("$(EXTRA_HIPFLAGS)", "").split()
    units = [u + ".hip" for u in re.findall(r"\$\(OUT\)/(\w+)\.o", var["OBJS"])
             if os.path.exists(os.path.join(CSRC, u + ".hip"))]
    return units, flags


def unit_report(unit, flags):
    out = subprocess.run(["/opt/rocm/bin/hipcc"] + flags + ["-c", unit, "-o", os.devnull,
                                                           "-Rpass-analysis=kernel-resource-usage"],
                         cwd=CSRC, capture_output=True, text=True, check=True).stderr
    kernels, cur = {}, None
    for line in out.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            kernels[cur] = {}
            continue
        m = re.search(r"remark:\s+(VGPRs Spill|ScratchSize \[bytes/lane\]|VGPRs): (\d+)", line)
        if m and cur:
            kernels[cur][m.group(1)] = int(m.group(2))
    return kernels


_REPORTS = {}


def resource_report(extra=()):
    """Merged report of every unit (compiled once per set of extra flags), and the kernel names more than one unit
    reports."""
    if extra in _REPORTS:
        return _REPORTS[extra]
    units, flags = makefile_units()
    assert "lmm_hip.hip" in units and "-ffp-contract=off" in flags, (units, flags)
    flags = flags + list(extra)
    with ThreadPoolExecutor(4) as ex:
        reports = list(ex.map(lambda u: unit_report(u, flags), units))
    kernels, twice = {}, []
    for unit, rep in zip(units, reports):
        twice += [(k, unit) for k in rep if k in kernels]
        kernels.update(rep)
    _REPORTS[extra] = (kernels, twice)
    return kernels, twice


def test_hot_kernels_do_not_spill():
    kernels, twice = resource_report()
    # every __global__ kernel is compiled in exactly one translation unit
    assert not twice, twice
    hot = {k: v for k, v in kernels.items() if any(h in k for h in HOT)}
    assert any("mm_persist" in k for k in hot) and any("mm_saturate" in k for k in hot), sorted(kernels)
    # the report was parsed (a format change must not make this test pass vacuously)
    assert all("VGPRs" in v and "VGPRs Spill" in v for v in hot.values()), hot
    bad = {k: v for k, v in hot.items() if v.get("VGPRs Spill", 0) or v.get("ScratchSize [bytes/lane]", 0)}
    assert not bad, bad


def test_diagnostic_build_compiles_the_same_kernels():
    """The round-anatomy build (-DLMM_ANAT=1) compiles, unit by unit (unit_report raises on a compiler error), into
    exactly the product build's kernels, and LMM_ANAT is a preprocessor matter of lmm_dev.hpp alone: the kernels speak
    to the probe type defined there.  (Its register counts are not asserted: the stamps cost registers, and nobody
    times that build.)"""
    product, _ = resource_report()
    diag, twice = resource_report(("-DLMM_ANAT=1",))
    assert not twice, twice
    assert sorted(diag) == sorted(product), sorted(set(diag) ^ set(product))
    named = []
    for f in sorted(os.listdir(CSRC)):
        if f.endswith("_kernels.hpp") or f.endswith(".hip"):
            for n, line in enumerate(open(os.path.join(CSRC, f)), 1):
                if line.lstrip().startswith("#") and "LMM_ANAT" in line:
                    named.append((f, n, line.strip()))
    assert not named, named
