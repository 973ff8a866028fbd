"""Host side of the batched FairBottleneck engine (CPU only): the lmmhip_last_engine binding, and the LDS budget
fb_batch_lds_bytes (simgrid_amd/csrc/lmm_fb_batch_kernels.hpp) compiled into a small host program
(tests/c/fb_batch_lds_check.cpp).  The kernel itself is pinned by tests/test_gpu_fb_batch.py.
"""
import os
import re
import subprocess

import pytest

from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAP = 64 * 1024  # kBatchLdsMax (simgrid_amd/csrc/lmm_ctx.hpp)


def test_last_engine_is_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "lmm", "lmm_hip.h")).read()
    assert re.search(r"int lmmhip_last_engine\(lmmhip_ctx\* ctx, int\* engine\);", hdr)
    names = ["PERSISTENT", "ROUNDS", "FRONTIER", "BATCH", "FB_ROUNDS", "FB_BATCH"]
    vals = [int(re.search(rf"#define LMMHIP_RAN_{n} (\d+)", hdr).group(1)) for n in names]
    assert len(set(vals)) == 6
    assert vals == [getattr(L.System, "RAN_" + n) for n in names]
    assert "lmmhip_last_engine" in L.SIGNATURES
    assert hasattr(L.lib(), "lmmhip_last_engine")  # exported by the built library
    assert callable(L.System.last_engine) and callable(M.DeviceBatch.last_engine)


@pytest.fixture(scope="module")
def lds_bytes(tmp_path_factory):
    exe = tmp_path_factory.mktemp("fbb") / "fb_batch_lds_check"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "simgrid_amd", "csrc"), "-o", str(exe),
                           os.path.join(ROOT, "tests", "c", "fb_batch_lds_check.cpp")])

    def run(triples):
        args = [str(x) for t in triples for x in t]
        out = subprocess.run([str(exe)] + args, capture_output=True, text=True, check=True).stdout.split()
        return [(int(out[2 * i]), int(out[2 * i + 1])) for i in range(len(triples))]

    return run


def test_lds_bytes_is_monotone(lds_bytes):
    sizes = [0, 1, 2, 7, 8, 9, 63, 64, 255, 256, 257, 1000, 4097, 65534]
    base = (58, 30, 200)
    for arg in range(3):
        triples = [tuple(s if k == arg else base[k] for k in range(3)) for s in sizes]
        got = lds_bytes(triples)
        for (a, aw), (b, bw) in zip(got, got[1:]):
            assert a <= b and aw <= bw, (arg, got)
        assert got[0][0] < got[-1][0]
    for b, bw in lds_bytes([(0, 0, 0), (1, 1, 1), (58, 30, 200)]):
        assert b % 16 == 0 and bw >= b


def flat_sizes(s):
    f = M.export_flat(s)
    return len(f.penalty), len(f.cbound), len(f.cnst_idx)


def test_lds_bytes_fits_the_tested_systems_and_not_a_large_member(lds_bytes):
    FB = L.System.FAIR_BOTTLENECK
    sizes = []
    for seed, kw in [(1000, dict(zero_bound_p=0.0, fatpipe_p=0.1)), (1005, dict(zero_bound_p=0.05, fatpipe_p=0.0))]:
        ops = K.random_script(seed, conc_limits=True, frees=2, bound_updates=3, zero_w_p=0.0, **kw)
        sizes.append(flat_sizes(K.replay(L, ops, kind=FB)[0]))
    for kw in [dict(topology=L.FAT_TREE, topo_parameters="2;4,4;1,2;1,2", n_flows=64),
               dict(topology=L.DRAGONFLY, topo_parameters="3,4;4,3;5,1;2", n_flows=256, policy=L.SHARED),
               dict(topology=L.DRAGONFLY, topo_parameters="3,4;4,3;5,1;2", n_flows=256, policy=L.FATPIPE)]:
        s = L.System(False, FB)
        s.gen_platform_flows(L.platform_params(model=L.L07, seed=1, **kw))
        sizes.append(flat_sizes(s))
    assert max(s[1] for s in sizes) > 256  # the dragonfly systems: more constraints than a workgroup has threads
    for (b, bw), sz in zip(lds_bytes(sizes), sizes):
        assert 0 < b <= CAP, (sz, b)
    # a member of 65,535 elements does not fit whatever its other sizes (and the driver refuses such sizes anyway)
    for b, _ in lds_bytes([(1, 1, 65535), (65535, 1, 65535), (70000, 80, 140000)]):
        assert b > CAP
