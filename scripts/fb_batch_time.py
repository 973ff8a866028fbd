#!/usr/bin/env python3
"""Batched FairBottleneck engine against the chunked engine on the same resident union.

Two workloads, each uploaded once through multi.DeviceBatch(kind=FAIR_BOTTLENECK):
  (a) 4,096 L07 systems: 64 flows on the 16-host fat tree "2;4,4;1,2;1,2", seeds 1..4096
  (b) the 40 random systems of tests/test_gpu_parity.py::test_random_fair_bottleneck_vs_oracle
Each is solved 5 + 20 times by the batch engine (one workgroup per system, lmm_fb_batch_kernels.hpp) and 5 + 20 times
with LMMHIP_BATCH=0 (the chunked engine on the union, lmm_fb_kernels.hpp: what lmm_solve_batch ran before the batch
engine existed), in this process on this device; device_ms is the solve's own event pair.  Prints and writes
(--out, default profiles/fb_batch_timing.json) the median and the spread (min, max) of the 20, and whether the
batch engine is faster by more than the two spreads together.

  python scripts/fb_batch_time.py [--systems 4096] [--warmup 5] [--solves 20] [--out FILE]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from simgrid_amd import lmm as L  # noqa: E402
from simgrid_amd import multi as M  # noqa: E402
from tests import lmm_cases as K  # noqa: E402
from tests.test_gpu_parity import FB_FATPIPE_SEEDS  # noqa: E402

FB = L.System.FAIR_BOTTLENECK


def l07_systems(n):
    out = []
    for seed in range(1, n + 1):
        s = L.System(False, FB)
        s.gen_platform_flows(L.platform_params(topology=L.FAT_TREE, topo_parameters="2;4,4;1,2;1,2", model=L.L07,
                                               n_flows=64, seed=seed), want_vars=False)
        out.append(s)
    return out


def random_systems():
    out = []
    for variant in ("fatpipe", "zero_bounds"):
        for i in range(20):
            seed = FB_FATPIPE_SEEDS[i] if variant == "fatpipe" else i
            kw = (dict(zero_bound_p=0.0, fatpipe_p=0.1) if variant == "fatpipe"
                  else dict(zero_bound_p=0.05, fatpipe_p=0.0))
            ops = K.random_script(1000 + seed, conc_limits=(seed % 3 == 0), frees=2, bound_updates=3, zero_w_p=0.0,
                                  **kw)
            out.append(K.replay(L, ops, kind=FB)[0])
    return out


def timed(b, batch, warmup, solves):
    if batch:
        os.environ.pop("LMMHIP_BATCH", None)
    else:
        os.environ["LMMHIP_BATCH"] = "0"
    ms = []
    for i in range(warmup + solves):
        b.solve()
        if i >= warmup:
            ms.append(b.stats()["device_ms"])
    want = L.System.RAN_FB_BATCH if batch else L.System.RAN_FB_ROUNDS
    assert b.last_engine() == want, (b.last_engine(), want)
    os.environ.pop("LMMHIP_BATCH", None)
    ms = np.array(ms)
    return dict(median_ms=float(np.median(ms)), min_ms=float(ms.min()), max_ms=float(ms.max()),
                spread_ms=float(ms.max() - ms.min()), rounds=int(b.stats()["rounds"])), b.values()


def measure(name, systems, warmup, solves):
    b = M.DeviceBatch(systems, kind=M.DeviceBatch.FAIR_BOTTLENECK)
    r = dict(workload=name, systems=len(systems), n_var=b.n_var, n_cnst=b.n_cnst, nnz=b.nnz)
    r["batch"], xb = timed(b, True, warmup, solves)
    r["chunked"], xc = timed(b, False, warmup, solves)
    r["same_bytes"] = xb.tobytes() == xc.tobytes()
    r["speedup"] = r["chunked"]["median_ms"] / r["batch"]["median_ms"]
    r["faster_beyond_spreads"] = (r["chunked"]["median_ms"] - r["batch"]["median_ms"] >
                                  r["chunked"]["spread_ms"] + r["batch"]["spread_ms"])
    b.close()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--systems", type=int, default=4096)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--solves", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fb_batch_timing.json"))
    a = ap.parse_args()
    res = dict(build_id=L.build_id(), warmup=a.warmup, solves=a.solves, workloads=[
        measure("a: L07 fat tree, 64 flows", l07_systems(a.systems), a.warmup, a.solves),
        measure("b: 40 random systems", random_systems(), a.warmup, a.solves)])
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
