#!/usr/bin/env python3
"""Times the device usage pass (mm_usage behind lmmhip_usage_device_ptr) and lmmhip_get_saturated on the SURVEY.md
§8(d) configurations, as bench.py builds them: C2 (gen_synthetic 1e6 x 1e7 x 8), C4 (1e5 LV08 flows, fat tree) and C5
(L07 flows on the dragonfly, FairBottleneck).

One process per (configuration, library): the library is chosen when simgrid_amd.lmm is imported (LMM_AMD_LIB), so
the driver starts the children one after the other, alternating an older build (--old LIB, e.g. the parent commit's
liblmm_amd.so) with this tree's: old, new, old, new ...  The spread between the runs of the same library is what a
difference between the two has to exceed.  Each child builds the system, solves it once, warms the timed calls up
and reports, per call, the median / min / max / standard deviation over --reps repetitions of the host clock around
the call plus a stream synchronise (both calls below end on the context's stream; lmmhip_get_saturated synchronises
itself and includes its n_cnst-byte copy to the host).

  python scripts/usage_pass_time.py --old build_ab/parent/liblmm_amd.so --out profiles/usage_pass.json

Byte model of the usage pass (printed with the result): per element 8 B csc_w + 4 B csc_v streamed + one 8-B gather of
x, per constraint 8 B cnst_ptr (two 4-B reads) + 1 B cflags + 8 B store: "20 B per element streamed" counts the
gather's 8 useful bytes.
"""
import argparse
import ctypes as ct
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

C4_PLATFORM = dict(topology=0, topo_parameters="3;16,16,16;1,16,16;1,1,1", loopback_bw=1e8)
C5_PLATFORM = dict(topology=1, topo_parameters="8,4;16,3;8,2;4", loopback_bw=1e9, limiter_bw=2e8)


def summary(ts):
    ms = [t * 1e3 for t in ts]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
                sd_ms=statistics.pstdev(ms), reps=len(ms))


def child(args):
    import numpy as np
    import torch

    from simgrid_amd import lmm

    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    lib = lmm.lib()
    t = time.time()
    if args.child == "c2":
        s = lmm.System(False)
        s.gen_synthetic(args.cnst, args.vars, 8, seed=1, want_vars=False)
    elif args.child == "c4":
        s = lmm.System(False)
        s.gen_platform_flows(lmm.platform_params(model=lmm.LV08, n_flows=args.c4_flows, seed=1, **C4_PLATFORM),
                             want_vars=False)
    else:
        s = lmm.System(False, lmm.System.FAIR_BOTTLENECK)
        s.gen_platform_flows(lmm.platform_params(model=lmm.L07, n_flows=args.c5_flows, seed=1, **C5_PLATFORM),
                             want_vars=False)
    s.prepare()
    s.device_solve()
    st = s.last_stats()
    ctx = s.device_ctx()
    # the stream is the caller's, so that the host can wait for it
    stream = torch.cuda.Stream()
    lmm._check_hip(lib.lmmhip_ctx_set_stream(ctx, ct.c_void_p(stream.cuda_stream)))
    out = dict(config=args.child, n_var=st["n_var"], n_cnst=st["n_cnst"], nnz=st["nnz"], engine=s.last_engine(),
               build_s=round(time.time() - t, 1), lib=os.environ.get("LMM_AMD_LIB") or "tree")
    cp = np.zeros(st["n_cnst"] + 1, np.uint32)  # the constraints' CSC offsets only (null arrays are skipped)
    lmm._check_hip(lib.lmmhip_flat_download(ctx, (ct.c_int64 * 3)(), None, None, None, cp.ctypes.data, None, None,
                                            None, None, None, None))
    deg = np.diff(cp.astype(np.int64))
    out["cnst_degree"] = dict(max=int(deg.max(initial=0)), median=float(np.median(deg)) if len(deg) else 0.0)

    sat = np.empty(st["n_cnst"], np.uint8)

    def saturated():
        lmm._check_hip(lib.lmmhip_get_saturated(ctx, sat.ctypes.data_as(ct.POINTER(ct.c_uint8))))

    dptr = ct.c_void_p()

    def usage():
        lmm._check_hip(lib.lmmhip_usage_device_ptr(ctx, ct.byref(dptr)))
        stream.synchronize()

    calls = {"get_saturated": saturated}
    if not os.environ.get("LMM_AMD_LIB"):  # (an older build does not have the usage pass)
        calls["usage_device_ptr"] = usage
    for name, fn in calls.items():
        for _ in range(args.warmup):
            fn()
        ts = []
        for _ in range(args.reps):
            stream.synchronize()
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        out[name] = summary(ts)
    out["saturated_count"] = int(np.count_nonzero(sat))
    if "usage_device_ptr" in calls:
        u = s.device_usage_dense()
        out["usage_sum"] = float(u.sum())
        nnz, nc = st["nnz"], st["n_cnst"]
        by = 20 * nnz + 17 * nc
        out["byte_model"] = dict(bytes=by, per_element=20, per_constraint=17,
                                 gb_per_s=by / (out["usage_device_ptr"]["median_ms"] * 1e-3) / 1e9,
                                 elements_per_s=nnz / (out["usage_device_ptr"]["median_ms"] * 1e-3))
    lmm._check_hip(lib.lmmhip_ctx_use_own_stream(ctx))
    print("RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", default=None, help="an older build of liblmm_amd.so to alternate with this tree's")
    ap.add_argument("--out", default=None, help="write the results here (JSON)")
    ap.add_argument("--configs", default="c2,c4,c5")
    ap.add_argument("--rounds", type=int, default=2, help="alternations old / new per configuration")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cnst", type=int, default=1_000_000)
    ap.add_argument("--vars", type=int, default=10_000_000)
    ap.add_argument("--c4-flows", type=int, default=100_000)
    ap.add_argument("--c5-flows", type=int, default=10_000_000)
    ap.add_argument("--child-timeout", type=int, default=420)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.child:
        return child(args)
    runs = []
    passthrough = ["--reps", str(args.reps), "--warmup", str(args.warmup), "--cnst", str(args.cnst), "--vars",
                   str(args.vars), "--c4-flows", str(args.c4_flows), "--c5-flows", str(args.c5_flows)]
    for cfg in args.configs.split(","):
        # FairBottleneck's saturated set does not use the reduction: nothing to compare with the older build there
        libs = ([args.old, None] if args.old and cfg != "c5" else [None]) * (args.rounds if cfg != "c5" else 1)
        for libpath in libs:
            env = dict(os.environ)
            env.pop("LMM_AMD_LIB", None)
            if libpath:
                env["LMM_AMD_LIB"] = os.path.abspath(libpath)
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", cfg] + passthrough, env=env,
                               capture_output=True, text=True, timeout=args.child_timeout)
            if r.returncode != 0:  # nothing more is started on the GPU after a failure
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                sys.exit(f"{cfg} ({libpath or 'tree'}) exited with {r.returncode}")
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1]
            runs.append(json.loads(line[len("RESULT "):]))
            print(line, flush=True)
            if args.out:  # after every run: a later failure keeps what was measured
                with open(args.out, "w") as fh:
                    json.dump(dict(runs=runs), fh, indent=1)


if __name__ == "__main__":
    main()
