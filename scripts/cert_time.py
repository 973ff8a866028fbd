#!/usr/bin/env python3
"""Times the max-min certificate of a solved C2 system (gen_synthetic, as bench.py builds it) two ways, alternating in
one process after a warm-up:

  (a) lmmhip_certificate: the device pass (cert_cnst, cert_var, cert_fold) over the values in HBM, host clock around
      the call (it ends in its own stream synchronise), counts only and with the witness array;
  (b) lmm_fetch then lmm_check_certificate: the host walk over the fetched values, the only way to the same three
      numbers without the device pass (after a solve of its own, which is not timed: a resident system's values are
      fetched once per solve).

and checks that (a) returns exactly the counts of (b).

  python scripts/cert_time.py --div 10 --out profiles/cert_time.json             # 1/10 of C2 (add --full for C2 too)
  rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o run -- python scripts/cert_time.py --div 10 --trace-run
  python scripts/cert_time.py --merge-stats DIR/run_kernel_stats.csv --out profiles/cert_time.json

The second line is a run of its own (solve, then --reps certificate calls) for the per-kernel split; the third folds
its cert_* rows into the JSON the first wrote.

Byte model (what the pass has to move, from the shapes; the file quotes GB/s against it):
  cert_cnst  per element 12 B of CSC stream (csc_w, csc_v) + two 8-B gathers (x, pen); per constraint 8 B cnst_ptr +
             1 B cflags + 8 B cbound + 8 B sattop store;
  cert_var   per element 4 B of CSR stream (csr_c) + one 8-B gather (sattop); per variable 4 B var_ptr + 24 B x, pen,
             vbound (+ 4 B witness store when asked for).
"""
import argparse
import csv
import ctypes as ct
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ts):
    ms = [t * 1e3 for t in ts]
    return dict(min_ms=min(ms), median_ms=statistics.median(ms), max_ms=max(ms), reps=len(ms))


def model_bytes(nv, nc, nnz, witness):
    return dict(csc_stream=12 * nnz + 25 * nc, gathers=16 * nnz + 8 * nnz, csr_stream=4 * nnz + (32 if witness else 28) * nv)


def measure(nc, nv, args):
    import numpy as np

    from simgrid_amd import lmm

    lib, prec = lmm.lib(), lmm.get_precision()
    t = time.time()
    s = lmm.System(False)
    s.gen_synthetic(nc, nv, 8, seed=1, want_vars=False)
    s.prepare()
    s.device_solve()
    st, ctx = s.last_stats(), s.device_ctx()
    out = dict(n_var=st["n_var"], n_cnst=st["n_cnst"], nnz=st["nnz"], engine=s.last_engine(),
               solve_device_ms=st["device_ms"], build_s=round(time.time() - t, 1))
    cert = lmm.LmmhipCert()
    wit = np.empty(st["n_var"], np.int32)

    def device(witness):
        lmm._check_hip(lib.lmmhip_certificate(ctx, prec, ct.byref(cert),
                                              wit.ctypes.data_as(ct.POINTER(ct.c_int32)) if witness else None))
        return cert.max_excess, cert.n_infeasible, cert.n_unbottlenecked

    def host():
        # (a resident system's values are fetched once per solve: solve again, untimed, then time fetch + walk)
        s.prepare()
        s.device_solve()
        t0 = time.perf_counter()
        s.fetch()
        r = s.check_certificate(prec)
        return r, time.perf_counter() - t0

    if args.trace_run:
        for _ in range(args.reps):
            device(False)
        return out
    for _ in range(args.warmup):
        device(False), device(True)
    h, _ = host()
    ta, tw, tb = [], [], []
    for i in range(args.reps):
        t0 = time.perf_counter()
        a = device(False)
        t1 = time.perf_counter()
        device(True)
        t2 = time.perf_counter()
        ta.append(t1 - t0)
        tw.append(t2 - t1)
        if i < args.host_reps:
            h, dt = host()
            tb.append(dt)
    out["device_certificate"] = summary(ta)
    out["device_certificate_with_witness"] = summary(tw)
    out["fetch_then_check_certificate"] = summary(tb)
    out["device"] = dict(max_excess=a[0], n_infeasible=a[1], n_unbottlenecked=a[2], n_judged_cnst=cert.n_judged_cnst,
                         n_judged_var=cert.n_judged_var, n_at_bound=cert.n_at_bound)
    out["host"] = dict(max_excess=h[0], n_infeasible=h[1], n_unbottlenecked=h[2])
    out["counts_equal"] = a[1:] == h[1:]
    for key, witness in (("device_certificate", False), ("device_certificate_with_witness", True)):
        by = model_bytes(st["n_var"], st["n_cnst"], st["nnz"], witness)
        by["total"] = sum(by.values())
        by["gb_per_s"] = by["total"] / (out[key]["median_ms"] * 1e-3) / 1e9
        out[key]["byte_model"] = by
    out["speedup_median"] = out["fetch_then_check_certificate"]["median_ms"] / out["device_certificate"]["median_ms"]
    assert out["counts_equal"], (a, h)
    return out


def merge_stats(path, out_path):
    with open(out_path) as fh:
        doc = json.load(fh)
    rows = {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            if "cert_" in r["Name"]:
                rows[r["Name"].split("(")[0]] = dict(calls=int(r["Calls"]), total_ns=float(r["TotalDurationNs"]),
                                                     avg_us=float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3)
    doc["kernel_trace"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own (--trace-run)", kernels=rows)
    with open(out_path, "w") as fh:
        json.dump(doc, fh, indent=1)
    print(json.dumps(doc["kernel_trace"]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cnst", type=int, default=1_000_000)
    ap.add_argument("--vars", type=int, default=10_000_000)
    ap.add_argument("--div", type=int, default=10, help="the C2 generator at 1/div size")
    ap.add_argument("--full", action="store_true", help="... and at full size")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-reps", type=int, default=10, help="repetitions of the host path (seconds each at full size)")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-run", action="store_true", help="solve and --reps certificate calls only (for rocprofv3)")
    ap.add_argument("--merge-stats", default=None, metavar="CSV", help="fold a kernel-stats CSV into --out")
    args = ap.parse_args()
    if args.merge_stats:
        return merge_stats(args.merge_stats, args.out)
    import torch

    assert torch.cuda.is_available(), "needs an MI355X"
    torch.cuda.set_device(0)
    doc = dict(runs=[])
    for div in [args.div] + ([1] if args.full else []):
        r = measure(args.cnst // div, args.vars // div, args)
        r["scale"] = f"C2 / {div}"
        doc["runs"].append(r)
        print("RESULT " + json.dumps(r), flush=True)
        if args.out and not args.trace_run:  # after every size: a later failure keeps what was measured
            with open(args.out, "w") as fh:
                json.dump(doc, fh, indent=1)


if __name__ == "__main__":
    main()
