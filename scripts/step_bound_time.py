#!/usr/bin/env python3
"""Wall time per step of the Lazy step glue alone (the solve excluded), two ways on the same workload:

  (a) per call — what a caller had to do before the resident table: fetch the touched variables, build the
      slot -> dense map on the host (step.dense_index), upload the whole table and its lazy state again, and pass
      the modified set as a host list;
  (b) resident — one bound table for the run (lmmhip_actions_bind): patch the actions the step changed and take
      the modified set on the device (lmmhip_actions_lazy_update_solved).

Workload: the bench's C2 generator (lmm_gen_synthetic) at 1/`--div` of its size, resident System, one Lazy CM02
action per variable, `--updates` penalty updates per step.  Two Systems get the same mutations (a context holds
one table); every step both solve (not timed), then both glues are timed, in alternating order.  After `--warmup`
steps, `--steps` timed ones; the result (median, min, max, every sample) goes to `--out` as JSON.

    python scripts/step_bound_time.py --div 10 --out profiles/step_bound.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(ms):
    ms = sorted(ms)
    return dict(median_ms=ms[len(ms) // 2], min_ms=ms[0], max_ms=ms[-1], samples_ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--div", type=int, default=10, help="1/div of C2 (1e6 constraints x 1e7 variables x 8)")
    ap.add_argument("--updates", type=int, default=1000)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "step_bound.json"))
    args = ap.parse_args()
    from simgrid_amd import lmm, step as D

    nc, nv = 1_000_000 // args.div, 10_000_000 // args.div
    systems, slots = [], None
    for _ in range(2):
        s = lmm.System(False)
        assert s.resident()
        vs = s.gen_synthetic(nc, nv, 8, seed=1)
        systems.append(s)
        slots = np.asarray(vs, np.int32)
    rng = np.random.default_rng(1)
    n = len(slots)
    host = dict(remains=rng.random(n) * 1e9 + 1e6, max_duration=np.full(n, -1.0), latency=np.zeros(n),
                penalty=np.ones(n), sharing_penalty=np.ones(n), flags=np.zeros(n, np.uint8))
    lazy = dict(last_update=np.zeros(n), last_value=np.zeros(n), start_time=np.zeros(n), date=np.zeros(n),
                heap_type=np.zeros(n, np.uint8))
    sa, sb = systems
    for s in systems:
        s.solve()
    bound = D.DeviceActions(sb.device_ctx(), np.full(n, -1, np.int32), **host)
    bound.lazy_init(**lazy)
    bound.bind(slots)

    def glue_a(now):
        t = time.perf_counter()
        vi = D.dense_index(sa.device_touched_vars(), slots)
        acts = D.DeviceActions(sa.device_ctx(), vi, **host)
        acts.lazy_init(**lazy)
        acts.lazy_update(D.MODEL_CM02, now, np.nonzero(vi >= 0)[0], 1e-5, 1e-5)
        return (time.perf_counter() - t) * 1e3

    def glue_b(now, idx, pen):
        t = time.perf_counter()
        bound.patch(idx, penalty=pen)
        bound.lazy_update_solved(D.MODEL_CM02, now, (), 1e-5, 1e-5)
        return (time.perf_counter() - t) * 1e3

    ta, tb = [], []
    for step in range(args.warmup + args.steps):
        idx = rng.choice(n, args.updates, replace=False)
        pen = rng.random(args.updates) + 0.5
        for s in systems:  # the same mutation on both, then the solve (not timed)
            for i, p in zip(idx, pen):
                s.update_variable_penalty(lmm.Variable(s, int(slots[i])), float(p))
            s.solve()
        host["penalty"][idx] = pen
        now = 1e-3 * (step + 1)
        if step % 2:
            a, b = glue_a(now), glue_b(now, idx, pen)
        else:
            b = glue_b(now, idx, pen)
            a = glue_a(now)
        if step >= args.warmup:
            ta.append(a)
            tb.append(b)
        print(f"step {step}: per-call {a:.2f} ms, resident {b:.3f} ms", flush=True)
    st = sa.last_stats()
    out = dict(workload=f"C2 generator at 1/{args.div}: {nc} constraints x {nv} variables x 8, resident System, one Lazy"
                        f" CM02 action per variable, {args.updates} penalty updates per step; glue only, solve excluded",
               actions=n, solved_vars=st["n_var"], warmup=args.warmup, steps=args.steps,
               per_call=summary(ta), resident=summary(tb),
               per_call_is="touched-vars fetch + step.dense_index + lmmhip_actions_upload + _lazy_upload +"
                           " lmmhip_actions_lazy_update with a host list",
               resident_is="lmmhip_actions_patch of the changed penalties + lmmhip_actions_lazy_update_solved")
    sa_, sb_ = out["per_call"], out["resident"]
    out["resident_faster_beyond_spread"] = bool(sb_["max_ms"] < sa_["min_ms"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in out.items() if k in ("per_call", "resident", "resident_faster_beyond_spread")}))


if __name__ == "__main__":
    main()
