"""Pin the oracle (CPU restatement) against the reference's own golden outputs and unit tests.

Goldens: tests/golden/maxmin_bench_{small,medium,large}.json, extracted by
tests/golden/make_golden.py from teshsuite/surf/maxmin_bench/*.tesh.  KATs: the 8 SECTIONs of
src/kernel/lmm/maxmin_test.cpp and lmm_usage.cpp's analytic answers.
"""
import json
import os

import pytest

from oracle import pyoracle as O
from tests import lmm_cases as K

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load(name):
    with open(os.path.join(GOLD, f"maxmin_bench_{name}.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("name,klass", [("small", 0), ("medium", 1)])
def test_oracle_reproduces_maxmin_bench_goldens(name, klass):
    d = load(name)
    for r in d["runs"]:
        s = O.System(False)
        cs, vs, a, b = s.gen_maxmin_bench(klass, r["run"])
        # RNG stream (maxmin_bench.cpp:178, :80)
        assert (a, b) == (r["check_start"], r["check_solve"])
        # construction: element lists in print() order, weights, bounds, concurrency (staging)
        for rk, eq in r["constraints"].items():
            c = cs[int(rk) - 1]
            els = c.elements()
            assert [e[0] for e in els] == [t[0] for t in eq["elems"]]
            assert all(abs(e[1] - t[1]) <= K.GOLDEN_TOL for e, t in zip(els, eq["elems"]))
            assert abs(c.get_bound() - eq["bound"]) <= K.GOLDEN_TOL
        assert [v.rank for v in s.variables()] == [o[0] for o in r["objective"]]
        s.solve()
        # lmm_solve init state (maxmin.cpp:541)
        for rk, (u, rem, cur, mx, lim) in r["init"].items():
            c = cs[int(rk) - 1]
            st = c.init_state()
            assert st is not None
            assert abs(st[0] - u) <= K.GOLDEN_TOL and abs(st[1] - rem) <= K.GOLDEN_TOL
            assert c.concurrency() == (cur, mx, lim)
        # solution (print(), maxmin.cpp:476-484)
        for rk, (pen, val) in r["values"].items():
            v = vs[int(rk) - 1]
            assert abs(v.get_penalty() - pen) <= K.GOLDEN_TOL
            assert abs(v.get_value() - val) <= K.GOLDEN_TOL, (rk, v.get_value(), val)
        # progressive-filling rounds == distinct fixing levels of the trace
        assert s.last_rounds == r["distinct_set_levels"]


def test_oracle_large_rng_stream():
    d = load("large")
    s = O.System(False)
    _, _, a, b = s.gen_maxmin_bench(2, d["run"])
    assert (a, b) == (d["check_start"], d["check_solve"]) == (807, 812)


@pytest.mark.parametrize("kat", K.MAXMIN_TEST_KATS, ids=lambda f: f.__name__)
def test_oracle_maxmin_test_kats(kat):
    s, expect = kat(O)
    for v, x in expect:
        assert abs(v.get_value() - x) < 1e-5  # double_equals(.., sg_maxmin_precision)


@pytest.mark.parametrize("case", [K.lmm_usage_test1, K.lmm_usage_test2])
def test_oracle_lmm_usage(case):
    s, expect = case(O)
    for v, x in expect:
        assert abs(v.get_value() - x) < 1e-9


def test_oracle_feasible_and_bottlenecked_on_random():
    # The max-min certificate, independent of any implementation: every constraint holds
    # (print()'s assertion, maxmin.cpp:470-471) and every positive variable is either at its bound
    # or has a saturated constraint on which no other variable has a larger level x*p.
    for seed in range(20):
        ops = K.random_script(seed, fatpipe_p=0.0)
        s, cs, vs = K.replay(O, ops)
        s.solve()
        prec = O.get_precision()
        for c in cs.values():
            if not (c.get_bound() > c.get_bound() * prec):
                continue  # skipped by lmm_solve (maxmin.cpp:524): a zero-bound constraint is ignored
            assert not (c.get_usage() - c.get_bound() > c.get_bound() * prec)


@pytest.mark.parametrize("kat", K.FB_TESH_KATS, ids=lambda f: f.__name__)
def test_oracle_fair_bottleneck_tesh_kats(kat):
    """Pin the FairBottleneck restatement (fair_bottleneck.cpp:23-153) on the answers the reference's L07
    tesh files print (examples/s4u/exec-ptask, teshsuite/simdag/comm-mxn-*, comm-p2p-latency-bound)."""
    _, expect = kat(O)
    assert not K.check_fb_kat(expect)


# ---- power-of-two scaling of the bounds (domain and magnitudes) -------------------------------------
# Multiplying every bound by 2^k is exact in fp64, and max-min is homogeneous in the bounds: the solution of the
# scaled script is ldexp(x, k).  The reference semantics keep that relation bit for bit upwards; downwards only
# without variable bounds (test_oracle_downward_scaling_with_bounded_variables_is_not_exact).  The device tests of
# tests/test_gpu_magnitudes.py rest on what is pinned here.
import functools  # noqa: E402

import numpy as np  # noqa: E402

SCALE_SCRIPTS = [("30x60", dict(frees=3, penalty_updates=4, bound_updates=4)),
                 ("300x3000", dict(n_cnst=300, n_var=3000, max_el=12, frees=20, penalty_updates=30, bound_updates=30))]


def _oracle_solution(ops):
    s, cs, vs = K.replay(O, ops)
    s.solve()
    keys = sorted(vs)
    return np.array([vs[k].get_value() for k in keys]), s.last_rounds, K.saturated(s, cs, O.get_precision()), vs


@functools.lru_cache(maxsize=None)
def _unscaled_solution(name, seed, unbounded):
    kw = dict(SCALE_SCRIPTS)[name]
    return _oracle_solution(K.unbounded_script(seed, **kw) if unbounded else K.random_script(seed, **kw))[:3]


def _check_oracle_scaling(name, seeds, unbounded, k):
    kw = dict(SCALE_SCRIPTS)[name]
    for seed in seeds:
        ops = K.unbounded_script(seed, **kw) if unbounded else K.random_script(seed, **kw)
        assert not unbounded or not any(op[0] == "vbound" or (op[0] == "var" and op[3] > 0) for op in ops)
        x0, r0, sat0 = _unscaled_solution(name, seed, unbounded)
        assert np.count_nonzero(x0) > 0
        x, r, sat, _ = _oracle_solution(K.scale_script(ops, k))
        assert x.tobytes() == np.ldexp(x0, k).tobytes(), (seed, k)
        assert r == r0 and sat == sat0, (seed, k)


# the 30 x 60 scripts: seeds 0..39 per case; the 300 x 3000 scripts: one seed (0..11) per case
SCALE_CASES = [("30x60", tuple(range(40)))] + [("300x3000", (seed,)) for seed in range(12)]
SCALE_IDS = [n if len(sd) > 1 else f"{n}-{sd[0]}" for n, sd in SCALE_CASES]


@pytest.mark.parametrize("k", (40, 150, 900))
@pytest.mark.parametrize("name,seeds", SCALE_CASES, ids=SCALE_IDS)
def test_oracle_upward_scaling_is_exact(name, seeds, k):
    _check_oracle_scaling(name, seeds, False, k)


@pytest.mark.parametrize("k", (-40, -160, -900))
@pytest.mark.parametrize("name,seeds", SCALE_CASES, ids=SCALE_IDS)
def test_oracle_downward_scaling_without_variable_bounds_is_exact(name, seeds, k):
    _check_oracle_scaling(name, seeds, True, k)


def test_oracle_downward_scaling_with_bounded_variables_is_not_exact():
    """The known exception: maxmin.cpp fixes a variable of the saturated set at its bound when
    double_equals(min_bound, bound * penalty, sg_maxmin_precision), an ABSOLUTE window of 1e-5.  Scaled down by 2^-40
    every bound level lies inside that window, every bounded variable of a saturated set is fixed at its bound, and the
    solution is no longer the scaled one.  (The device compares bound levels exactly; its tests scale downward only
    scripts without variable bounds.)"""
    name, kw = SCALE_SCRIPTS[1]
    ops = K.random_script(4, **kw)
    x0, r0, _, _ = _oracle_solution(ops)
    x, r, _, _ = _oracle_solution(K.scale_script(ops, -40))
    assert x.tobytes() != np.ldexp(x0, -40).tobytes()
    # upward the same script is exact (test_oracle_upward_scaling_is_exact): the window, not the scaling, is the cause


def test_scale_and_spread_scripts_touch_bounds_only():
    ops = K.random_script(3, n_cnst=40, n_var=120, frees=5, penalty_updates=8, bound_updates=12)
    up, sp = K.scale_script(ops, 7), K.spread_script(ops, 1, 80)
    assert len(up) == len(sp) == len(ops)
    e_c, seen = {}, 0
    for a, b, c in zip(ops, up, sp):
        assert a[0] == b[0] == c[0] and a[1] == b[1] == c[1]
        t = a[0]
        if t == "cnst" or t == "cbound" or t == "vbound":
            assert b[2] == a[2] * 128.0
            ratio = c[2] / a[2] if a[2] > 0 else 1.0
        elif t == "var":
            assert b[2] == a[2] and b[4] == a[4] and c[2] == a[2] and c[4] == a[4]
            assert b[3] == (a[3] * 128.0 if a[3] > 0 else -1.0)
            ratio = c[3] / a[3] if a[3] > 0 else 1.0
            assert a[3] > 0 or c[3] == -1.0
        else:
            assert a == b == c  # weights, penalties, frees, shares, limits
            continue
        e = np.log2(ratio)
        assert e == int(e) and 0 <= e <= 80
        if t in ("cnst", "cbound") and a[2] > 0:  # one exponent per constraint
            assert e_c.setdefault(a[1], e) == e
        seen += e > 0
    assert seen > 20


# ---- the scripted shapes of tests/test_gpu_engine_scripts.py: which vote kernel, and what they carry ------------
@pytest.mark.parametrize("shape", sorted(K.ENGINE_SHAPES))
def test_engine_script_shapes(shape):
    """Each shape's flattened mean row length lies in the bracket of the vote kernel it is there for, on every seed,
    and the script carries the things a solver gets wrong: variables fixed at their bound (on the oracle's solution),
    FATPIPE and zero-bound constraints, zero-weight elements, duplicate elements, zero-penalty variables."""
    from simgrid_amd import lmm as L
    from simgrid_amd import multi as M

    _, (lo, hi), seeds = K.ENGINE_SHAPES[shape]
    total = {}
    for seed in seeds:
        ops = K.engine_script(shape, seed)
        assert (seed % 2 == 0) == any(op[0] == "limit" for op in ops)
        s, _, _ = K.replay(L, ops)
        mean = K.mean_row(M.export_flat(s))
        assert lo < mean <= hi, (shape, seed, mean)
        feat = K.script_features(ops)
        o, _, ovs = K.replay(O, ops)
        o.solve()
        feat["fixed_at_bound"] = K.fixed_at_bound(ovs)
        for k, n in feat.items():
            total[k] = total.get(k, 0) + n
            # (WIDE has 6 constraints: a zero-bound one, drawn with probability 0.05 each, is there on some seeds only)
            assert n > 0 or (shape == "WIDE" and k == "zero_bound"), (shape, seed, k)
    assert all(n > 0 for n in total.values()), total
