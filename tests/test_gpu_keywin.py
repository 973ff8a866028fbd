"""Round engine: the 16-bit keys as codes of a per-solve window (simgrid_amd/csrc/lmm_keywin.hpp, DESIGN.md "Key window").

The round engine chooses a window {base, shift} over the f32 bits of each solve's initial ratios on the device and
makes every key in it; LMMHIP_KEY_WINDOW=0 keeps the window {0, 16} — the f32's upper 16 bits, the key of the other
engines — in the same build.  The keys are a prefilter: any monotone map gives the same targets, rounds and values.  So
for every system below the two must agree byte for byte on the values, the round count, the round that fixed every
variable and the saturated set; both are within the parity tolerance max(1e-9, 1e-6 |x|) of the oracle, and their values
and saturated set are the frontier engine's (32-bit keys of its own) byte for byte.  A bounded variable is fixed at its
bound on the keys alone when the key of bound * penalty is below the row's minimal key, takes no exact ratio when it is
above, and the exact compare when they tie: the systems put bound * penalty below every ratio, above every ratio, and
exactly on a constraint's ratio.
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from tests import lmm_cases as K

pytestmark = pytest.mark.gpu

STRESS = dict(penalty_mix=1, bounded_permille=100, fatpipe_permille=50)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


# ---- the systems: build(s) on an L.System or an O.System, returns the variables (objects, or gen_synthetic's handles) --

def _synthetic(nc, nv, seed, stress):
    def build(s):
        return s.gen_synthetic(nc, nv, 8, seed=seed, **(STRESS if stress else {}))
    return build


def _regular(s, nc, nv, k, bounds, weight, var, want_cs=False):
    """nv variables of k elements, variable i on the constraints (i + j * (nc // k)) % nc: with nc | nv every constraint
    holds nv * k / nc elements.  weight(i, j) and var(i) -> (penalty, bound) say the rest."""
    cs = [s.constraint_new(None, float(b)) for b in bounds]
    vs = []
    for i in range(nv):
        p, b = var(i)
        v = s.variable_new(None, float(p), float(b), k)
        for j in range(k):
            s.expand(cs[(i + j * (nc // k)) % nc], v, float(weight(i, j)))
        vs.append(v)
    return (cs, vs) if want_cs else vs


def _all_same(s):
    """Every constraint with the same bound and usage: every initial key ties at code 0 (the initial ratios span zero
    width; the window above them is the headroom alone)."""
    return _regular(s, 200, 2000, 4, np.full(200, 10.0), lambda i, j: 1.0, lambda i: (1.0, -1.0))


def _spread(s):
    """Ratios over 1e-30 .. 1e30: the coarsest windows (a shift of 12 or more)."""
    rng = np.random.default_rng(11)
    bounds = 10.0 ** rng.uniform(-30.0, 30.0, 500)
    w = rng.uniform(0.5, 2.0, (4000, 4))
    return _regular(s, 500, 4000, 4, bounds, lambda i, j: w[i, j], lambda i: (1.0 + i % 3, -1.0))


def _single(s):
    c = s.constraint_new(None, 3.0)
    v = s.variable_new(None, 2.0, -1.0, 1)
    s.expand(c, v, 0.5)
    return [v]


def _bounded(level, k=3, nc=300, nv=3000):
    """Two thirds of the variables bounded, penalties 1, 2, 4; the ratios start near 100 / (nv * k / nc * 1.25 / 2):
    level 'below' puts bound * penalty under every ratio of the solve, 'above' over every one, 'mid' among them."""
    def build(s):
        rng = np.random.default_rng(23 + k)
        bounds = rng.uniform(1.0, 100.0, nc)
        w = rng.uniform(0.5, 2.0, (nv, k))
        lv = dict(below=rng.uniform(1e-7, 1e-5, nv), above=rng.uniform(1e5, 1e7, nv),
                  mid=10.0 ** rng.uniform(-2.0, 1.0, nv))[level]

        def var(i):
            p = float(1 << (i % 3))
            return p, (lv[i] / p if i % 3 != 2 else -1.0)
        return _regular(s, nc, nv, k, bounds, lambda i, j: w[i, j], var)
    return build


N_TIES = 600


def _bound_on_ratio(s):
    """Gadgets of one constraint (bound B) and two variables a (weight 1, penalty 1) and b (weight wb, penalty 2): the
    initial ratio is r = B / (1 + wb / 2), in fp64 as the device computes it (a two-term sum).  a's bound * penalty is
    r exactly, one ulp under it, or one ulp over it (by gadget): the same key as the constraint's, so the exact compare
    decides — fixed at the bound only when strictly below."""
    vs = []
    for i in range(N_TIES):
        B, wb = 1.0 + 0.37 * (i % 29), 0.5 + 0.25 * (i % 5)
        r = B / (1.0 / 1.0 + wb / 2.0)
        ab = [r, np.nextafter(r, 0.0), np.nextafter(r, np.inf)][i % 3]
        c = s.constraint_new(None, B)
        a, b = s.variable_new(None, 1.0, float(ab), 1), s.variable_new(None, 2.0, -1.0, 1)
        s.expand(c, a, 1.0)
        s.expand(c, b, wb)
        vs += [a, b]
    return vs


N_GROWN = 300


def _grown_past_top(s):
    """Gadgets of three constraints S (bound 0.25 .. 0.37), T (bound 1), U (bound 2) and two variables a on S and T
    (weights 1) and b on T (weight 1e-3) and U (weight 1): the initial ratios lie in [0.25, 2], so the window's top code
    stands at most 2^8 above 0.25.  Round 0 saturates S and fixes a; T's usage falls to 1e-3 and its ratio grows from 1
    to about 700, past the window's top: its key clamps at kKeyTop, and b (U's ratio is 2) votes for U all the same."""
    vs = []
    for i in range(N_GROWN):
        cS, cT, cU = (s.constraint_new(None, 0.25 + 0.01 * (i % 13)), s.constraint_new(None, 1.0),
                      s.constraint_new(None, 2.0))
        a, b = s.variable_new(None, 1.0, -1.0, 2), s.variable_new(None, 1.0, -1.0, 2)
        s.expand(cS, a, 1.0)
        s.expand(cT, a, 1.0)
        s.expand(cT, b, 1e-3)
        s.expand(cU, b, 1.0)
        vs += [a, b]
    return vs


SYSTEMS = {
    "grown_past_top": (_grown_past_top, ()),
    "synthetic_plain": (_synthetic(1000, 10000, 5, False), ()),
    "synthetic_stress": (_synthetic(1000, 10000, 5, True), ()),
    # the record-less vote (the exact pass for every bounded variable) and the stamps' filter, under a window
    "synthetic_stress_no_crec": (_synthetic(1000, 10000, 5, True), (("LMMHIP_CREC", "0"),)),
    "synthetic_stress_stamps": (_synthetic(1000, 10000, 5, True), (("LMMHIP_VOTE_BITS", "0"), ("LMMHIP_RDQ", "0"))),
    "all_same": (_all_same, ()),
    "spread_1e60": (_spread, ()),
    "single": (_single, ()),
    "bounded_below": (_bounded("below"), ()),
    "bounded_above": (_bounded("above"), ()),
    "bounded_mid": (_bounded("mid"), ()),
    "bounded_on_ratio": (_bound_on_ratio, ()),
    # rows of 16 elements: the long-row vote (a group of lanes per row)
    "long_rows_bounded_below": (_bounded("below", k=16, nc=400, nv=1600), ()),
    "long_rows_bounded_mid": (_bounded("mid", k=16, nc=400, nv=1600), ()),
}


def _ids(vs):
    return vs if isinstance(vs, np.ndarray) else np.array([v.h for v in vs], dtype=np.int64)


def _solved(build, engine, monkeypatch, window=None, env=()):
    """(values, rounds, per-variable rounds, saturated set, key window) of one engine on a fresh context."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    if window is not None:
        monkeypatch.setenv("LMMHIP_KEY_WINDOW", window)
    s = L.System(False)
    ids = _ids(build(s))
    s.set_engine(engine)
    s.solve()
    rounds = engine == L.System.ENGINE_ROUNDS
    assert s.last_engine() == (L.System.RAN_ROUNDS if rounds else L.System.RAN_FRONTIER)
    return (s.values_of(ids), s.last_stats()["rounds"], s.device_var_rounds(), s.device_saturated(),
            s.key_window() if rounds else None)


@functools.lru_cache(maxsize=None)
def _oracle(name):
    o = O.System(False)
    vs = SYSTEMS[name][0](o)
    o.solve()
    y = np.array([v.get_value() for v in vs]) if isinstance(vs, list) else o.values_of(vs, len(vs))
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("name", sorted(SYSTEMS))
def test_window_on_off_oracle_frontier(name, monkeypatch):
    build, env = SYSTEMS[name]
    on = _solved(build, L.System.ENGINE_ROUNDS, monkeypatch, "1", env)
    off = _solved(build, L.System.ENGINE_ROUNDS, monkeypatch, "0", env)
    fr = _solved(build, L.System.ENGINE_FRONTIER, monkeypatch)
    y = _oracle(name)
    print(name, "rounds", on[1], "window", on[4], "legacy", off[4])
    assert off[4]["base"] == 0 and off[4]["shift"] == 16, off[4]
    assert on[4]["shift"] < 16, on[4]  # (16 bits over at most the whole f32 range: never coarser than 15)
    assert on[1] == off[1], (on[1], off[1])
    assert on[0].tobytes() == off[0].tobytes(), float(np.max(np.abs(on[0] - off[0])))
    np.testing.assert_array_equal(on[2], off[2])
    np.testing.assert_array_equal(on[3], off[3])
    tol = np.maximum(K.ABS_TOL, K.REL_TOL * np.abs(y))
    for x in (on[0], off[0]):
        d = np.abs(x - y)
        assert np.all(d <= tol), (float(d.max()), int(np.count_nonzero(d > tol)))
    assert on[0].tobytes() == fr[0].tobytes(), float(np.max(np.abs(on[0] - fr[0])))
    np.testing.assert_array_equal(on[3], fr[3])
    assert np.count_nonzero(on[0]) > 0


def test_the_systems_are_what_they_say(monkeypatch):
    """The bounded systems reach the paths they are named for (from the values: a variable fixed at its bound has it)."""
    def at_bound(name):
        build = SYSTEMS[name][0]
        o = O.System(False)
        vs = build(o)
        b = np.array([v.get_bound() for v in vs])
        return b, np.isclose(_oracle(name), b, rtol=1e-12, atol=0) & (b > 0)
    b, hit = at_bound("bounded_below")
    assert np.array_equal(hit, b > 0) and np.count_nonzero(hit) == 2000
    b, hit = at_bound("bounded_above")
    assert not hit.any()
    b, hit = at_bound("bounded_mid")
    assert 100 < np.count_nonzero(hit) < 1900, int(np.count_nonzero(hit))
    b, hit = at_bound("long_rows_bounded_below")
    assert np.array_equal(hit, b > 0)
    # the window of the spread system: the coarsest shifts
    w = _solved(SYSTEMS["spread_1e60"][0], L.System.ENGINE_ROUNDS, monkeypatch, "1")[4]
    assert w["shift"] >= 12, w
    # keys that clamp at the window's top: counted by the diagnostic launches of a profiled solve
    monkeypatch.setenv("LMMHIP_VOTE_DIAG", "1")
    monkeypatch.setenv("LMMHIP_KEY_WINDOW", "1")
    s = L.System(False)
    ids = _ids(_grown_past_top(s))
    s.set_engine(L.System.ENGINE_ROUNDS)
    s.set_profiling(True)
    s.solve()
    w = s.key_window()
    assert w["base"] == int(np.float32(0.25).view(np.uint32)) and w["shift"] <= 10, w
    assert w["key_clamped"] >= N_GROWN and w["key_stores"] >= w["key_clamped"], w
    x = s.values_of(ids)
    assert np.array_equal(x[1::2], np.full(N_GROWN, 2.0)), x[1::2][:4]
    monkeypatch.delenv("LMMHIP_VOTE_DIAG")
    w = _solved(_all_same, L.System.ENGINE_ROUNDS, monkeypatch, "1")[4]
    r = np.float32(10.0 / 40.0)  # (2000 * 4 / 200 elements of weight 1, penalty 1)
    assert w["base"] == int(r.view(np.uint32)), w


def _random_system(s, tight=False):
    rng = np.random.default_rng(17)
    nc, nv = 1000, 10000
    bounds = rng.uniform(1.0, 100.0, nc)
    w = rng.uniform(0.5, 2.0, (nv, 3))
    if tight:  # (as after _tighten)
        bounds[::3] *= 1e-3
    cs, vs = _regular(s, nc, nv, 3, bounds, lambda i, j: w[i, j],
                      lambda i: (1.0, rng.uniform(0.01, 1.0) if i % 4 == 0 else -1.0), want_cs=True)
    return cs, vs, bounds


def test_resolve_on_one_context_after_bound_changes(monkeypatch):
    """Solve, cut a third of the constraint bounds to a thousandth — another minimum ratio, so another window — and solve
    again on the same context: the bytes, rounds and saturated set of a fresh context under either window."""
    monkeypatch.setenv("LMMHIP_KEY_WINDOW", "1")
    s = L.System(False)
    cs, vs, bounds = _random_system(s)
    ids = _ids(vs)
    s.set_engine(L.System.ENGINE_ROUNDS)
    s.solve()
    w0 = s.key_window()
    for k in range(0, len(bounds), 3):
        s.update_constraint_bound(cs[k], float(bounds[k]) * 1e-3)
    s.solve()
    w1 = s.key_window()
    x, r1, vr, sat = s.values_of(ids), s.last_stats()["rounds"], s.device_var_rounds(), s.device_saturated()
    assert w1["base"] < w0["base"], (w0, w1)
    for window in ("1", "0"):
        monkeypatch.setenv("LMMHIP_KEY_WINDOW", window)
        f = L.System(False)
        _, fvs, _ = _random_system(f, tight=True)
        f.set_engine(L.System.ENGINE_ROUNDS)
        f.solve()
        assert r1 == f.last_stats()["rounds"], (r1, f.last_stats()["rounds"])
        assert x.tobytes() == f.values_of(_ids(fvs)).tobytes()
        np.testing.assert_array_equal(vr, f.device_var_rounds())
        np.testing.assert_array_equal(sat, f.device_saturated())
        if window == "1":
            assert f.key_window() == w1, (f.key_window(), w1)
