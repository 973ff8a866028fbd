"""Round engine: rows of saturated targets retired by the vote's filter (kSatKey).

mm_update marks a constraint that saturated with kSatKey and one that was exhausted by other constraints'
saturations with kDeadKey.  The short-row vote's filter retires a row whose target carries kSatKey with one store
(its variable was fixed by that saturation) and the re-votes read no variable state; LMMHIP_SATKEY=0 keeps the
state-read path in the same build.  The two must agree bit for bit on the values, the round count, the round that
fixed every variable and the saturated set; the rows that vote for an EXHAUSTED constraint are alive and must re-vote
(test_exhausted_target_keeps_its_voters_alive: the case a wrong key encoding gets wrong).
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K

pytestmark = pytest.mark.gpu

STRESS = dict(penalty_mix=1, bounded_permille=100, fatpipe_permille=50)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


def _synthetic(nc, nv, seed, stress):
    def build(s):
        return s.gen_synthetic(nc, nv, 8, seed=seed, **(STRESS if stress else {}))
    return build


def _bench_big(s):
    return np.array([v.h for v in s.gen_maxmin_bench(2, 0)[1]], dtype=np.int64)


def _duplicates(s):
    """A constraint holding two elements of each of its 40,000 variables: it saturates (1e6 / 40,000 per variable
    is below every small constraint's share) and claims every variable once."""
    big = s.constraint_new(None, 1e6)
    vs = []
    for i in range(40_000):
        c = s.constraint_new(None, 1.0 + (i % 97))
        v = s.variable_new(None, 1.0 + (i % 3), -1.0, 3)
        s.expand(big, v, 1.0)
        s.expand(c, v, 1.0)
        s.expand(big, v, 0.05 * (1 + i % 5))
        vs.append(v.h)
    return np.array(vs, dtype=np.int64)


def _solved(build, satkey, monkeypatch, env=()):
    """(system, ids, value bytes, rounds, per-variable rounds, saturated set) of the round engine under LMMHIP_SATKEY."""
    for k, v in env:
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("LMMHIP_SATKEY", satkey)
    s = L.System(False)
    ids = build(s)
    s.set_engine(L.System.ENGINE_ROUNDS)
    s.solve()
    assert s.last_engine() == L.System.RAN_ROUNDS
    return s, ids, s.values_of(ids), s.last_stats()["rounds"], s.device_var_rounds(), s.device_saturated()


def _assert_same(a, b):
    _, _, xa, ra, vra, sa = a
    _, _, xb, rb, vrb, sb = b
    assert ra == rb, (ra, rb)
    assert xa.tobytes() == xb.tobytes(), float(np.max(np.abs(xa - xb)))
    np.testing.assert_array_equal(vra, vrb)
    np.testing.assert_array_equal(sa, sb)


ON_OFF = {
    "synthetic_2e3x2e4": (_synthetic(2000, 20000, 3, False), ()),
    "synthetic_2e3x2e4_stress": (_synthetic(2000, 20000, 3, True), ()),
    # rows retired in buffers 1 and 2 across several compactions
    "synthetic_2e4x2e5_compact8": (_synthetic(20000, 200000, 7, False),
                                   (("LMMHIP_COMPACT_EVERY", "8"), ("LMMHIP_COMPACT_PCT", "100"))),
    "synthetic_2e4x2e5_stamps": (_synthetic(20000, 200000, 7, False), (("LMMHIP_VOTE_BITS", "0"),)),
    "synthetic_2e4x2e5_no_rdq": (_synthetic(20000, 200000, 7, False), (("LMMHIP_RDQ", "0"),)),
    "synthetic_2e4x2e5_no_crec": (_synthetic(20000, 200000, 7, False), (("LMMHIP_CREC", "0"),)),
    "big_run0": (_bench_big, ()),
    "duplicates": (_duplicates, ()),
}


@pytest.mark.parametrize("name", sorted(ON_OFF))
def test_satkey_on_off_bit_identical(name, monkeypatch):
    build, env = ON_OFF[name]
    on = _solved(build, "1", monkeypatch, env)
    off = _solved(build, "0", monkeypatch, env)
    _assert_same(on, off)
    assert on[3] > 1 and np.count_nonzero(on[2]) > 0


def _saturated_dense(f, x, prec):
    """Saturated constraints (`bound - usage <= bound * prec`) of the flattened system under the dense values x."""
    rows = np.repeat(np.arange(len(f.penalty)), np.diff(f.var_ptr))
    wx = f.weight * x[rows]
    use = np.bincount(f.cnst_idx, weights=wx, minlength=len(f.cbound))
    fat = (f.cflags & 1).astype(bool)
    if fat.any():
        mx = np.zeros(len(f.cbound))
        np.maximum.at(mx, f.cnst_idx, wx)
        use = np.where(fat, mx, use)
    return np.flatnonzero(~(f.cbound - use > f.cbound * prec))


@functools.lru_cache(maxsize=None)
def _oracle_values(stress):
    o = O.System(False)
    ov = o.gen_synthetic(2000, 20000, 8, seed=3, **(STRESS if stress else {}))
    o.solve()
    y = o.values_of(ov, 20000)
    y.setflags(write=False)
    return y


@pytest.mark.parametrize("stress", [False, True])
def test_satkey_vs_oracle(stress, monkeypatch):
    monkeypatch.setenv("LMMHIP_SATKEY", "1")
    s = L.System(False)
    pv = s.gen_synthetic(2000, 20000, 8, seed=3, **(STRESS if stress else {}))
    f = M.export_flat(s)
    s.set_engine(L.System.ENGINE_ROUNDS)
    s.solve()
    x, y = s.values_of(pv), _oracle_values(stress)
    diff, tol = np.abs(x - y), np.maximum(K.ABS_TOL, K.REL_TOL * np.abs(y))
    assert np.all(diff <= tol), (float(diff.max()), int(np.count_nonzero(diff > tol)))
    pos = np.searchsorted(pv, f.var_ids)
    assert np.all(np.diff(pv) > 0) and np.array_equal(pv[pos], f.var_ids)
    prec = L.get_precision()
    np.testing.assert_array_equal(_saturated_dense(f, x[pos], prec), _saturated_dense(f, y[pos], prec))


def _random_system(s, tight=False):
    """2,000 constraints, 20,000 variables of 3 elements each (short rows: the lane-per-row vote).  tight: every third
    constraint's bound a thousandth of it."""
    rng = np.random.default_rng(17)
    nc, nv = 2000, 20000
    bounds = rng.uniform(1.0, 100.0, nc)
    cs = [s.constraint_new(None, float(b)) for b in bounds]
    on = rng.integers(0, nc, (nv, 3))
    w = rng.uniform(0.5, 2.0, (nv, 3))
    vs = []
    for i in range(nv):
        v = s.variable_new(None, 1.0, -1.0, 3)
        for k in range(3):
            s.expand(cs[on[i, k]], v, float(w[i, k]))
        vs.append(v.h)
    if tight:
        _tighten(s, cs, bounds)
    return cs, bounds, np.array(vs, dtype=np.int64)


def _tighten(s, cs, bounds):
    for k in range(0, len(cs), 3):
        s.update_constraint_bound(cs[k], float(bounds[k]) * 1e-3)


def test_resolve_on_one_context_after_bound_changes(monkeypatch):
    """Solve, tighten a third of the constraint bounds (another round count) and solve again on the same context:
    the bytes, rounds and saturated set of a fresh context (no stale key, stamp or round hint survives)."""
    monkeypatch.setenv("LMMHIP_SATKEY", "1")
    s = L.System(False)
    cs, bounds, ids = _random_system(s)
    s.set_engine(L.System.ENGINE_ROUNDS)
    s.solve()
    r0 = s.last_stats()["rounds"]
    _tighten(s, cs, bounds)
    s.solve()
    x, r1, vr, sat = s.values_of(ids), s.last_stats()["rounds"], s.device_var_rounds(), s.device_saturated()
    f = L.System(False)
    _, _, fids = _random_system(f, tight=True)
    f.set_engine(L.System.ENGINE_ROUNDS)
    f.solve()
    assert r1 == f.last_stats()["rounds"], (r1, f.last_stats()["rounds"])
    assert x.tobytes() == f.values_of(fids).tobytes()
    np.testing.assert_array_equal(vr, f.device_var_rounds())
    np.testing.assert_array_equal(sat, f.device_saturated())
    assert r0 != r1, (r0, r1)  # (the first solve's hint was wrong)


N_GADGETS = 600


def _exhausted_gadgets(s):
    """N_GADGETS independent gadgets of three constraints S, T, U and two variables a, b (penalty 1, precision 1e-5):

      a on S (weight 1) and T (weight 1); b on T (weight wb << precision) and U (weight 1).
      ratio(S) < ratio(T) < ratio(U): a votes for S, b votes for T.  Round 0 saturates S alone (T is not ready: a votes
      elsewhere) and fixes a = bound(S).  T then leaves the light table WITHOUT saturating, while b, alive, votes for it:
        even gadgets, T FATPIPE, bound 1, wb = 1e-6: its usage, the max w/p over the unfixed elements, falls from 1 to
          1e-6 <= precision;
        odd gadgets, T SHARED, bound 1, wb = 1e-7, bound(S) in [0.999992, 0.999995] (< ratio(T) = 1 / (1 + 1e-7)):
          its remaining 1 - bound(S) <= 8e-6 falls below bound * precision.
      b must re-vote, for U, and ends at bound(U) — not retired at 0 as the voter of a saturated constraint is.
    Returns the variables (a0, b0, a1, b1, ...) and the expected values."""
    vs, want = [], []
    for i in range(N_GADGETS):
        fat = i % 2 == 0
        bs = 0.25 + 0.01 * (i % 13) if fat else 0.999995 - 1e-6 * (i % 4)
        bu = 50.0 + (i % 5)
        cS, cT, cU = s.constraint_new(None, bs), s.constraint_new(None, 1.0), s.constraint_new(None, bu)
        if fat:
            cT.unshare()
        a, b = s.variable_new(None, 1.0, -1.0, 2), s.variable_new(None, 1.0, -1.0, 2)
        s.expand(cS, a, 1.0)
        s.expand(cT, a, 1.0)
        s.expand(cT, b, 1e-6 if fat else 1e-7)
        s.expand(cU, b, 1.0)
        vs += [a, b]
        want += [bs, bu]
    return vs, np.array(want)


def test_exhausted_target_keeps_its_voters_alive(monkeypatch):
    """A constraint that dies exhausted while a live row votes for it (the gadgets above): that row re-votes.  Knob on
    against knob off (bit for bit), against the oracle, and against the values worked out by hand."""
    assert L.get_precision() == 1e-5

    def build(s):
        return np.array([v.h for v in _exhausted_gadgets(s)[0]], dtype=np.int64)

    on = _solved(build, "1", monkeypatch)
    off = _solved(build, "0", monkeypatch)
    x = on[2]
    assert np.all(x[1::2] > 0), int(np.count_nonzero(x[1::2] == 0))  # no b retired at 0
    _assert_same(on, off)
    o = O.System(False)
    ovs, want = _exhausted_gadgets(o)
    o.solve()
    y = np.array([v.get_value() for v in ovs])
    tol = np.maximum(K.ABS_TOL, K.REL_TOL * np.abs(y))
    assert np.all(np.abs(x - y) <= tol), float(np.max(np.abs(x - y)))
    assert np.all(np.abs(x - want) <= np.maximum(K.ABS_TOL, K.REL_TOL * want)), float(np.max(np.abs(x - want)))
