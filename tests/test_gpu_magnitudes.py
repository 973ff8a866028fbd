"""Max-min engines across magnitudes: every bound scaled by 2^k, and bounds of mixed exponents.

Every bound elsewhere in the suite lies in [0, 1e2] or in the platforms' 1e8..1e10.  Three pieces of the device path
depend on the exponent: ratio_key (the upper 16 bits of the ratio rounded down to f32: above FLT_MAX every ratio has the
key 0x7F7F, below 2^-133 the key 0, which is also row_floor's "sensitive row"), the frontier engine's ratio_key32
(saturating the same way), and the per-constraint fixed-point exponents dec_scale / cexp_pack (clamped to +-1000, packed
into signed 12-bit fields).  The keys only filter — equal keys fall back to the exact fp64 compare — and the fixed-point
scales are powers of two, so scaling every bound by 2^k (exact in fp64) must scale the device's solution EXACTLY:
the value bytes of the scaled system are ldexp(x, k) of the unscaled system's, after the same rounds, with every variable
fixed in the same round and the same saturated set.

  k = 40          the keys move 40 binades, still normal f32
  k = 150         every ratio above FLT_MAX: all keys equal, every vote a key tie, every row sensitive
  k = -160        below the smallest f32 subnormal: every key 0
  k = +-900       dec_scale within 100 of its clamp, the cexp fields near the ends of their 12 bits

Downward only scripts without variable bounds are scaled: the reference fixes a variable at its bound inside an
ABSOLUTE 1e-5 window (tests/test_oracle.py::test_oracle_downward_scaling_with_bounded_variables_is_not_exact), the
device compares bound levels exactly (domain and magnitudes).
"""
import functools

import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from tests import lmm_cases as K
from tests.test_gpu_engine_scripts import ENGINES, Solved, assert_same_solve

pytestmark = pytest.mark.gpu

UP, DOWN = (40, 150, 900), (-40, -160, -900)
CASES = [("R8", 0), ("R8", 1), ("R32", 1), ("R32", 3)]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


@functools.lru_cache(maxsize=None)
def _oracle(shape, seed, unbounded, k):
    """(values in key order, saturated set) of the oracle on the scaled script: solved once for the three engines."""
    o, ocs, ovs = K.replay(O, K.scale_script(K.engine_script(shape, seed, unbounded), k))
    o.solve()
    y = np.array([ovs[key].get_value() for key in sorted(ovs)])
    y.setflags(write=False)
    return y, frozenset(K.saturated(o, ocs, O.get_precision()))


@functools.lru_cache(maxsize=None)
def _unscaled(shape, seed, unbounded, engine):
    """The engine's own solve of the unscaled script (solved once, never modified): the x0 of ldexp(x0, k)."""
    base = Solved(K.engine_script(shape, seed, unbounded), engine, K.ENGINE_SHAPES[shape][1])
    assert np.count_nonzero(base.x) > 0 and base.rounds > 1
    return base


def _check_scaling(shape, seed, engine, unbounded, k):
    base = _unscaled(shape, seed, unbounded, engine)
    d = Solved(K.scale_script(K.engine_script(shape, seed, unbounded), k), engine)
    what = (shape, seed, engine, k)
    want = np.ldexp(base.x, k)
    y, osat = _oracle(shape, seed, unbounded, k)
    tol = np.maximum(np.ldexp(K.ABS_TOL, k), K.REL_TOL * np.abs(y))
    diff = np.abs(d.x - y)
    print(f"{what}: rounds {d.rounds} (unscaled {base.rounds}), max |x - oracle| * 2^-k = "
          f"{float(np.ldexp(diff.max(), -k)):.3e}, bytes equal: {d.x.tobytes() == want.tobytes()}")
    assert d.rounds == base.rounds, (what, d.rounds, base.rounds)
    assert d.x.tobytes() == want.tobytes(), \
        (what, int(np.count_nonzero(d.x != want)), float(np.ldexp(np.max(np.abs(d.x - want)), -k)))
    np.testing.assert_array_equal(d.var_rounds, base.var_rounds, err_msg=str(what))
    np.testing.assert_array_equal(d.sat, base.sat, err_msg=str(what))
    assert np.all(diff <= tol), (what, int(np.count_nonzero(diff > tol)))
    assert K.saturated(d.s, d.cs, L.get_precision()) == osat, what


@pytest.mark.parametrize("k", UP)
@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("shape,seed", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_upward_scaling_is_exact(shape, seed, engine, k):
    _check_scaling(shape, seed, engine, False, k)


@pytest.mark.parametrize("k", DOWN)
@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("shape,seed", CASES, ids=[f"{a}-{b}" for a, b in CASES])
def test_downward_scaling_without_variable_bounds_is_exact(shape, seed, engine, k):
    _check_scaling(shape, seed, engine, True, k)


def _batch_values(scripts):
    ps = [K.replay(L, ops) for ops in scripts]
    L.solve_batch([p[0] for p in ps])
    assert ps[0][0].last_engine() == L.System.RAN_BATCH
    return [np.array([vs[k].get_value() for k in sorted(vs)]) for _, _, vs in ps]


@pytest.mark.parametrize("direction", ["up", "down"])
def test_batch_engine_scaling_is_exact(direction):
    """The batch engine (one workgroup per system, state in LDS: its own copy of the init, vote, saturation and
    update) on the 30 x 60 scripts of seeds 0..7: each member's bytes are the ldexp of its unscaled bytes."""
    kw = dict(frees=3, penalty_updates=4, bound_updates=4)
    if direction == "up":
        scripts = [K.random_script(seed, conc_limits=(seed % 2 == 0), **kw) for seed in range(8)]
    else:
        scripts = [K.unbounded_script(seed, conc_limits=(seed % 2 == 0), **kw) for seed in range(8)]
    base = _batch_values(scripts)
    assert all(np.count_nonzero(x) > 0 for x in base)
    for i, ops in enumerate(scripts):  # the unscaled members against the oracle
        o, _, ovs = K.replay(O, ops)
        o.solve()
        y = np.array([ovs[k].get_value() for k in sorted(ovs)])
        assert np.all(np.abs(base[i] - y) <= np.maximum(K.ABS_TOL, K.REL_TOL * np.abs(y))), i
    for k in (UP if direction == "up" else DOWN):
        got = _batch_values([K.scale_script(ops, k) for ops in scripts])
        for i, (x, x0) in enumerate(zip(got, base)):
            assert x.tobytes() == np.ldexp(x0, k).tobytes(), (direction, k, i, int(np.count_nonzero(x != np.ldexp(x0, k))))


@functools.lru_cache(maxsize=None)
def _spread(seed):
    """The spread script of `seed`, the oracle's solution of it, and the round engine's (each solved once)."""
    ops = K.spread_script(K.engine_script("R8", seed), seed, 80)
    o, ocs, ovs = K.replay(O, ops)
    o.solve()
    y = np.array([ovs[k].get_value() for k in sorted(ovs)])
    y.setflags(write=False)
    return ops, y, frozenset(K.saturated(o, ocs, O.get_precision())), Solved(ops, "rounds", K.ENGINE_SHAPES["R8"][1])


@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("seed", range(4))
def test_mixed_exponents(seed, engine):
    """Bounds spread over 80 binades inside one system (K.spread_script of the R8 script): the oracle's values at the
    usual tolerances, the same saturated set, and the three engines bit for bit."""
    ops, y, osat, ref = _spread(seed)
    # the spread is there, and the absolute floor of the comparison is inert (3.8e-3 is the smallest over the four seeds)
    assert y.max() / y[y > 0].min() > 1e20
    assert y[y > 0].min() > 1e3 * K.ABS_TOL
    d = Solved(ops, engine, K.ENGINE_SHAPES["R8"][1])
    diff = np.abs(d.x - y)
    tol = np.maximum(K.ABS_TOL, K.REL_TOL * np.abs(y))
    print(f"spread seed {seed} {engine}: rounds {d.rounds}, max relative error "
          f"{float(np.max(diff[y > 0] / y[y > 0])):.3e}")
    assert np.all(diff <= tol), (engine, int(np.count_nonzero(diff > tol)), float(np.max(diff[y > 0] / y[y > 0])))
    assert K.saturated(d.s, d.cs, L.get_precision()) == osat, engine
    assert_same_solve(ref, d, "rounds / " + engine)
