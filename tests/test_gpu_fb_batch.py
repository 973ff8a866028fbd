"""The batched FairBottleneck engine (lmm_fb_batch_kernels.hpp: one workgroup per system, the system in LDS)
against the oracle, against every system solved alone by the chunked engine (lmm_fb_kernels.hpp) and against the
chunked engine on the same union (LMMHIP_BATCH=0).

Values are compared as bytes: the batch kernel performs the reference's floating-point operations in the
reference's order, like the chunked engine.  Rounds, saturated sets and work counters are those of each system
solved alone (the union's round count is their maximum).
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K
from tests.test_gpu_parity import FB_FATPIPE_SEEDS

pytestmark = pytest.mark.gpu
FB = L.System.FAIR_BOTTLENECK


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


def random_scripts():
    """The 40 operation scripts of tests/test_gpu_parity.py::test_random_fair_bottleneck_vs_oracle."""
    out = []
    for variant in ("fatpipe", "zero_bounds"):
        for i in range(20):
            seed = FB_FATPIPE_SEEDS[i] if variant == "fatpipe" else i
            kw = (dict(zero_bound_p=0.0, fatpipe_p=0.1) if variant == "fatpipe"
                  else dict(zero_bound_p=0.05, fatpipe_p=0.0))
            out.append(K.random_script(1000 + seed, conc_limits=(seed % 3 == 0), frees=2, bound_updates=3,
                                       zero_w_p=0.0, **kw))
    return out


def values_bytes(vs):
    return np.array([vs[k].get_value() for k in sorted(vs)]).tobytes()


class Solo:
    """One script solved alone on the device (the chunked engine) and by the oracle."""

    def __init__(self, ops):
        self.ops = ops
        s, _, vs = K.replay(L, ops, kind=FB)
        s.solve()
        assert s.last_engine() == L.System.RAN_FB_ROUNDS
        self.bytes = values_bytes(vs)
        self.rounds = s.last_stats()["rounds"]
        self.saturated = s.device_saturated()
        self.work = s.fb_work()
        o, _, self.ovs = K.replay(O, ops, kind=O.System.FAIR_BOTTLENECK)
        o.solve()
        self.oracle_rounds = o.last_rounds
        self._keep = o


@pytest.fixture(scope="module")
def solos():
    return [Solo(ops) for ops in random_scripts()]


def solve_batch_bytes(scripts):
    """The scripts replayed on fresh systems and solved by one lmm_solve_batch: (systems, variables, bytes)."""
    built = [K.replay(L, ops, kind=FB) for ops in scripts]
    ps = [b[0] for b in built]
    L.solve_batch(ps)
    return ps, [b[2] for b in built], [values_bytes(b[2]) for b in built]


def test_random_systems(solos):
    ps, pvs, got = solve_batch_bytes([s.ops for s in solos])
    assert ps[0].last_engine() == L.System.RAN_FB_BATCH
    for vs, solo, b in zip(pvs, solos, got):
        _, bad = K.compare_values(vs, solo.ovs)
        assert not bad, bad[:5]
        assert b == solo.bytes
    assert ps[0].last_stats()["rounds"] == max(s.rounds for s in solos)


@pytest.mark.parametrize("grid", ["3", "1"])
def test_lds_reuse(solos, grid, monkeypatch):
    """Fewer workgroups than systems: every workgroup restages its LDS for several systems."""
    monkeypatch.setenv("LMMHIP_FB_BATCH_GRID", grid)
    ps, _, got = solve_batch_bytes([s.ops for s in solos])
    assert ps[0].last_engine() == L.System.RAN_FB_BATCH
    assert got == [s.bytes for s in solos]
    assert ps[0].last_stats()["rounds"] == max(s.rounds for s in solos)


def test_weights_read_from_hbm(solos, monkeypatch):
    """The kernel variant of systems whose weights do not fit the LDS budget (LMMHIP_FB_BATCH_WLDS=0 selects it)."""
    monkeypatch.setenv("LMMHIP_FB_BATCH_WLDS", "0")
    ps, _, got = solve_batch_bytes([s.ops for s in solos])
    assert ps[0].last_engine() == L.System.RAN_FB_BATCH
    assert got == [s.bytes for s in solos]


def test_chunked_engine_on_the_union(solos, monkeypatch):
    monkeypatch.setenv("LMMHIP_BATCH", "0")
    ps, _, got = solve_batch_bytes([s.ops for s in solos])
    assert ps[0].last_engine() == L.System.RAN_FB_ROUNDS
    assert got == [s.bytes for s in solos]
    assert ps[0].last_stats()["rounds"] == max(s.rounds for s in solos)


def l07_params():
    ps = [dict(topology=L.FAT_TREE, topo_parameters="2;4,4;1,2;1,2", model=L.L07, n_flows=64, seed=s)
          for s in range(1, 65)]
    # 453 constraints each: the per-constraint loops stride past the workgroup's 256 threads
    ps += [dict(topology=L.DRAGONFLY, topo_parameters="3,4;4,3;5,1;2", model=L.L07, n_flows=256, seed=s, policy=pol)
           for pol in (L.SHARED, L.FATPIPE) for s in range(1, 5)]
    return ps


def test_l07_flows():
    params = l07_params()
    want = []
    for p in params:
        o = O.System(False, O.System.FAIR_BOTTLENECK)
        _, ov = o.gen_platform_flows(O.platform_params(**p))
        o.solve()
        want.append(o.values_of(ov, p["n_flows"]).tobytes())
    alone = []
    for p in params:
        s = L.System(False, FB)
        _, vs = s.gen_platform_flows(L.platform_params(**p))
        s.solve()
        alone.append(s.values_of(vs).tobytes())
    ps, ids = [], []
    for p in params:
        s = L.System(False, FB)
        _, vs = s.gen_platform_flows(L.platform_params(**p))
        ps.append(s)
        ids.append(vs)
    L.solve_batch(ps)
    assert ps[0].last_engine() == L.System.RAN_FB_BATCH
    got = [s.values_of(v).tobytes() for s, v in zip(ps, ids)]
    assert got == want   # the reference's operations in the reference's order
    assert got == alone


def cnst_bounds_of(ops):
    b = {}
    for op in ops:
        if op[0] in ("cnst", "cbound"):
            b[op[1]] = op[2]
    return b


def test_saturated_set_and_work_counters(solos):
    # 16 systems whose round counts differ: the slowest and the fastest FATPIPE ones, and zero-bound ones
    fat = sorted(range(20), key=lambda i: solos[i].oracle_rounds)
    pick = fat[:4] + fat[-4:] + list(range(20, 28))
    assert len({solos[i].oracle_rounds for i in pick}) > 4
    assert len({solos[i].rounds for i in pick}) > 4
    systems = [K.replay(L, solos[i].ops, kind=FB)[0] for i in pick]
    b = M.DeviceBatch(systems, kind=M.DeviceBatch.FAIR_BOTTLENECK)
    b.solve()
    assert b.last_engine() == L.System.RAN_FB_BATCH
    x, sat, work = b.values(), b.saturated(), b.fb_work()
    np.testing.assert_array_equal(sat, np.concatenate([solos[i].saturated for i in pick]))
    assert work == tuple(sum(solos[i].work[k] for i in pick) for k in range(3))
    assert b.stats()["rounds"] == max(solos[i].rounds for i in pick)
    b.solve()  # every solve re-initialises the state
    assert b.values().tobytes() == x.tobytes()
    np.testing.assert_array_equal(b.saturated(), sat)
    assert b.fb_work() == work
    # new bounds for the constraints of the systems without FATPIPE constraints (their round counts stay small),
    # against freshly built systems with those bounds
    fresh = []
    for i in pick:
        s, cs, vs = K.replay(L, solos[i].ops, kind=FB)
        if i >= 20:
            upd = [("cbound", c, round(0.75 * v + 0.1, 3) if v > 0 else 0.0)
                   for c, v in cnst_bounds_of(solos[i].ops).items()]
            K.replay(L, upd, sys_=s, cs=cs, vs=vs)
        fresh.append(s)
    flats = [M.export_flat(s) for s in fresh]
    cb = np.concatenate([f.cbound for f in flats])
    assert len(cb) == b.n_cnst and not np.array_equal(cb, b.arrays[5])
    b.update_cnst_bounds(cb)
    b.solve()
    xs, sats, works = [], [], []
    for s in fresh:
        s.solve()
        xs.append(s.device_values())
        sats.append(s.device_saturated())
        works.append(s.fb_work())
    assert b.values().tobytes() == np.concatenate(xs).tobytes()
    np.testing.assert_array_equal(b.saturated(), np.concatenate(sats))
    assert b.fb_work() == tuple(sum(w[k] for w in works) for k in range(3))
    b.close()


def degenerate_members():
    """Fresh systems: constraints without a variable, one variable on one constraint, a lone variable of penalty
    0, L07 flows with an unshared CPU (FATPIPE with an enabled zero-weight element, cflags bit1), two ordinary."""
    out = []
    s = L.System(False, FB)
    s.constraint_new(None, 3.0)
    s.constraint_new(None, 0.0)
    out.append(s)
    s = L.System(False, FB)
    s.expand(s.constraint_new(None, 3.0), s.variable_new(None, 1.0, -1.0, 1), 2.0)
    out.append(s)
    s = L.System(False, FB)
    s.expand(s.constraint_new(None, 3.0), s.variable_new(None, 0.0, -1.0, 1), 1.0)
    out.append(s)
    s = L.System(False, FB)
    p = L.platform_params(topology=L.FAT_TREE, topo_parameters="2;4,4;1,2;1,2", model=L.L07, n_flows=64, seed=7)
    cs, _ = s.gen_platform_flows(p)
    n_links, _ = L.platform_size(p)
    cpus = [L.Constraint(s, int(h)) for h in cs[n_links:]]
    cpu = next(c for c in cpus if c.elements())  # a CPU some flow runs on (at weight 0) ...
    cpu.unshare()
    s.expand(cpu, s.variable_new(None, 1.0, 0.5, 1), 1.0)  # ... and a bounded computation: the CPU is flattened
    assert 3 in M.export_flat(s).cflags
    out.append(s)
    scripts = random_scripts()
    out += [K.replay(L, scripts[21], kind=FB)[0], K.replay(L, scripts[2], kind=FB)[0]]
    return out


def test_degenerate_members():
    alone = degenerate_members()
    for s in alone:
        s.solve()
    ps = degenerate_members()
    L.solve_batch(ps)
    assert ps[0].last_engine() == L.System.RAN_FB_BATCH
    n = 0
    for a, p in zip(alone, ps):
        xa = np.array([v.get_value() for v in a.variables()])
        xp = np.array([v.get_value() for v in p.variables()])
        assert xa.tobytes() == xp.tobytes()
        n += len(xa)
    assert n > 150
    assert L.lib().lmm_solve_batch((L.P * 0)(), 0) == 0


def test_round_guard():
    s = L.System(False, FB)  # test_fair_bottleneck_nonterminating_input_is_reported's system
    z = s.constraint_new(None, 0.0)
    f = s.constraint_new(None, 5.0)
    f.unshare()
    a = s.variable_new(None, 1.0, -1.0, 2)
    b = s.variable_new(None, 1.0, -1.0, 1)
    s.expand(z, a, 1.0)
    s.expand(f, a, 1.0)
    s.expand(f, b, 1.0)
    scripts = random_scripts()
    with pytest.raises(L.LmmError, match="round guard"):
        L.solve_batch([s] + [K.replay(L, scripts[i], kind=FB)[0] for i in (20, 21)])
    ps, _, got = solve_batch_bytes([scripts[20], scripts[21]])
    assert ps[0].last_engine() == L.System.RAN_FB_BATCH
    alone = []
    for i in (20, 21):
        q, _, vs = K.replay(L, scripts[i], kind=FB)
        q.solve()
        alone.append(values_bytes(vs))
    assert got == alone


def test_dispatch():
    fresh = L.System(False, FB)
    with pytest.raises(L.LmmError):  # LMMHIP_E_STATE before any solve
        fresh.last_engine()
    scripts = random_scripts()

    def members():
        big = L.System(False, FB)  # 70,000 flows: more elements than a workgroup's 16-bit indices reach
        _, vs = big.gen_platform_flows(L.platform_params(topology=L.FAT_TREE, topo_parameters="2;4,4;1,2;1,2",
                                                         model=L.L07, n_flows=70_000, seed=3))
        small = [K.replay(L, scripts[i], kind=FB) for i in (22, 23)]
        return [small[0][0], big, small[1][0]], lambda: [values_bytes(small[0][2]), big.values_of(vs).tobytes(),
                                                           values_bytes(small[1][2])]

    alone, alone_bytes = members()
    for s in alone:
        s.solve()
    ps, got = members()
    L.solve_batch(ps)
    assert ps[0].last_engine() == L.System.RAN_FB_ROUNDS
    assert got() == alone_bytes()
    # profiling times every phase launch: the chunked engine
    built = [K.replay(L, scripts[i], kind=FB) for i in (22, 23)]
    built[0][0].set_profiling(True)
    L.solve_batch([b[0] for b in built])
    assert built[0][0].last_engine() == L.System.RAN_FB_ROUNDS
    assert [values_bytes(b[2]) for b in built] == [alone_bytes()[0], alone_bytes()[2]]
    # max-min: the batch engine for a batch, one of the global engines otherwise
    mm = [L.System(False) for _ in range(4)]
    for i, s in enumerate(mm):
        s.gen_maxmin_bench(0, i)
    L.solve_batch(mm)
    assert mm[0].last_engine() == L.System.RAN_BATCH
    one = L.System(False)
    one.gen_maxmin_bench(0, 0)
    one.solve()
    assert one.last_engine() in (L.System.RAN_PERSISTENT, L.System.RAN_ROUNDS, L.System.RAN_FRONTIER)


def test_device_batch_default_kind_is_maxmin():
    ps = [L.System(False) for _ in range(3)]
    for i, s in enumerate(ps):
        s.gen_maxmin_bench(0, i)
    b = M.DeviceBatch(ps)
    b.solve()
    assert b.last_engine() == L.System.RAN_BATCH and b.kind == M.DeviceBatch.MAXMIN
    x = b.values()
    for i, s in enumerate(ps):
        s.solve()
        assert np.allclose(s.device_values(), x[b.var_off[i]:b.var_off[i + 1]], rtol=1e-6, atol=1e-9)
    b.close()
