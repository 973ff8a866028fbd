"""The batched max-min engine (lmm_batch_kernels.hpp, mm_batch_lds: one workgroup per system, the system in LDS)
on systems the maxmin_bench generator does not make: bounded variables, FATPIPE and zero-bound constraints,
penalties other than 1, more than 64 variables and more than 256 constraints, members of unlike sizes in one
batch, a member close to the 64-KB LDS budget and one beyond it.

Every member is built twice by the same call sequence, on the product and on the oracle.  Values are compared
with the oracle at the tolerances of tests/lmm_cases.py, saturated sets exactly.  Between two runs of the batch
engine the comparison is of bytes: the initial usage is summed sequentially in CSC order and the decrements are
fixed-point integers, so neither the other members of the batch, nor their order, nor the number of workgroups
may change a bit.  The global engines reduce in another order: tolerance there.
"""
import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K
from tests.test_gpu_configs import _close, _sat_dense

pytestmark = pytest.mark.gpu

STRESS = dict(penalty_mix=1, bounded_permille=100, fatpipe_permille=50)
GLOBAL_ENGINES = (L.System.RAN_PERSISTENT, L.System.RAN_ROUNDS, L.System.RAN_FRONTIER)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


class Script:
    """A member made by replaying an operation script (tests/lmm_cases.py)."""

    def __init__(self, ops):
        self.ops = ops

    def build(self, mod):
        """(system, constraints by script key, variables in ascending key order)."""
        s, cs, vs = K.replay(mod, self.ops)
        return s, cs, [vs[k] for k in sorted(vs)]


class Synthetic:
    """A member made by the synthetic generator (lmm_generators.hpp), stress mix."""

    def __init__(self, nb_cnst, nb_var, seed):
        self.args = (nb_cnst, nb_var, 8, seed)

    def build(self, mod):
        s = mod.System(False)
        return s, None, s.gen_synthetic(*self.args, **STRESS)


def _members():
    kw = dict(frees=3, penalty_updates=4, bound_updates=4)
    m = {f"A{i}": Script(K.random_script(i, conc_limits=(i % 2 == 0), **kw)) for i in range(40)}
    for i in range(2):
        # ~280 variables on 300 constraints: the per-constraint loops stride past the workgroup's 256 threads
        m[f"B{i}"] = Script(K.random_script(2000 + i, n_cnst=300, n_var=300, max_el=12))
        # rows of up to 30 elements: past the 16 weights the saturation prefetches
        m[f"C{i}"] = Script(K.random_script(2100 + i, n_cnst=40, n_var=80, max_el=30))
        # ~380 variables on 6 constraints, half of them FATPIPE: long FATPIPE recomputes
        m[f"E{i}"] = Script(K.random_script(2200 + i, n_cnst=6, n_var=400, max_el=3, fatpipe_p=0.5))
    m["D"] = Synthetic(100, 600, 3)
    m["N"] = Synthetic(100, 900, 4)    # 900 x 100 x 7200: 61,408 of the 65,536 bytes of LDS
    m["X"] = Synthetic(200, 2000, 5)   # 135,008 bytes: no batch engine for a batch it is in
    return m


MEMBERS = _members()
A = [f"A{i}" for i in range(40)]
MIXED = A + ["B0", "B1", "C0", "C1", "E0", "E1", "D", "N"]
# a large member, then a small one, then a large one of another shape ...: every restaging changes the sizes
ALTERNATING = [n for pair in zip(["N", "B0", "E0", "C0", "D", "B1", "E1", "C1"], A) for n in pair] + A[8:]


def values_of(s, vs):
    """Values of a product system's variables `vs` (a list of Variables or an array of ids)."""
    return s.values_of(vs if isinstance(vs, np.ndarray) else np.array([v.h for v in vs], np.int64))


class Want:
    """A member solved by the oracle: values in the member's variable order, saturated set (scripts)."""

    def __init__(self, m, prec, change=None):
        s, cs, vs = m.build(O)
        if change:
            change(O, s, cs)
        s.solve()
        self.y = s.values_of(vs, len(vs)) if cs is None else np.array([v.get_value() for v in vs])
        self.saturated = None if cs is None else K.saturated(s, cs, prec)


@pytest.fixture(scope="module")
def want():
    prec = L.get_precision()
    return {n: Want(m, prec) for n, m in MEMBERS.items()}


class Batch:
    """Fresh product systems of the named members, solved by one lmm_solve_batch."""

    def __init__(self, names, flats=False):
        self.names = list(names)
        self.built = [MEMBERS[n].build(L) for n in self.names]
        self.systems = [b[0] for b in self.built]
        self.flats = [M.export_flat(s) for s in self.systems] if flats else None
        L.solve_batch(self.systems)
        self.engine = self.systems[0].last_engine()
        self.rounds = self.systems[0].last_stats()["rounds"]
        self.x = {n: values_of(b[0], b[2]) for n, b in zip(self.names, self.built)}
        self.bytes = {n: x.tobytes() for n, x in self.x.items()}

    def saturated(self, name, prec):
        s, cs, _ = self.built[self.names.index(name)]
        return K.saturated(s, cs, prec)


@pytest.fixture(scope="module")
def mixed():
    return Batch(MIXED, flats=True)


def dense_order(flat, vs, y):
    """`y` (the member's variable order) in the dense order of the member's flattened system."""
    ids = vs if isinstance(vs, np.ndarray) else [v.h for v in vs]
    pos = {int(h): j for j, h in enumerate(ids)}
    return y[[pos[int(h)] for h in flat.var_ids]]


def check_against_oracle(batch, want, prec):
    for n in batch.names:
        bad, worst = _close(batch.x[n], want[n].y)
        assert len(bad) == 0, (n, len(bad), worst)
        if want[n].saturated is not None:
            assert batch.saturated(n, prec) == want[n].saturated, n


def test_random_systems_vs_oracle(mixed, want):
    """V: bound fixes and their decrement records, penalties in x = ratio / p and w / p, the loops over more than
    64 variables; init: FATPIPE maximum, zero-bound constraints; S: rows longer than the prefetch, the FATPIPE
    skip; U: FATPIPE recompute, more than 256 constraints; members far below the batch maxima and one near the LDS
    budget."""
    prec = L.get_precision()
    assert mixed.engine == L.System.RAN_BATCH
    check_against_oracle(mixed, want, prec)
    # the batch carries what it is here for (random_script may change): counted on the flattened members
    at_bound = fatpipe = zero_bound = most_vars = most_cnsts = longest_row = 0
    for n, f, b in zip(mixed.names, mixed.flats, mixed.built):
        yd = dense_order(f, b[2], want[n].y)
        at_bound += int(np.count_nonzero((f.vbound > 0) & (yd == f.vbound)))
        fatpipe += int(np.count_nonzero(f.cflags & 1))
        zero_bound += int(np.count_nonzero(f.cbound == 0))
        most_vars = max(most_vars, len(f.penalty))
        most_cnsts = max(most_cnsts, len(f.cbound))
        longest_row = max(longest_row, int(np.max(np.diff(f.var_ptr), initial=0)))
        assert len(set(f.penalty.tolist())) > 1, n
    assert at_bound >= 100 and fatpipe >= 100 and zero_bound >= 50, (at_bound, fatpipe, zero_bound)
    assert most_vars > 64 and most_cnsts > 256 and longest_row > 16, (most_vars, most_cnsts, longest_row)
    f = mixed.flats[mixed.names.index("N")]
    assert (len(f.penalty), len(f.cbound), len(f.cnst_idx)) == (900, 100, 7200)  # 61,408 bytes of LDS


ALONE = A[:8] + ["B0", "C0", "E0", "N"]


@pytest.mark.parametrize("name", ALONE)
def test_member_alone_has_the_same_bytes(mixed, name):
    """The LDS layout depends on the other members (the batch's largest counts, or the member's own when those
    do not fit together: the mixed batch, 74,404 bytes): a member's values may not."""
    b = Batch([name])
    assert b.engine == L.System.RAN_BATCH
    assert b.bytes[name] == mixed.bytes[name]


def test_same_bytes_run_to_run_and_reversed(mixed):
    again, rev = Batch(MIXED), Batch(MIXED[::-1])
    assert again.engine == rev.engine == L.System.RAN_BATCH
    assert again.bytes == mixed.bytes
    assert rev.bytes == mixed.bytes
    assert again.rounds == rev.rounds == mixed.rounds


@pytest.mark.parametrize("grid", ["1", "3"])
def test_lds_restaging_across_unlike_systems(mixed, grid, monkeypatch):
    """Fewer workgroups than systems (LMMHIP_BATCH_GRID): every workgroup restages its LDS for systems of other
    sizes, a small one after a large one and the reverse; nothing of the previous system may survive."""
    monkeypatch.setenv("LMMHIP_BATCH_GRID", grid)
    b = Batch(ALTERNATING)
    assert b.engine == L.System.RAN_BATCH
    assert sorted(b.names) == sorted(MIXED)
    assert b.bytes == mixed.bytes
    assert b.rounds == mixed.rounds


# at most 600 variables (D), 300 constraints (B0) and 4,800 elements (D): 56,104 bytes of LDS, one layout for all
SAME_LAYOUT = [n for pair in zip(["D", "B0", "E0", "C0"], A) for n in pair] + A[4:12]


@pytest.mark.parametrize("grid", ["1", "3"])
def test_lds_restaging_in_the_layout_of_the_batch_maxima(mixed, grid, monkeypatch):
    """As above for a batch whose largest counts fit the LDS budget together: one layout for every system, the
    arrays of a small system spread over the allocation."""
    monkeypatch.setenv("LMMHIP_BATCH_GRID", grid)
    b = Batch(SAME_LAYOUT, flats=True)
    assert b.engine == L.System.RAN_BATCH
    assert [max(len(getattr(f, k)) for f in b.flats) for k in ("penalty", "cbound", "cnst_idx")] == [600, 300, 4800]
    assert b.bytes == {n: mixed.bytes[n] for n in SAME_LAYOUT}


def test_global_engine_on_the_same_union(mixed, want, monkeypatch):
    monkeypatch.setenv("LMMHIP_BATCH", "0")
    prec = L.get_precision()
    g = Batch(MIXED)
    assert g.engine in GLOBAL_ENGINES
    check_against_oracle(g, want, prec)
    for n in MIXED:
        bad, worst = _close(g.x[n], mixed.x[n])
        assert len(bad) == 0, (n, len(bad), worst)
        if want[n].saturated is not None:
            assert g.saturated(n, prec) == mixed.saturated(n, prec), n


def test_dispatch_with_an_over_budget_member(want):
    prec = L.get_precision()
    b = Batch(["A0", "X", "A1"])
    assert b.engine in GLOBAL_ENGINES
    check_against_oracle(b, want, prec)
    b = Batch(["A0", "A1"])
    assert b.engine == L.System.RAN_BATCH
    check_against_oracle(b, want, prec)


def scale_bounds(mod, s, cs):
    """Every constraint of positive bound gets a new one (zero bounds stay: the same flattened structure).  Script
    members: the script's constraints; synthetic ones: the active constraints (all of theirs have elements)."""
    cs = dict(enumerate(s.active_constraints())) if cs is None else cs
    K.replay(mod, [("cbound", k, round(0.75 * c.get_bound() + 0.1, 3)) for k, c in cs.items() if c.get_bound() > 0],
             sys_=s, cs=cs)


def test_device_batch_saturated_set_and_bound_updates(want):
    prec = L.get_precision()
    names = A[:12] + ["B0", "C0", "E0", "D"]
    built = [MEMBERS[n].build(L) for n in names]
    b = M.DeviceBatch([x[0] for x in built])
    assert b.kind == M.DeviceBatch.MAXMIN

    def oracle_dense(ws):
        yd = np.zeros(b.n_var)
        for i, (w, x) in enumerate(zip(ws, built)):
            ids = x[2] if isinstance(x[2], np.ndarray) else [v.h for v in x[2]]
            pos = {int(h): j for j, h in enumerate(ids)}
            yd[b.var_off[i]:b.var_off[i + 1]] = w.y[[pos[int(h)] for h in b.var_ids[i]]]
        return yd

    b.solve()
    assert b.last_engine() == L.System.RAN_BATCH
    x, sat = b.values(), b.saturated()
    yd = oracle_dense([want[n] for n in names])
    bad, worst = _close(x, yd)
    assert len(bad) == 0, (len(bad), worst)
    np.testing.assert_array_equal(sat, _sat_dense(b.flat(), yd, prec))
    assert 0 < np.count_nonzero(sat) < len(sat)
    b.solve()  # every solve re-initialises the state
    assert b.values().tobytes() == x.tobytes()
    np.testing.assert_array_equal(b.saturated(), sat)
    # new bounds, against freshly built systems carrying them (their own DeviceBatch) and the oracle
    fresh = []
    for n in names:
        s, cs, _ = MEMBERS[n].build(L)
        scale_bounds(L, s, cs)
        fresh.append(s)
    wants = [Want(MEMBERS[n], prec, scale_bounds) for n in names]
    flats = [M.export_flat(s) for s in fresh]
    cb = np.concatenate([f.cbound for f in flats])
    assert len(cb) == b.n_cnst and not np.array_equal(cb, b.arrays[5])
    assert np.array_equal(cb == 0, b.arrays[5] == 0)
    assert np.array_equal(np.concatenate([f.cnst_idx + b.cnst_off[i] for i, f in enumerate(flats)]), b.arrays[1])
    b.update_cnst_bounds(cb)
    b.solve()
    assert b.last_engine() == L.System.RAN_BATCH
    fb = M.DeviceBatch(fresh)
    fb.solve()
    assert fb.last_engine() == L.System.RAN_BATCH
    assert b.values().tobytes() == fb.values().tobytes()
    np.testing.assert_array_equal(b.saturated(), fb.saturated())
    yd = oracle_dense(wants)
    bad, worst = _close(b.values(), yd)
    assert len(bad) == 0, (len(bad), worst)
    assert not np.array_equal(yd, oracle_dense([want[n] for n in names]))
    np.testing.assert_array_equal(b.saturated(), _sat_dense(b.flat(), yd, prec))
    fb.close()
    b.close()


def degenerate_members():
    """[(system, [(variable, expected value)])], for an ordinary member [(system, its variables)]: fresh max-min
    systems."""
    out = []
    s = L.System(False)  # constraints only
    s.constraint_new(None, 3.0)
    s.constraint_new(None, 0.0)
    out.append((s, []))
    s = L.System(False)  # one variable on one constraint
    v = s.variable_new(None, 1.0, -1.0, 1)
    s.expand(s.constraint_new(None, 3.0), v, 2.0)
    out.append((s, [(v, 1.5)]))
    s = L.System(False)  # a lone enabled variable
    out.append((s, [(s.variable_new(None, 1.0), 0.0)]))
    s, _, vs = MEMBERS["A5"].build(L)  # an ordinary member between them
    out.append((s, vs))
    s = L.System(False)  # a variable of penalty 0 on a constraint
    v = s.variable_new(None, 0.0, -1.0, 1)
    s.expand(s.constraint_new(None, 3.0), v, 1.0)
    out.append((s, [(v, 0.0)]))
    s = L.System(False)  # a variable whose only constraints have bound 0 (it stays at 0), next to an ordinary one
    z0, z1, c = s.constraint_new(None, 0.0), s.constraint_new(None, 0.0), s.constraint_new(None, 4.0)
    a, v = s.variable_new(None, 1.0, -1.0, 2), s.variable_new(None, 2.0, -1.0, 1)
    s.expand(z0, a, 1.0)
    s.expand(z1, a, 0.5)
    s.expand(c, v, 2.0)
    out.append((s, [(a, 0.0), (v, 2.0)]))
    out.append((L.System(False), []))  # test_gpu_parity.py::test_edge_cases: the empty system ...
    s = L.System(False)  # ... constraints only, variables without constraints, disabled ones, a zero bound ...
    c0, c1 = s.constraint_new(None, 0.0), s.constraint_new(None, 4.0)
    a, d, lone = s.variable_new(None, 1.0, -1.0, 2), s.variable_new(None, 0.0, -1.0, 1), s.variable_new(None, 1.0)
    s.expand(c0, a, 1.0)
    s.expand(c1, a, 2.0)
    s.expand(c1, d, 1.0)
    out.append((s, [(a, 2.0), (d, 0.0), (lone, 0.0)]))
    s, _, vs = MEMBERS["A6"].build(L)
    out.append((s, vs))
    s = L.System(False)  # ... and a bounded variable below its share
    c = s.constraint_new(None, 10.0)
    x, y = s.variable_new(None, 1.0, 1.5), s.variable_new(None, 1.0)
    s.expand(c, x, 1.0)
    s.expand(c, y, 1.0)
    out.append((s, [(x, 1.5), (y, 8.5)]))
    return out


def test_degenerate_members(mixed):
    alone = degenerate_members()
    for s, _ in alone:
        s.solve()
    ms = degenerate_members()
    L.solve_batch([s for s, _ in ms])
    assert ms[0][0].last_engine() == L.System.RAN_BATCH
    n = 0
    for k, ((a, _), (s, expect)) in enumerate(zip(alone, ms)):
        xa = np.array([v.get_value() for v in a.variables()])
        xs = np.array([v.get_value() for v in s.variables()])
        bad, worst = _close(xs, xa)
        assert len(bad) == 0, (k, len(bad), worst)
        if k in (3, 8):  # the ordinary members: the bytes they have in any other company
            assert values_of(s, expect).tobytes() == mixed.bytes["A5" if k == 3 else "A6"]
            continue
        for v, x in expect:
            assert abs(v.get_value() - x) <= 1e-12, (k, v.get_value(), x)
        n += len(expect)
    assert n == 10
    assert L.lib().lmm_solve_batch((L.P * 0)(), 0) == 0


@pytest.mark.parametrize("grid", [None, "1"])
def test_dead_constraints_at_init(grid, monkeypatch):
    """What the host flatten never hands over but the upload accepts: a variable all of whose constraints have
    bound 0 (one of them FATPIPE) and a constraint without an element.  They are out from the init on; the
    variable stays at 0.  Uploaded by hand, two systems (with one workgroup: one after the other)."""
    import ctypes as ct

    import torch

    if grid:
        monkeypatch.setenv("LMMHIP_BATCH_GRID", grid)
    lib = L.lib()
    #      system 0: v0 on c0 (0) and c3 (0, FATPIPE), v1 on c0 (0) and c1 (4), c2 (5) unused; system 1: v2 on c4 (3)
    var_ptr, cnst_idx = np.array([0, 2, 4, 5], np.int64), np.array([0, 3, 0, 1, 4], np.int32)
    weight = np.array([1.0, 1.0, 1.0, 2.0, 2.0])
    pen, vbound = np.ones(3), -np.ones(3)
    cbound, cflags = np.array([0.0, 4.0, 5.0, 0.0, 3.0]), np.array([0, 0, 0, 1, 0], np.uint8)
    var_off, cnst_off = np.array([0, 2, 3], np.int64), np.array([0, 4, 5], np.int64)

    def p(a, t):
        return a.ctypes.data_as(ct.POINTER(t))

    ctx = ct.c_void_p()
    L._check_hip(lib.lmmhip_ctx_create(torch.cuda.current_device(), ct.byref(ctx)))
    try:
        L._check_hip(lib.lmmhip_upload(ctx, 3, 5, 5, p(var_ptr, ct.c_int64), p(cnst_idx, ct.c_int32),
                                       p(weight, ct.c_double), p(pen, ct.c_double), p(vbound, ct.c_double),
                                       p(cbound, ct.c_double), p(cflags, ct.c_uint8)))
        L._check_hip(lib.lmmhip_set_batch(ctx, 2, p(var_off, ct.c_int64), p(cnst_off, ct.c_int64)))
        L._check_hip(lib.lmmhip_solve(ctx, 0, L.get_precision()))
        e = ct.c_int()
        L._check_hip(lib.lmmhip_last_engine(ctx, ct.byref(e)))
        assert e.value == L.System.RAN_BATCH
        x = np.full(3, np.nan)
        L._check_hip(lib.lmmhip_get_values(ctx, p(x, ct.c_double)))
        assert np.max(np.abs(x - [0.0, 2.0, 1.5])) <= 1e-12, x
    finally:
        lib.lmmhip_ctx_destroy(ctx)


def test_device_var_rounds():
    """lmmhip_get_var_rounds: the batch engine records no per-variable rounds (an error, not stale numbers); a
    global engine's are 1 + the round that fixed the variable."""
    b = Batch(["A0", "B0"])
    assert b.engine == L.System.RAN_BATCH
    with pytest.raises(L.LmmError, match="batch engine"):
        b.systems[0].device_var_rounds()
    s = MEMBERS["B0"].build(L)[0]
    s.set_engine(L.System.ENGINE_ROUNDS)
    s.solve()
    assert s.last_engine() == L.System.RAN_ROUNDS
    st = s.last_stats()
    r, x = s.device_var_rounds(), s.device_values()
    assert r.dtype == np.int32 and len(r) == st["n_var"] == len(x) and len(r) > 64
    assert r.min() >= 0 and r.max() <= st["rounds"], (int(r.min()), int(r.max()), st["rounds"])
    assert np.all(r[x > 0] >= 1)
    assert np.count_nonzero(x > 0) > 64
