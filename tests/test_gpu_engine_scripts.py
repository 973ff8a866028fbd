"""Every max-min engine on scripted systems (tests/lmm_cases.random_script).

The round engine, the frontier engine and the persistent engine otherwise meet the oracle on the regular generators
only (gen_synthetic: 8 elements per row, no zero penalty, no frees or updates; the platforms).  Here each of them is
forced (set_engine) onto scripts with zero weights, zero penalties, zero-bound constraints, duplicate elements,
expand_add, concurrency staging, FATPIPE, frees and penalty / bound updates, in shapes chosen so that every vote kernel
runs (K.ENGINE_SHAPES: the lane vote with groups of 4 and 8, mm_vote<16>, <32>, <64>, and a few constraints of very
high degree):

* each engine against the oracle, and the three engines against each other bit for bit (values, round count, the
  round that fixed every variable);
* the round engine's variants (row records, ready queue, change stamps, kSatKey) with the alive-row compaction and the
  constraint-list rewrite forced to happen inside these short solves;
* solve / mutate / solve again on one context against a fresh context, per engine;
* degenerate systems under the forced multi-launch engines (nothing flattened: launches sized by 0).
"""
import ctypes as ct
import functools
import itertools
import json
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K

pytestmark = pytest.mark.gpu

ENGINES = {"rounds": (L.System.ENGINE_ROUNDS, L.System.RAN_ROUNDS),
           "frontier": (L.System.ENGINE_FRONTIER, L.System.RAN_FRONTIER),
           "persistent": (L.System.ENGINE_PERSISTENT, L.System.RAN_PERSISTENT)}
MAIN_SHAPES = ("R4", "R8", "R16", "R32", "R64", "WIDE")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


def _launches(s):
    """Kernel launches per slot of the last solve (lmmhip_stats.kernel_launches; 6 = termination test, polls,
    compactions)."""
    st = L.LmmhipStats()
    assert L.lib().lmmhip_get_stats(s.device_ctx(), ct.byref(st)) == 0
    return list(st.kernel_launches)


class Solved:
    """A script replayed on the device and solved by one engine: the system, its constraints and variables by script
    key, the values in key order, and the device's view of the solve."""

    def __init__(self, ops, engine, check_bracket=None):
        self.s, self.cs, self.vs = K.replay(L, ops)
        if check_bracket is not None:
            lo, hi = check_bracket
            mean = K.mean_row(M.export_flat(self.s))
            assert lo < mean <= hi, mean  # (the vote kernel the shape is here for)
        self.s.set_engine(ENGINES[engine][0])
        self.engine = engine
        self.solve()

    def solve(self):
        self.s.solve()
        assert self.s.last_engine() == ENGINES[self.engine][1]
        if self.engine == "persistent":
            assert self.s.engine_fallbacks() == 0
        self.keys = sorted(self.vs)
        self.x = self.s.values_of([self.vs[k].h for k in self.keys])
        self.rounds = self.s.last_stats()["rounds"]
        self.var_rounds = self.s.device_var_rounds()
        self.sat = self.s.device_saturated()
        self.launches6 = _launches(self.s)[6]


def assert_same_solve(a, b, what=""):
    """Two device solves took the same decisions: value bytes, rounds, the round of every variable, saturated set."""
    assert a.keys == b.keys, what
    assert a.rounds == b.rounds, (what, a.rounds, b.rounds)
    assert a.x.tobytes() == b.x.tobytes(), (what, float(np.max(np.abs(a.x - b.x))))
    np.testing.assert_array_equal(a.var_rounds, b.var_rounds, err_msg=str(what))
    np.testing.assert_array_equal(a.sat, b.sat, err_msg=str(what))


def assert_matches_oracle(dev, osys, ocs, ovs, what=""):
    assert sorted(ovs) == dev.keys, what
    _, bad = K.compare_values(dev.vs, ovs)
    assert not bad, (what, bad[:5])
    prec = L.get_precision()
    assert K.saturated(dev.s, dev.cs, prec) == K.saturated(osys, ocs, prec), what


@functools.lru_cache(maxsize=None)
def oracle_solved(shape, seed):
    """The oracle's solution of a shape's script (solved once, read by every engine's test)."""
    o, ocs, ovs = K.replay(O, K.engine_script(shape, seed))
    o.solve()
    return o, ocs, ovs


@functools.lru_cache(maxsize=None)
def rounds_solved(shape, seed):
    """The round engine's solve of a shape's script under the default knobs: what the other engines and the round
    engine's variants are compared with bit for bit (solved once, never modified)."""
    return Solved(K.engine_script(shape, seed), "rounds", K.ENGINE_SHAPES[shape][1])


SHAPE_SEEDS = [(sh, seed) for sh in MAIN_SHAPES for seed in K.ENGINE_SHAPES[sh][2]]


@pytest.mark.parametrize("engine", sorted(ENGINES))
@pytest.mark.parametrize("shape,seed", SHAPE_SEEDS, ids=[f"{a}-{b}" for a, b in SHAPE_SEEDS])
def test_engines_on_scripts(shape, seed, engine):
    """Each engine, forced, against the oracle (values and saturated set) and against the round engine bit for bit:
    values, round count, the round that fixed every variable, the saturated set."""
    o, ocs, ovs = oracle_solved(shape, seed)
    assert K.fixed_at_bound(ovs) > 0 and o.last_rounds > 1
    d = Solved(K.engine_script(shape, seed), engine, K.ENGINE_SHAPES[shape][1])
    assert np.count_nonzero(d.x) > 0 and d.rounds > 1
    assert_matches_oracle(d, o, ocs, ovs, (shape, seed, engine))
    assert_same_solve(rounds_solved(shape, seed), d, (shape, seed, "rounds / " + engine))


# (LMMHIP_CREC, LMMHIP_RDQ, LMMHIP_VOTE_BITS) of test_round_engine_variants_bit_identical x LMMHIP_SATKEY of test_gpu_satkey
VARIANTS = [dict(LMMHIP_CREC=c, LMMHIP_RDQ=q, LMMHIP_VOTE_BITS=b, LMMHIP_SATKEY=k)
            for (c, q, b), k in itertools.product((("0", "0", "1"), ("1", "0", "1"), ("1", "1", "1"), ("1", "1", "0")),
                                                  ("1", "0"))]
# the alive rows re-counted and rewritten, and the constraint list rebuilt, at the end of every chunk of rounds (the
# defaults, every 48 and 8 rounds when under 75 % of the rows are alive, leave a solve of a few dozen rounds untouched)
COMPACT = dict(LMMHIP_COMPACT_EVERY="2", LMMHIP_COMPACT_PCT="100", LMMHIP_CLIST_EVERY="1")


# (the large shapes with the compaction knobs only: without them they repeat what R4 and R8 show, at 3x the time)
VARIANT_CASES = [(sh, i, c) for sh in ("R4", "R8", "R4L", "R8L") for i in range(len(VARIANTS)) for c in (False, True)
                 if c or not sh.endswith("L")]


@pytest.mark.parametrize("shape,variant,compact", VARIANT_CASES,
                         ids=[f"{sh}-" + "".join(VARIANTS[i].values()) + ("-compact" if c else "") for sh, i, c in VARIANT_CASES])
def test_round_engine_variants_on_scripts(shape, variant, compact, monkeypatch):
    """Every vote / ready variant of the round engine (ids: CREC RDQ VOTE_BITS SATKEY), with and without forced
    compactions, gives the default's bytes, round count, per-variable rounds and saturated set, and the default meets
    the oracle.  R4 and R8 are below the 4096 rows / constraints under which the round engine never compacts (the knobs
    must change nothing there); R4L and R8L are above, and the compaction launches are counted (kernel_launches 6)."""
    seed = 1
    for k in list(VARIANTS[0]) + list(COMPACT):
        monkeypatch.delenv(k, raising=False)
    base = rounds_solved(shape, seed)
    assert base.rounds > 2 and np.count_nonzero(base.x) > 0
    if variant == 0:
        assert_matches_oracle(base, *oracle_solved(shape, seed), shape)
    large = shape.endswith("L")
    if large:
        st = base.s.last_stats()
        assert st["n_var"] > 4096 and st["n_cnst"] > 4096, st
    env = dict(VARIANTS[variant], **(COMPACT if compact else {}))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    d = Solved(K.engine_script(shape, seed), "rounds")
    assert_same_solve(base, d, (shape, env))
    # the knobs add nothing else to slot 6 (the chunks, hence the termination tests and polls, are the default's):
    # 4 more launches are one whole row compaction (count, scan, write) and the switch of the buffers
    if large and compact:
        assert _launches(d.s)[6] >= base.launches6 + 4, (env, _launches(d.s)[6], base.launches6)


# ---- every mode of the round engine (simgrid_amd/csrc/lmm_round_mode.hpp) --------------------------------------------
# the nine vote modes by their knobs: (name, LMMHIP_CREC, LMMHIP_CMP_ROWS, LMMHIP_RDQ, LMMHIP_SATKEY); without row records
# (Arrays) the queue and the filter do not exist, whatever their knobs say
ROUND_MODES = [("Arrays", "0", "1", "1", "1")]
ROUND_MODES += [(f"{form}-q{q}-f{f}", "1", rows, q, f)
                for form, rows in (("Rec8", "0"), ("Rec16", "1")) for q in "01" for f in "01"]
MODE_KNOBS = ("LMMHIP_CREC", "LMMHIP_CMP_ROWS", "LMMHIP_RDQ", "LMMHIP_SATKEY")
# (mode, forced compactions): every mode below the compaction threshold; above it, under COMPACT, the three row forms
# x the queue — there the records and the two compaction families matter
MODE_CASES = [(m, False) for m in ROUND_MODES]
MODE_CASES += [(("Arrays-q1", "0", "1", "1", "1"), True), (("Arrays-q0", "0", "1", "0", "1"), True)]
MODE_CASES += [(m, True) for m in ROUND_MODES[1:] if m[0].endswith("f1")]


@pytest.mark.parametrize("mode,compact", MODE_CASES, ids=[m[0] + ("-compact" if c else "") for m, c in MODE_CASES])
def test_every_round_mode_matches_the_default(mode, compact, monkeypatch):
    """Each of the nine vote modes, in both forms of the lane vote (LMMHIP_VOTE_BITS 1, 0) and both update paths
    (LMMHIP_UPD_QUAD 1, 0), on R4 seed 0 (below the 4096 rows under which nothing compacts); and the three row forms x
    the ready queue on R4L seed 1 with the compactions forced.  Every solve gives the default's bytes, round count,
    per-variable rounds and saturated set, and the default meets the oracle.  The mm_ready pass (slot 3) is launched
    exactly when the mode has no ready queue: the one way a test sees which family of kernels ran."""
    shape, seed = ("R4L", 1) if compact else ("R4", 0)
    for k in MODE_KNOBS + ("LMMHIP_VOTE_BITS", "LMMHIP_UPD_QUAD", "LMMHIP_UPD_BLOCKS", "LMMHIP_UPDQ_BLOCKS") + tuple(COMPACT):
        monkeypatch.delenv(k, raising=False)
    base = rounds_solved(shape, seed)
    assert base.rounds > 2 and np.count_nonzero(base.x) > 0
    assert_matches_oracle(base, *oracle_solved(shape, seed), shape)
    name, crec = mode[0], mode[1]
    queue = crec == "1" and mode[3] == "1"
    for bits, quad in (("1", "1"),) if compact else itertools.product("10", "10"):
        env = dict(zip(MODE_KNOBS, mode[1:]), LMMHIP_VOTE_BITS=bits, LMMHIP_UPD_QUAD=quad, **(COMPACT if compact else {}))
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        d = Solved(K.engine_script(shape, seed), "rounds")
        assert_same_solve(base, d, (name, env))
        n = _launches(d.s)
        assert n[2] > 0 and n[5] > 0 and (n[3] == 0) == queue, (name, env, n)
        if compact:  # (as in test_round_engine_variants_on_scripts: at least one whole row compaction and the switch)
            assert n[6] >= base.launches6 + 4, (name, env, n[6], base.launches6)


# ---- the launch sequence of the two round-chain engines ----------------------------------------------------------------
# (shape, engine, forced compactions): the small shapes are below the 4096 rows / constraints under which nothing
# compacts, the L ones are the smallest above them; the frontier engine has no compaction knobs
LAUNCH_CASES = [(sh, eng, False) for sh in ("R4", "R8", "R16", "R4L", "R8L") for eng in ("rounds", "frontier")]
LAUNCH_CASES += [(sh, "rounds", True) for sh in ("R4L", "R8L")]
LAUNCH_RECORD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "round_chain_launches.json")


def launch_case_id(shape, engine, compact):
    return f"{shape}-{engine}" + ("-compact" if compact else "")


def launch_counts(shape, engine):
    """kernel_launches (8 slots) of a first solve of the shape's script (seed 1) and of a second solve of the same
    system on the same context, which chunks by the first one's round count (the hint)."""
    d = Solved(K.engine_script(shape, 1), engine)
    first = _launches(d.s)
    d.s.device_solve()
    return [first, _launches(d.s)]


@pytest.mark.parametrize("shape,engine,compact", LAUNCH_CASES, ids=[launch_case_id(*c) for c in LAUNCH_CASES])
def test_round_chain_launch_sequence(shape, engine, compact, monkeypatch):
    """The launches per slot of the round engine and the frontier engine, for an unhinted and a hinted solve, equal the
    record taken before their host side became a plan per solve and one chunk driver (round_chain_launches.json: the
    counts depend on the control words only, not on the number of CUs, since every poll waits for the previous chunk's
    words).  A change of the chunk policy, the compaction cadence or a kernel's place in the round shows here; a change
    that means to alter them re-records the file."""
    for k in list(VARIANTS[0]) + list(COMPACT) + ["LMMHIP_ROUND_HINT", "LMMHIP_CHUNK_MAX"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in (COMPACT if compact else {}).items():
        monkeypatch.setenv(k, v)
    with open(LAUNCH_RECORD) as f:
        want = json.load(f)["launches"][launch_case_id(shape, engine, compact)]
    got = launch_counts(shape, engine)
    assert len(got[0]) == 8 and len(got[1]) == 8
    assert got == want, (got, want)


def _mutations(step, vkeys, ckeys):
    """The penalty / vbound / cbound / free ops of tests/test_gpu_parity.py::test_resolve_after_mutations, on the keys
    alive at that step."""
    upd = [("penalty", k, 2.0) for k in vkeys[step::7]] + [("vbound", k, 0.3) for k in vkeys[1 + step::9]]
    upd += [("cbound", k, 5.0 + step) for k in ckeys[step::5]] + [("free", k) for k in vkeys[2 + step::11]]
    return upd


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("engine", sorted(ENGINES))
def test_resolve_on_one_context_per_engine(engine, seed):
    """Solve, mutate (penalties, variable and constraint bounds, frees), solve again, four times on one context: after
    every step the oracle's values, and the bytes, rounds, per-variable rounds and saturated set of a fresh context of
    the same engine that replayed the same operations (no key, stamp, queue, round hint or frontier map of the previous
    solve survives).  Seed 0 has concurrency limits: its frees enable staged variables.  The shape is R8S, a quarter of
    R8 in the same bracket: the test builds the system five times."""
    ops = K.engine_script("R8S", seed)
    dev = Solved(ops, engine, K.ENGINE_SHAPES["R8S"][1])
    o, ocs, ovs = K.replay(O, ops)
    o.solve()
    done = list(ops)
    rounds = []
    for step in range(4):
        if step:
            upd = _mutations(step - 1, list(ovs), list(ocs))
            K.replay(L, upd, sys_=dev.s, cs=dev.cs, vs=dev.vs)
            K.replay(O, upd, sys_=o, cs=ocs, vs=ovs)
            done += upd
            dev.solve()
            o.solve()
        assert_matches_oracle(dev, o, ocs, ovs, (engine, seed, step))
        fresh = Solved(done, engine)
        assert_same_solve(dev, fresh, (engine, seed, step))
        rounds.append(dev.rounds)
    assert len(set(rounds)) > 1, rounds  # (the solves differ: the previous one's round hint was wrong at least once)


# ---- degenerate systems: what the flatten leaves may be empty --------------------------------------------------------
def _sys_empty(Mod):
    return Mod.System(False), []


def _sys_constraints_only(Mod):
    s = Mod.System(False)
    for b in (1.0, 0.0, 3.5):
        s.constraint_new(None, b)
    return s, []


def _sys_single(Mod):
    s = Mod.System(False)
    c = s.constraint_new(None, 3.0)
    v = s.variable_new(None, 2.0)
    s.expand(c, v, 1.5)
    return s, [v]


def _sys_all_penalties_zero(Mod):
    s = Mod.System(False)
    cs = [s.constraint_new(None, 2.0 + i) for i in range(3)]
    vs = [s.variable_new(None, 0.0, -1.0, 2) for _ in range(5)]
    for i, v in enumerate(vs):
        s.expand(cs[i % 3], v, 1.0)
        s.expand(cs[(i + 1) % 3], v, 0.5)
    return s, vs


def _sys_all_bounds_zero(Mod):
    s = Mod.System(False)
    cs = [s.constraint_new(None, 0.0) for _ in range(3)]
    vs = [s.variable_new(None, 1.0 + i, 2.0 if i == 1 else -1.0, 2) for i in range(5)]
    for i, v in enumerate(vs):
        s.expand(cs[i % 3], v, 1.0)
        s.expand(cs[(i + 1) % 3], v, 0.5)
    return s, vs


def _sys_lone_variable(Mod):
    s = Mod.System(False)
    c = s.constraint_new(None, 6.0)
    a, b = s.variable_new(None, 1.0), s.variable_new(None, 2.0)
    lone = s.variable_new(None, 1.0, 4.0)
    s.expand(c, a, 1.0)
    s.expand(c, b, 1.0)
    return s, [a, b, lone]


def _sys_edge_mixed(Mod):  # tests/test_gpu_parity.py::test_edge_cases, second system
    s = Mod.System(False)
    c0 = s.constraint_new(None, 0.0)
    c1 = s.constraint_new(None, 4.0)
    a = s.variable_new(None, 1.0, -1.0, 2)
    b = s.variable_new(None, 0.0, -1.0, 1)
    lone = s.variable_new(None, 1.0)
    s.expand(c0, a, 1.0)
    s.expand(c1, a, 2.0)
    s.expand(c1, b, 1.0)
    return s, [a, b, lone]


def _sys_edge_bounded(Mod):  # test_edge_cases, third system
    s = Mod.System(False)
    c = s.constraint_new(None, 10.0)
    x = s.variable_new(None, 1.0, 1.5)
    y = s.variable_new(None, 1.0)
    s.expand(c, x, 1.0)
    s.expand(c, y, 1.0)
    return s, [x, y]


def _sys_chain3(Mod):
    """Three variables fixed one per round (each constraint is ready only once the previous one has saturated): as
    many rounds as variables, the case a round guard that counts QUEUED rounds gets wrong — the polls are one chunk
    behind, and 6 rounds are queued when the words of the first two arrive."""
    s = Mod.System(False)
    c1, c2, c3 = (s.constraint_new(None, b) for b in (1.0, 3.0, 6.0))
    v1, v2, v3 = (s.variable_new(None, 1.0, -1.0, 2) for _ in range(3))
    s.expand(c1, v1, 1.0)
    s.expand(c2, v1, 1.0)
    s.expand(c2, v2, 1.0)
    s.expand(c3, v2, 1.0)
    s.expand(c3, v3, 1.0)
    return s, [v1, v2, v3]


DEGENERATE = {"chain3": (_sys_chain3, [1.0, 2.0, 4.0]),
              "empty": (_sys_empty, []), "constraints_only": (_sys_constraints_only, []),
              "single": (_sys_single, [2.0]), "all_penalties_zero": (_sys_all_penalties_zero, [0.0] * 5),
              "all_bounds_zero": (_sys_all_bounds_zero, [0.0] * 5), "lone_variable": (_sys_lone_variable, [4.0, 2.0, 0.0]),
              "edge_mixed": (_sys_edge_mixed, [2.0, 0.0, 0.0]), "edge_bounded": (_sys_edge_bounded, [1.5, 8.5])}


@pytest.mark.parametrize("engine", ["rounds", "frontier"])
@pytest.mark.parametrize("name", sorted(DEGENERATE))
def test_degenerate_systems_forced_engine(name, engine):
    """Systems whose flattened form is empty or tiny, under the forced multi-launch engines: a clean return (no launch
    of zero workgroups, no round guard) and the oracle's values, which are also worked out by hand.  Solved twice on
    the context, the second time after a bound update that changes nothing structural."""
    build, want = DEGENERATE[name]
    s, vs = build(L)
    o, ovs = build(O)
    s.set_engine(ENGINES[engine][0])
    s.solve()
    o.solve()
    x = [v.get_value() for v in vs]
    y = [v.get_value() for v in ovs]
    assert all(K.close(a, b) for a, b in zip(x, y)), (x, y)
    assert all(abs(a - b) < 1e-12 for a, b in zip(x, want)), (x, want)
    # again on the same context after a mutation (an added, unused constraint; every variable's bound rewritten)
    s.constraint_new(None, 1.0)
    o.constraint_new(None, 1.0)
    for v, ov in zip(vs, ovs):
        s.update_variable_bound(v, v.get_bound())
        o.update_variable_bound(ov, ov.get_bound())
    s.solve()
    o.solve()
    assert [v.get_value() for v in vs] == x
    assert all(K.close(a.get_value(), b.get_value()) for a, b in zip(vs, ovs))
