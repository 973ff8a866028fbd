"""The round engine's update moving each touched constraint record as one 64-B request per quad of lanes
(LMMHIP_UPD_QUAD, the default) against the lane-by-lane path it replaces (knob 0, the same build).

The knob picks mm_update<rdq, quad> and may not change a decision of the solve: value bytes, rounds, the round of every
variable, the saturated set, the launches per slot, and per round the alive variables / elements and the re-evaluated
rows / elements.

* knob on against knob off on scripted systems (FATPIPE recompute: WIDE; many groups and a partial last one: R4L, R8L;
  mm_update<false, *>: LMMHIP_RDQ=0; four groups of a wave in flight with the tile reused group by group:
  LMMHIP_UPDQ_BLOCKS=1, where a workgroup's stride is below the number of constraints), each against the oracle;
* a hand-built hub system whose first update sees exactly m touched constraints at once, m at the edges of the quad
  passes (16 records per pass, 4 passes per group of 64 lanes).
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from tests import lmm_cases as K
from tests.test_gpu_engine_scripts import COMPACT, assert_matches_oracle, assert_same_solve, oracle_solved
from tests.test_gpu_vote0_rows import Profiled, assert_same_profile

pytestmark = pytest.mark.gpu

KNOBS = ("LMMHIP_UPD_QUAD",)
OFF, ON = ("0",), ("1",)  # (OFF: the parent's path)
# every knob that picks another round-engine variant, grid or cadence: unset unless a case sets it
OTHER = ("LMMHIP_CREC", "LMMHIP_RDQ", "LMMHIP_VOTE_BITS", "LMMHIP_SATKEY", "LMMHIP_CMP_ROWS", "LMMHIP_ROUND_HINT",
         "LMMHIP_CHUNK_MAX", "LMMHIP_UPDQ_BLOCKS", "LMMHIP_UPD_BLOCKS", "LMMHIP_ENGINE") + tuple(COMPACT)
NO_RDQ = (("LMMHIP_RDQ", "0"),)  # the mm_ready pass: mm_update<false, *>
# one update workgroup per 1,024 constraints: R4L and R8L get 5 workgroups, a wave's groups are 1,280 constraints
# apart and all LMM_UPD_K = 4 of them hold constraints (the default grid gives every wave one group at these sizes)
FEW_BLOCKS = (("LMMHIP_UPDQ_BLOCKS", "1"),)


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


@contextlib.contextmanager
def knobs(combo, extra=()):
    """The environment of one solve: the knob, `extra`, and none of the other round-engine knobs (round_plan reads
    them once per solve)."""
    env = dict(zip(KNOBS, combo), **dict(extra))
    saved = {k: os.environ.get(k) for k in KNOBS + OTHER}
    try:
        for k in KNOBS + OTHER:
            os.environ.pop(k, None)
        os.environ.update(env)
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@functools.lru_cache(maxsize=None)
def parent_path(shape, seed, extra=()):
    """The script solved with the knob off (solved once, never modified)."""
    with knobs(OFF, extra):
        return Profiled(K.engine_script(shape, seed), K.ENGINE_SHAPES[shape][1])


SCRIPTS = [("R4", 1, ()), ("R8", 1, ()), ("R8S", 0, ()), ("R8S", 1, ()), ("WIDE", 0, ()), ("WIDE", 1, ()), ("WIDE", 2, ()),
           ("R4L", 1, ()), ("R8L", 1, ()), ("R8L", 1, NO_RDQ), ("R4L", 1, FEW_BLOCKS), ("R8L", 1, FEW_BLOCKS)]


def _script_id(shape, seed, extra):
    return f"{shape}-{seed}" + "".join("-" + k[len("LMMHIP_"):].lower() + v for k, v in extra)


@pytest.mark.parametrize("shape,seed,extra", SCRIPTS, ids=[_script_id(*c) for c in SCRIPTS])
def test_knob_changes_nothing_on_scripts(shape, seed, extra):
    """The knob on against off: the same solve bit for bit, the same launches slot by slot, the same per-round
    profiles; and both meet the oracle."""
    base = parent_path(shape, seed, extra)
    assert base.rounds > 2 and np.count_nonzero(base.x) > 0
    assert_matches_oracle(base, *oracle_solved(shape, seed), (shape, seed))
    if shape.endswith("L"):
        st = base.s.last_stats()
        assert st["n_cnst"] > 4096, st  # (many groups of 64; 5,000 and 4,500 as scripted: a partial last group)
    if extra == NO_RDQ:
        assert base.launches[3] > 0, base.launches  # (the mm_ready pass ran: the update is mm_update<false, *>)
    else:
        assert base.launches[3] == 0, base.launches
    with knobs(ON, extra):
        d = Profiled(K.engine_script(shape, seed))
    assert_same_solve(base, d, (shape, seed, extra))
    assert_same_profile(base, d, (shape, seed, extra))
    assert_matches_oracle(d, *oracle_solved(shape, seed), (shape, seed, extra))


# ---- touched counts at the pass edges ----------------------------------------------------------------------------------
def hub_script(m):
    """Constraints C_0..C_{m-1} (bound 10), each holding v_i and u_i; then H (bound 1) holding every v_i; weights and
    penalties 1.  Flattening (lmm_system.cpp, flatten_maxmin) numbers the constraints in the order of the active list,
    which a constraint joins at its first expand, and the variables by creation: C_i is constraint i, H — created and
    expanded last — is constraint m, v_i is variable 2 i and u_i variable 2 i + 1.

    Round 0: every v_i votes for H (1 / m < 10 / 2), every u_i for its C_i; H alone is ready, saturates and fixes every
    v_i at 1 / m, so round 0's update sees constraints 0..m-1 touched at once and H saturated: min(m, 64) touched lanes
    in the first group of 64, the rest in the next ones.  Each C_i is left with u_i alone and is ready; round 1 fixes
    u_i at 10 - 1 / m."""
    ops = []
    for i in range(m):
        ops += [("cnst", ("C", i), 10.0), ("var", ("v", i), 1.0, -1.0, 2), ("var", ("u", i), 1.0, -1.0, 1),
                ("expand", ("C", i), ("v", i), 1.0), ("expand", ("C", i), ("u", i), 1.0)]
    ops.append(("cnst", "H", 1.0))
    ops += [("expand", "H", ("v", i), 1.0) for i in range(m)]
    return ops


# 1, 16, 17, 63, 64 touched lanes in a group (one pass, a full pass, a second pass of one quad, all but one lane, every
# lane); 65: a second group with one touched lane; 200: full groups and a partial one
HUB_SIZES = (1, 16, 17, 63, 64, 65, 200)


@pytest.mark.parametrize("m", HUB_SIZES)
def test_hub_touched_counts_at_the_pass_edges(m):
    """One update with exactly m touched constraints, ids 0..m-1 (hub_script): the oracle's values, the values worked
    out by hand, two rounds, and knob on against knob off bit for bit."""
    ops = hub_script(m)
    o, ocs, ovs = K.replay(O, ops)
    o.solve()
    with knobs(OFF):
        base = Profiled(ops)
    with knobs(ON):
        d = Profiled(ops)
    for dev in (base, d):
        assert dev.s.last_stats()["n_cnst"] == m + 1 and dev.s.last_stats()["n_var"] == 2 * m
        assert dev.rounds == 2, dev.rounds
        assert_matches_oracle(dev, o, ocs, ovs, m)
        # by hand: v = 1 / m is one correctly rounded division of exact operands (0 ulp); u = (10 - q(1 / m)) / 1, q the
        # fixed-point decrement (rounded at 2^-61 of the bound), one rounding at 10: within 1 ulp(10) = 1.8e-15 of
        # Python's 10 - 1 / m, itself one rounding
        for i in range(m):
            assert abs(dev.vs[("v", i)].get_value() - 1.0 / m) <= 1e-15, (m, i)
            assert abs(dev.vs[("u", i)].get_value() - (10.0 - 1.0 / m)) <= 1e-14, (m, i)
    assert_same_solve(base, d, m)
    assert_same_profile(base, d, m)


def bound_clamp_script(m):
    """The hub with numbers that make the update's clamp `remaining < bound * precision` (precision 1e-5) decide, so
    that the record's `bound` — the last 8 bytes of its line, which no other decision of these systems depends on —
    has to reach the owner lane: C_i has bound 100 and holds v_i with weight 8 and u_i with weight 2e-5; H holds every
    v_i with weight 1 and has bound 12.4999375 m.  H's ratio, 12.4999375, is below C_i's, 100 / 8.00002 = 12.49996...,
    so round 0 fixes every v_i at 12.4999375 and leaves C_i a remaining of 100 - 99.9995 = 5e-4 and a usage of 2e-5
    (above the precision).  5e-4 is below bound * precision = 1e-3: the remaining is clamped to 0, C_i leaves the light
    table and u_i stays at 0.  Against any threshold below 5e-4 — the record's usage, 8.00002, taken for its bound
    gives 8e-5 — C_i would stay alive and u_i end at 5e-4 / 2e-5 = 25."""
    ops = []
    for i in range(m):
        ops += [("cnst", ("C", i), 100.0), ("var", ("v", i), 1.0, -1.0, 2), ("var", ("u", i), 1.0, -1.0, 1),
                ("expand", ("C", i), ("v", i), 8.0), ("expand", ("C", i), ("u", i), 2e-5)]
    ops.append(("cnst", "H", 12.4999375 * m))
    ops += [("expand", "H", ("v", i), 1.0) for i in range(m)]
    return ops


@pytest.mark.parametrize("m", (17, 65))
def test_bound_reaches_the_owner_lane(m):
    """bound_clamp_script: every u_i stays at 0 (the oracle's answer and the one worked out by hand), knob on and off."""
    ops = bound_clamp_script(m)
    o, ocs, ovs = K.replay(O, ops)
    o.solve()
    assert all(ovs[("u", i)].get_value() == 0.0 for i in range(m))
    with knobs(OFF):
        base = Profiled(ops)
    with knobs(ON):
        d = Profiled(ops)
    for dev in (base, d):
        assert_matches_oracle(dev, o, ocs, ovs, m)
        for i in range(m):
            assert dev.vs[("u", i)].get_value() == 0.0, (m, i, dev.vs[("u", i)].get_value())
            assert abs(dev.vs[("v", i)].get_value() - 12.4999375) <= 4e-15, (m, i)  # (2 ulp of one division)
    assert_same_solve(base, d, m)
    assert_same_profile(base, d, m)
