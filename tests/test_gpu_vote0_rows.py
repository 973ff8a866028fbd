"""The round engine's 16-B row records with the compaction that leaves the elements in place (LMMHIP_CMP_ROWS),
against the path they replace (knob 0, the same build: 8-B records, the alive rows' elements copied).

The knob applies to the row-record mode of the round engine (short rows: the lane vote with groups of 4 and 8) and may
not change a decision of the solve: value bytes, rounds, the round of every variable, the saturated set, the launches
per slot, and per round the alive variables / elements and the re-evaluated rows / elements.

* knob on against knob off on scripted systems, the large ones with compactions forced into the solve;
* solve / mutate / solve on one context against a fresh context (the bounded bit and the records are per solve);
* compactions that count and decide not to rewrite (the alive bits are produced and never read).
"""
import contextlib
import functools
import os

import numpy as np
import pytest

from simgrid_amd import lmm as L
from tests import lmm_cases as K
from tests.test_gpu_engine_scripts import (COMPACT, Solved, _launches, assert_matches_oracle, assert_same_solve,
                                           oracle_solved)

pytestmark = pytest.mark.gpu

KNOBS = ("LMMHIP_CMP_ROWS",)
OFF, ON = ("0",), ("1",)  # (OFF: the parent's path)
# every knob that picks another round-engine variant or cadence: unset unless a case sets it
OTHER = ("LMMHIP_CREC", "LMMHIP_RDQ", "LMMHIP_VOTE_BITS", "LMMHIP_SATKEY", "LMMHIP_ROUND_HINT", "LMMHIP_CHUNK_MAX",
         "LMMHIP_ENGINE") + tuple(COMPACT)
# counted at every chunk's end, never rewritten
COUNT_ONLY = dict(LMMHIP_COMPACT_EVERY="2", LMMHIP_COMPACT_PCT="0", LMMHIP_CLIST_EVERY="1")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


@contextlib.contextmanager
def knobs(combo, extra=None):
    """The environment of one solve: the knob, `extra`, and none of the other round-engine knobs (round_plan reads
    them once per solve)."""
    env = dict(zip(KNOBS, combo), **(extra or {}))
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


class Profiled(Solved):
    """A Solved, plus the launches per slot of that solve and the per-round profiles of a profiled solve of the same
    system on the same context."""

    def __init__(self, ops, bracket=None):
        super().__init__(ops, "rounds", bracket)
        self.launches = _launches(self.s)
        self.s.set_profiling(True)
        self.s.device_solve()
        self.s.set_profiling(False)
        self.profile = [np.array(a) for a in self.s.round_profile() + self.s.vote_profile()]


def assert_same_profile(a, b, what):
    assert a.launches == b.launches, (what, a.launches, b.launches)
    for x, y, name in zip(a.profile, b.profile, ("alive vars", "alive elems", "re-voted rows", "re-voted elems")):
        np.testing.assert_array_equal(x, y, err_msg=f"{what} {name}")


@functools.lru_cache(maxsize=None)
def parent_path(shape, seed, extra=()):
    """The script solved with the knob off (solved once, never modified)."""
    with knobs(OFF, dict(extra)):
        return Profiled(K.engine_script(shape, seed), K.ENGINE_SHAPES[shape][1])


SCRIPTS = [(sh, seed, False) for sh in ("R4", "R8", "WIDE") for seed in (0, 1, 2)] + [("R4L", 1, True), ("R8L", 1, True)]


@pytest.mark.parametrize("shape,seed,compact", SCRIPTS, ids=[f"{a}-{b}" + ("-compact" if c else "") for a, b, c in SCRIPTS])
def test_knob_changes_nothing_on_scripts(shape, seed, compact):
    """The knob on against off: the same solve bit for bit, the same launches slot by slot, the same per-round
    profiles; and both meet the oracle.  R4L and R8L run under forced
    compactions (a count, a scan, a write and a switch of buffers at the end of every chunk)."""
    extra = tuple(sorted(COMPACT.items())) if compact else ()
    base = parent_path(shape, seed, extra)
    assert base.rounds > 2 and np.count_nonzero(base.x) > 0
    assert_matches_oracle(base, *oracle_solved(shape, seed), (shape, seed))
    if compact:
        st = base.s.last_stats()
        assert st["n_var"] > 4096 and st["n_cnst"] > 4096, st
        # (the compactions were launched: 4 launches each on top of the default cadence's)
        assert base.launches[6] >= parent_path(shape, seed).launches[6] + 4, base.launches
    with knobs(ON, dict(extra)):
        d = Profiled(K.engine_script(shape, seed))
    assert_same_solve(base, d, (shape, seed))
    assert_same_profile(base, d, (shape, seed))
    assert_matches_oracle(d, *oracle_solved(shape, seed), (shape, seed))


@pytest.mark.parametrize("shape", ["R4L", "R8L"])
def test_count_without_rewrite(shape):
    """LMMHIP_COMPACT_PCT=0: every chunk's end counts the alive rows (and, with the 16-B records, leaves their alive
    bits) and decides not to rewrite; the write returns at once and the solve stays on buffer 0."""
    base = parent_path(shape, 1)
    for combo in (OFF, ON):
        with knobs(combo, COUNT_ONLY):
            d = Solved(K.engine_script(shape, 1), "rounds")
        assert_same_solve(base, d, (shape, combo))
        assert _launches(d.s)[6] >= base.launches[6] + 4, (combo, _launches(d.s), base.launches)


# ---- re-solves on one context ------------------------------------------------------------------------------------------
def test_resolve_rebuilds_bounded_bits_and_records():
    """R8L under forced compactions, solved three times on one context: as scripted; with every ninth unbounded
    variable bounded and every seventh penalty doubled; with those bounds taken away again.  After each solve the
    bytes, rounds, per-variable rounds and saturated set of a fresh context that replayed the same operations: the
    bounded bit (cvar, records) and the records of all three buffers are written by each solve, and nothing of an
    earlier solve's buffers 1 / 2 is read."""
    ops = K.engine_script("R8L", 1)
    with knobs(ON, COMPACT):
        dev = Solved(ops, "rounds", K.ENGINE_SHAPES["R8L"][1])
        free = [k for k in dev.keys if dev.vs[k].get_bound() <= 0]
        assert len(free) > 100
        flip = free[1::9]
        steps = [[("vbound", k, 0.3) for k in flip] + [("penalty", k, 2.0) for k in dev.keys[::7]],
                 [("vbound", k, -1.0) for k in flip] + [("penalty", k, 1.0) for k in dev.keys[3::7]]]
        done = list(ops)
        rounds = [dev.rounds]
        for n, upd in enumerate(steps):
            K.replay(L, upd, sys_=dev.s, cs=dev.cs, vs=dev.vs)
            done += upd
            dev.solve()
            if n == 0:
                assert K.fixed_at_bound({k: dev.vs[k] for k in flip}) > 0  # (some of the new bounds bind)
            fresh = Solved(done, "rounds")
            assert_same_solve(dev, fresh, ("step", n))
            assert _launches(dev.s)[6] > 8  # (compactions ran)
            rounds.append(dev.rounds)
        assert len(set(rounds)) > 1, rounds
    with knobs(OFF, COMPACT):  # the last state once more on the parent's path
        assert_same_solve(Solved(done, "rounds"), dev, "knob off")
