"""Every engine in turn on one device context.

A context holds one uploaded system (its Dev, lmm_dev.hpp) and the private buffers of each engine: the round engine's
mode buffers, the frontier engine's fields (FrDev), FairBottleneck's (FbDev; the one-context solve paced by progress
words or polled, and the sharded protocol with the caller's exchange buffers).  What one engine's solve leaves behind
must not reach the next one's: a solve on a context that has run every other engine before gives the bytes, and the
rounds, of the same solve on a fresh context.  The solves go through lmmhip_ctx_set_engine / lmmhip_solve directly, on
the upload of one System: lmmhip_solve takes the solver as an argument, and a host upload (lmmhip_upload) serves both
kinds — a resident flatten is built for one kind and refuses the other, so the System is taken out of resident mode.
"""
import ctypes as ct

import numpy as np
import pytest

from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests.test_gpu_engines import _synthetic

pytestmark = pytest.mark.gpu

S = L.System
MAXMIN, FAIR = 0, 1  # LMMHIP_KIND_*
# (what to run, what lmmhip_last_engine must say): the max-min engines by their ENGINE_* constant, FairBottleneck by
# the value of LMMHIP_FB_PACE
ROUNDS = (MAXMIN, S.ENGINE_ROUNDS, S.RAN_ROUNDS)
FRONTIER = (MAXMIN, S.ENGINE_FRONTIER, S.RAN_FRONTIER)
PERSISTENT = (MAXMIN, S.ENGINE_PERSISTENT, S.RAN_PERSISTENT)
FB_PACED = (FAIR, "1", S.RAN_FB_ROUNDS)
FB_POLLED = (FAIR, "0", S.RAN_FB_ROUNDS)
TURNS = [ROUNDS, FRONTIER, FB_PACED, PERSISTENT, FRONTIER, FB_POLLED, ROUNDS]


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


def _stress_system():
    """The 2,000 x 20,000 stress system of tests/test_gpu_engines.py (penalties {1,2,4}, 10 % bounded, 5 % FATPIPE),
    uploaded once."""
    s = S(False)
    s.set_resident(False)
    _synthetic(2000, 20000, 3, True)(s)
    s.prepare()
    return s


def _solve(s, turn, monkeypatch):
    """One solve on s's context: (values in the dense order, device rounds, lmmhip_last_engine)."""
    kind, how, _ = turn
    lib, ctx = L.lib(), s.device_ctx()
    if kind == MAXMIN:
        assert lib.lmmhip_ctx_set_engine(ctx, how) == 0
    else:
        monkeypatch.setenv("LMMHIP_FB_PACE", how)
    assert lib.lmmhip_solve(ctx, kind, L.get_precision()) == 0, lib.lmmhip_last_error().decode()
    st = L.LmmhipStats()
    assert lib.lmmhip_get_stats(ctx, ct.byref(st)) == 0
    return s.device_values(), st.rounds, s.last_engine()


def test_every_engine_in_turn_on_one_context(monkeypatch):
    fresh = {turn: _solve(_stress_system(), turn, monkeypatch) for turn in sorted(set(TURNS), key=TURNS.index)}
    s = _stress_system()
    for i, turn in enumerate(TURNS):
        x, rounds, ran = _solve(s, turn, monkeypatch)
        want, want_rounds, _ = fresh[turn]
        assert ran == turn[2], (i, turn, ran)
        assert rounds == want_rounds, (i, turn, rounds, want_rounds)
        assert x.tobytes() == want.tobytes(), (i, turn, int(np.count_nonzero(x != want)))
    # the three max-min engines take the same decisions, and the two ways of ending a FairBottleneck solve the same
    for turn in (FRONTIER, PERSISTENT):
        assert fresh[turn][1] == fresh[ROUNDS][1], (turn, fresh[turn][1], fresh[ROUNDS][1])
        assert fresh[turn][0].tobytes() == fresh[ROUNDS][0].tobytes(), turn
    assert fresh[FB_POLLED][0].tobytes() == fresh[FB_PACED][0].tobytes()
    for turn, (x, rounds, _) in fresh.items():
        assert rounds > 0 and np.all(np.isfinite(x)) and np.any(x > 0), turn


def test_sharded_fb_right_after_a_paced_solve_on_the_same_contexts(monkeypatch):
    """A two-shard in-process sharded FairBottleneck solve (the driver of test_c5_sharded_matches_single_context) on
    contexts that have just run a paced one-context solve: each shard's context first solves its own variable block
    alone (progress words, locality order, its own exchange buffers), then the sharded protocol begins again on it with
    the caller's buffers.  400 L07 flows on the example dragonfly, FATPIPE loopbacks included; the bytes of the
    one-context solve of the whole system."""
    from tests.test_gpu_multi import device_shard_maker
    from tests.test_multi import fb_pair

    monkeypatch.setenv("LMMHIP_FB_PACE", "1")
    s, _, _ = fb_pair()
    f = M.export_flat(s)
    s.solve()
    assert s.last_engine() == S.RAN_FB_ROUNDS
    want = s.values_of(f.var_ids)
    plan = M.FbShardPlan(f, 2)
    gather = M.FbGather(plan, device=True)
    shards = []
    try:
        for p in range(2):
            sh = device_shard_maker(shards)(plan, p, gather)
            assert L.lib().lmmhip_solve(sh.ctx, FAIR, L.get_precision()) == 0, L.lib().lmmhip_last_error().decode()
            e = ct.c_int()
            assert L.lib().lmmhip_last_engine(sh.ctx, ct.byref(e)) == 0 and e.value == S.RAN_FB_ROUNDS
        for sh in shards:
            sh.begin()
        M.fb_solve_sharded(shards, M.LocalExchange(), gather)
        x = np.zeros(len(f.penalty))
        for sh in shards:
            x[sh.idx] = sh.values()
    finally:
        for sh in shards:
            sh.close()
    assert np.any(want > 0)
    assert x.tobytes() == want.tobytes(), int(np.count_nonzero(x != want))
