"""The resident action table (lmmhip_actions_bind / _patch / _lazy_update_solved / _events / _var_index,
simgrid_amd.step.DeviceActions): a table bound to variable slots follows every upload and flatten on the device,
and gives the bytes of the per-call path that re-uploads the table with host-computed dense indices."""
import ctypes as ct

import numpy as np
import pytest

from oracle import step_oracle as S
from simgrid_amd import lmm as L
from simgrid_amd import step as D
from tests import actions_bound as AB

pytestmark = pytest.mark.gpu

K_BLOCK, K_MAX_BLOCKS = 256, 2048  # lmm_dev.hpp kBlock, kMaxBlocks: grid_for caps the grid, the kernels stride beyond
E_ARG, E_STATE = -3, -4


# ---- 1. rebind follows the flatten ----
@pytest.mark.parametrize("n", [0, 1, K_BLOCK - 1, K_BLOCK, K_BLOCK + 1, K_BLOCK * K_MAX_BLOCKS + 1])
@pytest.mark.parametrize("way", ["selective", "full", "host_flatten"])
def test_rebind_follows_the_flatten(way, n):
    """After every solve var_index() is step.dense_index over the touched variables: through full flattens, the
    refresh path (step 5: bounds only), a freed variable, a disabled one, one whose only constraint has bound 0,
    new variables in new and in reused slots; a slot without an action, -1 and a slot past the table."""
    s = L.System(way == "selective")
    if way == "host_flatten":  # lmmhip_upload: the caller's ids are the dense indices, a slot >= n_var is not solved
        s.set_resident(False)
    cs, vs, _, _ = s.gen_maxmin_bench(1, 0)
    lone_c = s.constraint_new(None, 10.0)
    lone_v = s.variable_new(None, 1.0, -1.0, 1)
    s.expand(lone_c, lone_v, 1.0)
    live = list(vs)
    # slots of the table: -1, two past the current slot count (the second one is reached by the new variables),
    # every variable but vs[3] (a slot with no action), the lone variable; repeated up to n entries
    cand = [-1, lone_v.h + 2, lone_v.h + 40] + [v.h for v in vs if v is not vs[3]] + [lone_v.h]
    slots = np.resize(np.array(cand, np.int32), n)
    acts = D.DeviceActions(s.device_ctx(), np.full(n, -1, np.int32), np.zeros(n))
    acts.bind(slots)
    assert np.array_equal(acts.var_index(), np.full(n, -1, np.int32))  # no system on the device yet
    seen = set()
    for step in range(6):
        if step < 5:
            s.variable_free(live.pop(2 * step))
            s.update_variable_penalty(live[3 * step + 1], 0.0)  # disabled: leaves the system
            v = s.variable_new(None, 1.0, -1.0, 2)
            s.expand(cs[step], v, 1.0)
            s.expand(cs[step + 10], v, 0.5)
            live.append(v)
        if step == 2:
            s.update_constraint_bound(lone_c, 0.0)  # the lone variable's only constraint: bound 0
        if step == 4:
            s.update_constraint_bound(lone_c, 5.0)
        c = cs[step + 20]
        s.update_constraint_bound(c, c.get_bound() * 0.75)
        s.solve()
        want = AB.dense_of(s.device_touched_vars(), slots)
        got = acts.var_index()
        assert got.dtype == np.int32 and np.array_equal(got, want), (way, n, step)
        seen.add(want.tobytes())
    if n >= K_BLOCK - 1:
        assert len(seen) > 1 and (want >= 0).any() and (want < 0).any()  # the numbering did move


# ---- 2. bit-identity with the per-call path ----
@pytest.mark.parametrize("model", [D.MODEL_CPU, D.MODEL_CM02])
def test_lazy_resident_table_equals_per_call_path(model):
    a = AB.Twin(False, True, True, model)
    b = AB.Twin(True, True, True, model)
    finished = 0
    for step in range(8):
        ra, rb = a.lazy_step(step), b.lazy_step(step)
        AB.assert_same(ra, rb, (step,))
        finished += ra["nfin"] + len(ra["ids"])
    assert finished > 0


@pytest.mark.parametrize("model", [D.MODEL_CPU, D.MODEL_CM02, D.MODEL_L07])
def test_full_resident_table_equals_per_call_path(model):
    a = AB.Twin(False, False, False, model)
    b = AB.Twin(True, False, False, model)
    events = 0
    for step in range(8):
        ra, rb = a.full_step(step), b.full_step(step)
        AB.assert_same(ra, rb, (step,))
        events += ra["nev"]
    assert events > 0


# ---- 3. oracle ----
@pytest.mark.parametrize("model", [D.MODEL_CPU, D.MODEL_CM02])
def test_lazy_solved_set_matches_heap_oracle(model):
    """test_lazy_glue_matches_heap_oracle's shape with slot binding and the modified set taken on the device,
    against LazyModel fed [i for i if vi[i] >= 0] + extra."""
    rng = np.random.default_rng(23 + model)
    s = L.System(False)
    cs, vs, _, _ = s.gen_maxmin_bench(2, 1)
    n = 6000
    vslots = np.array([v.h for v in vs], np.int32)
    slots = np.where(rng.random(n) < 0.7, rng.choice(vslots, n), -1).astype(np.int32)
    slots[rng.random(n) < 0.02] = vslots.max() + 7  # past the mirror
    st = dict(remains=rng.choice([0.0, 1e-9, 1.0, 5.0, 1e3], size=n) * rng.random(n),
              max_duration=np.where(rng.random(n) < 0.3, rng.random(n) * 2, -1.0),
              penalty=np.where(rng.random(n) < 0.2, 0.0, 1.0),
              flags=np.where(rng.random(n) < 0.05, S.ACT_NOT_STARTED, 0).astype(np.uint8))
    lat_hat = (rng.random(n) < 0.2) if model == D.MODEL_CM02 else np.zeros(n, bool)
    lz = dict(last_update=np.zeros(n), last_value=np.where(rng.random(n) < 0.5, rng.random(n), 0.0),
              start_time=np.zeros(n), date=np.where(lat_hat, rng.random(n) * 1e-3, 0.0),
              heap_type=np.where(lat_hat, S.HEAP_LATENCY, S.HEAP_UNSET).astype(np.uint8))
    acts = D.DeviceActions(s.device_ctx(), np.full(n, -1, np.int32), **st)
    acts.lazy_init(**lz)
    acts.bind(slots)
    ost = {k: list(v) for k, v in st.items()}
    ost.update({k: list(v) for k, v in lz.items()})
    ost["date"] = [d if h else float("inf") for d, h in zip(ost["date"], ost["heap_type"])]
    O = S.LazyModel(model, ost)
    h = dict(st, heap_type=lz["heap_type"])
    # the hand-pushed actions: without a solved variable, and dated by a max duration (or skipped)
    no_var = slots < 0
    can_extra = np.nonzero(no_var & ((st["max_duration"] != S.NO_MAX_DURATION) | (st["penalty"] <= 0)))[0]
    now, pops = 0.0, 0
    for step in range(8):
        for j in rng.choice(len(vs), 5, replace=False):  # the system moves: new values, the refresh path
            s.update_variable_penalty(vs[int(j)], float(rng.random() + 0.5))
        s.solve()
        vi = AB.dense_of(s.device_touched_vars(), slots)
        assert np.array_equal(acts.var_index(), vi)
        x = s.device_values()
        values = [x[k] if k >= 0 else 0.0 for k in vi]
        extra = rng.permutation(can_extra)[:50]
        modified = [int(i) for i in np.nonzero(vi >= 0)[0]] + [int(i) for i in extra]
        h["heap_type"] = np.array(ost["heap_type"], np.uint8)
        h["max_duration"] = np.array(ost["max_duration"])
        bad = AB.undated(h, vi, x, modified)  # every action the loop does not skip gets a date (Model.cpp:96)
        assert not bad, bad
        nmod, nfin = acts.lazy_update_solved(model, now, extra, 1e-5, 1e-5)
        want_ev, want_fin = O.next_occuring_event_lazy(values, now, modified, 1e-5, 1e-5)
        got_ev = acts.next_occuring_event_lazy(now)
        assert nmod == len(modified) and nfin == len(want_fin) and got_ev == want_ev, (step, got_ev, want_ev)
        ids, evs = acts.events()
        assert ids.tolist() == sorted(want_fin) and set(evs.tolist()) <= {S.EV_FINISHED}
        if got_ev < 0:
            break
        now = now + got_ev
        ids, evs = acts.lazy_due(model, now, 1e-5)
        want = sorted(O.update_actions_state_lazy(now, 1e-5))
        assert list(zip(ids.tolist(), evs.tolist())) == want, step
        pops += len(want)
        dev, lzs = acts.state(), acts.lazy_state()
        for k in ("remains", "max_duration"):
            assert np.array_equal(dev[k], np.array(ost[k])), (step, k)
        for k in ("last_update", "last_value", "date"):
            assert np.array_equal(lzs[k], np.array(ost[k])), (step, k)
        assert np.array_equal(lzs["heap_type"], np.array(ost["heap_type"], np.uint8)), step
    assert pops > 0


# ---- 4. events() ----
def _solved_system():
    s = L.System(False)
    _, vs, _, _ = s.gen_maxmin_bench(1, 0)
    s.solve()
    return s, vs


def _events_of(acts):
    ev = acts.state()["events"]
    ids = np.nonzero(ev)[0].astype(np.int32)
    return ids, ev[ids]


def test_events_are_the_nonzero_entries_in_order():
    s, vs = _solved_system()
    n = 3 * K_BLOCK + 5
    rng = np.random.default_rng(3)
    slots = rng.choice(s.device_touched_vars(), n).astype(np.int32)  # every action's variable is solved
    acts = D.DeviceActions(s.device_ctx(), np.full(n, -1, np.int32), remains=rng.random(n) * 1e-3 + 1e-4,
                           max_duration=np.where(rng.random(n) < 0.5, rng.random(n) * 0.05, -1.0),
                           latency=np.where(rng.random(n) < 0.3, 1e-6, 0.0))
    acts.lazy_init()
    acts.bind(slots)
    ids, evs = acts.events()
    assert len(ids) == 0 and len(evs) == 0  # nothing ran yet
    # a Full update with events of both kinds
    nev = acts.update_actions_state(D.MODEL_CM02, 0.01, 1e-5, 1e-5)
    want = _events_of(acts)
    got = acts.events()
    assert nev == len(want[0]) > 0 and set(want[1].tolist()) > {D.EV_FINISHED}
    assert AB.same_bytes(got[0], want[0]) and AB.same_bytes(got[1], want[1])
    # the size query agrees; a capacity below it is an argument error and returns nothing
    lib, k = L.lib(), ct.c_int64()
    assert lib.lmmhip_actions_events(acts.ctx, None, None, 0, ct.byref(k)) == 0 and k.value == nev
    ib, eb = np.full(nev, -7, np.int32), np.zeros(nev, np.uint8)
    rc = lib.lmmhip_actions_events(acts.ctx, ib.ctypes.data_as(ct.POINTER(ct.c_int32)),
                                   eb.ctypes.data_as(ct.POINTER(ct.c_uint8)), nev - 1, ct.byref(k))
    assert rc == E_ARG and (ib == -7).all() and b"capacity" in lib.lmmhip_last_error()
    # a step without events: a tiny delta finishes nothing
    acts.patch(np.arange(n), remains=1e6, max_duration=-1.0, latency=0.0)
    assert acts.update_actions_state(D.MODEL_CM02, 1e-9, 1e-5, 1e-5) == 0
    assert len(acts.events()[0]) == 0 and not acts.state()["events"].any()
    # a lazy update: half of the actions are out of work
    acts.patch(np.arange(0, n, 2), remains=0.0)
    nmod, nfin = acts.lazy_update_solved(D.MODEL_CM02, 1.0, (), 1e-5, 1e-5)
    want = _events_of(acts)
    got = acts.events()
    assert nmod == n and nfin == len(want[0]) == (n + 1) // 2
    assert AB.same_bytes(got[0], want[0]) and AB.same_bytes(got[1], want[1])


# ---- 5. patch semantics ----
def _snapshot(acts):
    out = dict(acts.state())
    out.update(acts.lazy_state())
    out["var_index"] = acts.var_index()
    return out


def test_patch_partial_mask_unset_heap_and_vacant_table():
    s, vs = _solved_system()
    n = K_BLOCK + 3
    rng = np.random.default_rng(4)
    acts = D.DeviceActions(s.device_ctx(), np.full(n, -1, np.int32), remains=rng.random(n) + 1,
                           max_duration=rng.random(n) + 2, latency=rng.random(n), penalty=rng.random(n) + 0.5)
    acts.lazy_init(last_update=rng.random(n), last_value=rng.random(n), date=rng.random(n) + 5,
                   heap_type=np.full(n, D.HEAP_NORMAL, np.uint8))
    acts.bind(rng.choice([v.h for v in vs], n).astype(np.int32))
    before = _snapshot(acts)
    idx = np.array([n - 1, 0, 77, K_BLOCK], np.int32)  # unsorted on purpose
    acts.patch(idx, remains=[1.5, 2.5, 3.5, 4.5], last_value=9.0)
    after = _snapshot(acts)
    for k in before:
        want = before[k].copy()
        if k == "remains":
            want[idx] = [1.5, 2.5, 3.5, 4.5]
        if k == "last_value":
            want[idx] = 9.0
        assert AB.same_bytes(after[k], want), k
    # a heap type UNSET forces the date +inf, whatever date comes with it; a date alone is kept
    acts.patch([3, 4], heap_type=[D.HEAP_UNSET, D.HEAP_LATENCY], date=[1.0, 2.0])
    acts.patch([5], date=3.0)
    lz = acts.lazy_state()
    assert lz["heap_type"][3] == D.HEAP_UNSET and lz["date"][3] == np.inf
    assert lz["heap_type"][4] == D.HEAP_LATENCY and lz["date"][4] == 2.0 and lz["date"][5] == 3.0
    # a patched variable slot is rebound at once: -1, a solved variable, a slot past the mirror
    touched = s.device_touched_vars()
    new = np.array([-1, touched[5], touched.max() + 1000], np.int32)
    acts.patch([10, 11, 12], var_slot=new)
    assert np.array_equal(acts.var_index()[10:13], D.dense_index(touched, new))
    # an entirely vacant table: no event, no date, nothing in either next-event reduction
    acts.patch(np.arange(n), **D.VACANT)
    assert acts.next_occuring_event(with_latency=True) == -1.0
    assert acts.next_occuring_event_lazy(0.0) == -1.0
    assert acts.update_actions_state(D.MODEL_CM02, 1.0, 1e-5, 1e-5) == 0
    assert acts.lazy_update_solved(D.MODEL_CM02, 1.0, (), 1e-5, 1e-5) == (0, 0)
    ids, evs = acts.lazy_due(D.MODEL_CM02, 1.0, 1e-5)
    assert len(ids) == 0 and len(acts.events()[0]) == 0
    lz = acts.lazy_state()
    assert (lz["heap_type"] == D.HEAP_UNSET).all() and np.isinf(lz["date"]).all()
    # ... and the same table as reserve() builds it
    s2, _ = _solved_system()
    res = D.DeviceActions.reserve(s2.device_ctx(), n, lazy=True)
    assert res.next_occuring_event(True) == -1.0 and res.next_occuring_event_lazy(0.0) == -1.0
    assert (res.var_index() == -1).all()


def test_patch_errors_leave_the_table_alone():
    lib = L.lib()
    s, vs = _solved_system()
    n = 40
    ctx = s.device_ctx()
    PI32, PD, PU8 = ct.POINTER(ct.c_int32), ct.POINTER(ct.c_double), ct.POINTER(ct.c_uint8)

    def patch(idx, fields, var_slot=None, remains=None, date=None, heap_type=None):
        ix = np.asarray(idx, np.int32)
        keep = [ix] + [None if a is None else np.asarray(a, t) for a, t in
                       ((var_slot, np.int32), (remains, np.float64), (date, np.float64), (heap_type, np.uint8))]
        p = [None if a is None else a.ctypes.data_as(t) for a, t in zip(keep, (PI32, PI32, PD, PD, PU8))]
        return lib.lmmhip_actions_patch(ctx, len(ix), p[0], fields, p[1], p[2], None, None, None, None, None, None,
                                        None, None, p[3], p[4])

    c2 = ct.c_void_p()
    assert lib.lmmhip_ctx_create(-1, ct.byref(c2)) == 0
    try:  # no table yet
        assert lib.lmmhip_actions_patch(c2, 0, None, 0, *([None] * 12)) == E_STATE
        assert lib.lmmhip_actions_bind(c2, 0, None) == E_STATE
        k = ct.c_int64()
        assert lib.lmmhip_actions_events(c2, None, None, 0, ct.byref(k)) == E_STATE
        assert lib.lmmhip_actions_var_index(c2, None) == E_STATE
        assert lib.lmmhip_actions_lazy_update_solved(c2, 0, 0.0, 1e-5, 1e-5, 0, None, None, None) == E_STATE
    finally:
        lib.lmmhip_ctx_destroy(c2)
    acts = D.DeviceActions(ctx, np.full(n, -1, np.int32), remains=np.arange(n) + 1.0)
    assert patch([0], 2048, heap_type=[0]) == E_ARG and b"lazy" in lib.lmmhip_last_error()  # before lazy_upload
    assert patch([0], 1, var_slot=[1]) == E_STATE  # a variable id on an unbound table
    nm = ct.c_int64()
    assert lib.lmmhip_actions_lazy_update_solved(ctx, 0, 0.0, 1e-5, 1e-5, 0, None, ct.byref(nm), None) == E_STATE
    acts.lazy_init(date=np.arange(n) + 1.0, heap_type=np.full(n, D.HEAP_NORMAL, np.uint8))
    assert lib.lmmhip_actions_lazy_update_solved(ctx, 0, 0.0, 1e-5, 1e-5, 0, None, ct.byref(nm), None) == E_STATE
    acts.bind(np.array([v.h for v in vs[:n]], np.int32))
    before = _snapshot(acts)
    cases = {
        "index out of range": patch([1, n], 2, remains=[0.0, 0.0]),
        "negative index": patch([-1], 2, remains=[0.0]),
        "duplicate index": patch([3, 5, 3], 2, remains=[0.0, 0.0, 0.0]),
        "var_slot < -1": patch([2], 1, var_slot=[-2]),
        "unknown heap type": patch([2], 2048, heap_type=[4]),
        "null array of a set bit": patch([2], 2 | 1024, remains=[0.0]),
        "unknown field bit": patch([2], 4096),
    }
    assert all(rc == E_ARG for rc in cases.values()), cases
    assert lib.lmmhip_last_error()
    assert lib.lmmhip_actions_bind(ctx, n - 1, None) == E_ARG
    bad = np.full(n, -2, np.int32)
    assert lib.lmmhip_actions_bind(ctx, n, bad.ctypes.data_as(PI32)) == E_ARG
    ex = np.array([n], np.int32)
    assert lib.lmmhip_actions_lazy_update_solved(ctx, 0, 0.0, 1e-5, 1e-5, 1, ex.ctypes.data_as(PI32), None,
                                                 None) == E_ARG
    after = _snapshot(acts)
    for k in before:
        assert AB.same_bytes(after[k], before[k]), k
    assert patch([2], 2, remains=[7.0]) == 0 and acts.state()["remains"][2] == 7.0  # the table still works


def test_unbound_table_is_not_rebound():
    """An unbound table keeps the var_index it was uploaded with through later flattens."""
    s, vs = _solved_system()
    vi = np.array([0, -1, 3, 2], np.int32)
    acts = D.DeviceActions(s.device_ctx(), vi, np.ones(4))
    s.update_variable_penalty(vs[0], 0.0)
    s.solve()
    assert np.array_equal(acts.var_index(), vi)
    with pytest.raises(L.LmmError, match="bind first"):
        acts.lazy_init()
        acts.lazy_update_solved(D.MODEL_CPU, 0.0)


# ---- 6. scenario replays on a resident table ----
@pytest.mark.parametrize("variant,name", [(1, "surf_usage"), (2, "surf_usage2")])
def test_surf_usage_on_a_resident_table(variant, name):
    from tests import surf_scenario as SC

    be = AB.ResidentBackend()
    assert SC.run_surf_usage(be, variant) == SC.expected(name)


@pytest.mark.parametrize("run", ["lv08_lazy", "lv08_full", "cm02_lazy"])
def test_pingpong_on_a_resident_table(run):
    from tests import pingpong_scenario as PP

    be = AB.ResidentPing()
    out, ed = PP.run_pingpong(be, run)
    assert out == PP.expected(run)
    _, eo = PP.run_pingpong(PP.PingOracle(), run)
    assert ed.now == eo.now and np.float64(ed.now).tobytes() == np.float64(eo.now).tobytes()
    t = ed.net._tab  # one table for the whole run, patched a handful of times
    assert t.acts.n == AB.CAP and 0 < t.patched < 16
