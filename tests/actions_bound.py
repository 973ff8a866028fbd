"""TEST INFRASTRUCTURE ONLY: helpers of tests/test_gpu_actions_bound.py — the resident action table
(lmmhip_actions_bind / _patch / _lazy_update_solved / _events, simgrid_amd.step.DeviceActions).

  * Twin — one System + one table of actions driven by a scripted sequence of mutations, either the per-call way
    (re-upload the table after every solve with step.dense_index over the touched variables, explicit modified
    list) or the resident way (upload once, bind, patch what the script changed, lazy_update_solved).  Two Twins
    fed the same script must hold the same bytes after every pass.
  * ResidentBackend / ResidentPing — the scenario backends of tests/surf_scenario.py and tests/pingpong_scenario.py
    over ONE table per model: a shadow of what the device holds, a patch of exactly the actions whose host record
    differs from it, and the assertion that the device then equals the host records.
"""
import numpy as np

from simgrid_amd import lmm as L
from simgrid_amd import step as D
from tests import pingpong_scenario as PP
from tests import surf_scenario as SC

FIELDS = list(D.PATCH_FIELDS)
STATE_FIELDS = ("remains", "max_duration", "latency", "penalty")
LAZY_FIELDS = ("last_update", "last_value", "date", "heap_type")
FULL_UPLOAD = ("remains", "max_duration", "latency", "penalty", "sharing_penalty", "flags")
LAZY_UPLOAD = ("last_update", "last_value", "start_time", "date", "heap_type")


def vacant_table(cap):
    return {k: np.full(cap, D.VACANT[k], D.PATCH_FIELDS[k][1]) for k in FIELDS}


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dense_of(touched, slots):
    """step.dense_index(touched, slots), computed once per distinct slot (the table may be large)."""
    slots = np.asarray(slots, np.int32)
    uniq, inv = np.unique(slots, return_inverse=True)
    return D.dense_index(touched, uniq)[inv].astype(np.int32) if len(slots) else np.zeros(0, np.int32)


def undated(h, vi, values, idx):
    """The actions of `idx` the lazy loop does not skip and that would get no date (DIE_IMPOSSIBLE, Model.cpp:96):
    no share and no max duration."""
    bad = []
    for i in idx:
        skip = (h["flags"][i] & D.ACT_NOT_STARTED) or h["penalty"][i] <= 0 or h["heap_type"][i] == D.HEAP_LATENCY
        value = values[vi[i]] if vi[i] >= 0 else 0.0
        if not skip and not (value > 0 or h["max_duration"][i] != D.NO_MAX_DURATION):
            bad.append(int(i))
    return bad


class Twin:
    """maxmin_bench 'medium' run `run` + one action per variable in a table of `cap` entries; script(step) mutates
    the System and the host records (self.h) and notes which fields of which actions it changed."""

    def __init__(self, bound, selective, lazy, model, run=0, cap=128, seed=5):
        self.bound, self.lazy, self.model, self.cap = bound, lazy, model, cap
        self.s = L.System(selective)
        self.cs, vs, _, _ = self.s.gen_maxmin_bench(1, run)
        rng = np.random.default_rng(seed)
        nv = len(vs)
        self.var = {i: vs[i] for i in range(nv)}  # action index -> its Variable
        h = self.h = vacant_table(cap)
        h["var_slot"][:nv] = [v.h for v in vs]
        h["remains"][:nv] = rng.choice([1e-9, 1.0, 5.0, 1e3], size=nv) * rng.random(nv)
        h["max_duration"][:nv] = np.where(rng.random(nv) < 0.3, rng.random(nv) * 2, -1.0)
        h["penalty"][:nv] = 1.0
        h["sharing_penalty"][:nv] = rng.random(nv) + 0.5
        if not lazy:
            h["latency"][:nv] = np.where(rng.random(nv) < 0.3, rng.random(nv) * 1e-3, 0.0)
            h["flags"][:nv] = rng.choice([0, 0, 0, D.ACT_NO_CNST, D.ACT_SUSPENDED], size=nv)
        else:
            h["flags"][:nv] = np.where(rng.random(nv) < 0.05, D.ACT_NOT_STARTED, 0)
            h["last_value"][:nv] = np.where(rng.random(nv) < 0.5, rng.random(nv), 0.0)
            if model == D.MODEL_CM02:  # latency hats: the variable is disabled until the latency is paid
                for i in np.nonzero(rng.random(nv) < 0.15)[0]:
                    h["heap_type"][i], h["date"][i] = D.HEAP_LATENCY, (1 + i) * 1e-4
                    self.s.update_variable_penalty(self.var[int(i)], 0.0)
        # two actions without a variable, kept in the modified set by hand (a sleep: cpu_cas01.cpp:193-196)
        self.extra = [nv, nv + 1]
        for i in self.extra:
            h["remains"][i], h["max_duration"][i], h["penalty"][i] = 1.0, 3.0 + i, 1.0
        self.next_free = nv + 2
        self.rng = np.random.default_rng(seed + 1)
        self.dirty = {}
        self.acts = None
        self.now = 0.0

    # ---- the script ----
    def touch(self, i, *fields):
        self.dirty.setdefault(int(i), set()).update(fields)

    def retire(self, i):
        self.s.variable_free(self.var.pop(i))
        for k in FIELDS:
            self.h[k][i] = D.VACANT[k]
        self.touch(i, *FIELDS)

    def script(self, step):
        s, h, rng = self.s, self.h, self.rng
        live = sorted(self.var)
        for i in rng.choice(live, 3, replace=False):  # penalty updates
            if h["heap_type"][i] == D.HEAP_LATENCY:
                continue
            p = float(rng.random() + 0.25)
            s.update_variable_penalty(self.var[int(i)], p)
            h["penalty"][i] = p
            self.touch(i, "penalty")
        self.retire(int(rng.choice(live)))  # an action ends: its variable leaves, its entry becomes vacant
        i, self.next_free = self.next_free, self.next_free + 1  # an action starts in a reserved entry
        v = s.variable_new(None, 1.0, -1.0, 2)
        s.expand(self.cs[step], v, 1.0)
        s.expand(self.cs[step + 20], v, 0.5)
        self.var[i] = v
        h["var_slot"][i], h["remains"][i], h["penalty"][i] = v.h, 10.0 + step, 1.0
        h["sharing_penalty"][i], h["max_duration"][i] = 1.0, (-1.0 if step % 2 else 50.0)
        if self.lazy:
            h["last_update"][i] = h["start_time"][i] = self.now
        self.touch(i, *FIELDS)
        c = self.cs[step + 40]
        s.update_constraint_bound(c, c.get_bound() * 0.5)

    # ---- the device passes ----
    def _finish(self, ids, evs):
        for i, ev in zip(ids.tolist(), evs.tolist()):
            if ev & D.EV_LATENCY_PAID and i in self.var:  # the variable gets its penalty (network_cm02.cpp:112-116)
                self.s.update_variable_penalty(self.var[i], float(self.h["sharing_penalty"][i]))
            if ev & D.EV_FINISHED and i in self.var:
                self.retire(i)

    def _table(self):
        """The per-call way: a new table from the host records; the resident way: patch what the script changed."""
        h = self.h
        if not self.bound:
            vi = dense_of(self.s.device_touched_vars(), h["var_slot"])
            self.acts = D.DeviceActions(self.s.device_ctx(), vi, **{k: h[k] for k in FULL_UPLOAD})
            if self.lazy:
                self.acts.lazy_init(**{k: h[k] for k in LAZY_UPLOAD})
            self.dirty = {}
            return vi
        if self.acts is None:
            self.acts = D.DeviceActions(self.s.device_ctx(), np.full(self.cap, -1, np.int32),
                                        **{k: h[k] for k in FULL_UPLOAD})
            if self.lazy:
                self.acts.lazy_init(**{k: h[k] for k in LAZY_UPLOAD})
            self.acts.bind(h["var_slot"])
        else:
            groups = {}
            for i, fs in self.dirty.items():
                fs = fs if self.lazy else fs - set(LAZY_UPLOAD)
                groups.setdefault(tuple(sorted(fs)), []).append(i)
            for fs, idx in groups.items():
                self.acts.patch(idx, **{k: h[k][idx] for k in fs})
        self.dirty = {}
        return self.acts.var_index()

    def _download(self):
        st = self.acts.state()
        for k in STATE_FIELDS:
            self.h[k][:] = st[k]
        out = dict(st)
        if self.lazy:
            lz = self.acts.lazy_state()
            for k in LAZY_FIELDS:
                self.h[k][:] = lz[k]
            out.update(lz)
        return out

    def lazy_step(self, step):
        """One Lazy step; returns everything the two ways must agree on."""
        self.script(step)
        self.s.solve()
        vi = self._table()
        extra = [i for i in self.extra if self.h["penalty"][i] > 0]
        modified = [i for i in range(self.cap) if vi[i] >= 0] + [i for i in extra if vi[i] < 0]
        bad = undated(self.h, vi, self.s.device_values(), modified)
        assert not bad, bad  # the reference would die here (Model.cpp:96): a fault of the test's script
        if self.bound:
            nmod, nfin = self.acts.lazy_update_solved(self.model, self.now, extra, 1e-5, 1e-5)
            assert nmod == len(modified)
        else:
            nfin = self.acts.lazy_update(self.model, self.now, modified, 1e-5, 1e-5)
        after_update = self._download()
        ev = self.acts.next_occuring_event_lazy(self.now)
        self.now = self.now + ev if ev >= 0 else self.now + 1.0
        ids, evs = self.acts.lazy_due(self.model, self.now, 1e-5)
        after_due = self._download()
        self._finish(ids, evs)
        return dict(vi=vi, nfin=nfin, ev=ev, ids=ids, evs=evs, after_update=after_update, after_due=after_due)

    def full_step(self, step):
        self.script(step)
        self.s.solve()
        vi = self._table()
        ev = self.acts.next_occuring_event(with_latency=self.model != D.MODEL_CPU)
        delta = ev if ev > 0 else 0.01
        nev = self.acts.update_actions_state(self.model, delta, 1e-5, 1e-5)
        st = self._download()
        ids = np.nonzero(st["events"])[0].astype(np.int32)
        evs = st["events"][ids]
        if self.bound:
            got = self.acts.events()
            assert same_bytes(got[0], ids) and same_bytes(got[1], evs)
        self.now += delta
        self._finish(ids, evs)
        return dict(vi=vi, ev=ev, nev=nev, state=st)


def assert_same(a, b, where):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], dict):
            assert_same(a[k], b[k], where + (k,))
        elif isinstance(a[k], np.ndarray):
            assert same_bytes(a[k], b[k]), where + (k,)
        else:
            assert np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes(), where + (k, a[k], b[k])


# ---- scenario backends over one resident table per model ----
CAP = 4  # entries per model: the scenarios never run more actions at once, and ended ones are reused


class _Table:
    def __init__(self, ctx, lazy):
        self.lazy = lazy
        self.fields = [k for k in FIELDS if lazy or k not in LAZY_UPLOAD]
        self.acts = D.DeviceActions.reserve(ctx, CAP, lazy=lazy)
        self.shadow = {k: v for k, v in vacant_table(CAP).items() if k in self.fields}
        self.slot_of = {}   # id(action) -> table index
        self.action = {}    # table index -> action
        self.patched = 0


class ResidentBackend(SC.DeviceBackend):
    """simgrid_amd.lmm.System (resident, selective update) + ONE DeviceActions table per model, bound to the
    variables' host slots: no re-upload, no dense_index, no host modified list but the hand-pushed actions."""

    def _record(self, model, a):
        """The host record of action `a` (what DeviceBackend._acts uploads), or the vacant one."""
        if a is None or not a.alive:
            return dict(D.VACANT)
        return dict(D.VACANT, var_slot=a.var.h, remains=a.remains, max_duration=a.max_duration,
                    penalty=a.sharing_penalty, sharing_penalty=1.0,
                    flags=0 if a.state == SC.Action.STARTED else D.ACT_NOT_STARTED, last_update=a.last_update,
                    last_value=a.last_value, start_time=a.start_time, date=a.date, heap_type=a.heap_type)

    def _lazy_table(self, model):
        return True

    def _sync(self, model):
        """Patch exactly the entries whose host record differs from the shadow, then check that the device holds
        the host records."""
        t = model.__dict__.get("_tab")
        if t is None:
            t = model._tab = _Table(model.sys.device_ctx(), self._lazy_table(model))
        for a in model.actions:  # a new action takes a vacant entry; an ended one keeps its entry until it is patched
            if a.alive and self._tracked(model, a) and id(a) not in t.slot_of:
                free = [i for i in range(CAP) if i not in t.action or not self._tracked(model, t.action[i])]
                assert free, "action table full"
                old = t.action.pop(free[0], None)
                if old is not None:
                    del t.slot_of[id(old)]
                t.slot_of[id(a)], t.action[free[0]] = free[0], a
        for i in range(CAP):
            a = t.action.get(i)
            rec = self._record(model, a if a is not None and self._tracked(model, a) else None)
            diff = {k: rec[k] for k in t.fields
                    if np.asarray(rec[k], t.shadow[k].dtype).tobytes() != t.shadow[k][i].tobytes()}
            if diff:
                t.acts.patch([i], **diff)
                t.patched += 1
                for k, v in diff.items():
                    t.shadow[k][i] = v
        dev = dict(t.acts.state())
        if t.lazy:
            dev.update(t.acts.lazy_state())
        for k in t.fields:
            if k in dev:
                assert same_bytes(dev[k], t.shadow[k]), (k, dev[k], t.shadow[k])
        return t

    def _tracked(self, model, a):
        return a.alive

    def _back(self, model, t, keys):
        """The device's state into the host actions and the shadow (what DeviceBackend._back does per call)."""
        dev = dict(t.acts.state())
        if t.lazy:
            dev.update(t.acts.lazy_state())
        for k in keys:
            t.shadow[k][:] = dev[k]
        for i, a in t.action.items():
            if self._tracked(model, a):
                for k in keys:
                    setattr(a, k, (int if k == "heap_type" else float)(dev[k][i]))

    LAZY_BACK = ("remains", "max_duration", "last_update", "last_value", "date", "heap_type")

    def solve(self, model):
        model._solved = bool(model.sys.modified)  # lmm_solve flattens and solves only then (maxmin.cpp:487-489)
        model.sys.lmm_solve()
        model.sys.clear_modified_actions()
        return []  # the modified set is taken on the device; Model adds the hand-pushed actions

    def lazy_update(self, model, mod, now):
        t = self._sync(model)
        extra = [t.slot_of[id(a)] for a in mod]
        if model._solved:
            t.acts.lazy_update_solved(model.kind, now, extra, SC.MAXMIN_PREC, SC.SURF_PREC)
            ids, evs = t.acts.events()
        else:  # no solve, no modified set but the hand-pushed actions
            t.acts.lazy_update(model.kind, now, extra, SC.MAXMIN_PREC, SC.SURF_PREC)
            ids, evs = t.acts.events()
            keep = np.isin(ids, extra)
            ids, evs = ids[keep], evs[keep]
        self._back(model, t, self.LAZY_BACK)
        return [t.action[int(i)] for i, e in zip(ids, evs) if e & 1]

    def lazy_due(self, model, now):
        t = self._sync(model)
        top = t.acts.next_occuring_event_lazy(now)
        if top < 0 or not abs(top) < SC.SURF_PREC:
            return []
        ids, evs = t.acts.lazy_due(model.kind, now, SC.SURF_PREC)
        self._back(model, t, self.LAZY_BACK)
        return [(t.action[int(i)], int(e)) for i, e in zip(ids, evs)]


class ResidentPing(ResidentBackend, PP.PingDevice):
    """PingDevice over the resident table: Lazy as ResidentBackend, Full through act_next_event / act_update on a
    table that holds the started actions."""

    def _lazy_table(self, model):
        return not isinstance(model, PP.FullModel)

    def _tracked(self, model, a):
        return a.alive and (self._lazy_table(model) or a.state == SC.Action.STARTED)

    def _record(self, model, a):
        if self._lazy_table(model) or a is None:
            return super()._record(model, a)
        return dict(D.VACANT, var_slot=a.var.h, remains=a.remains, max_duration=a.max_duration, latency=a.latency,
                    penalty=a.var.get_penalty(), sharing_penalty=a.sharing_penalty,
                    flags=0 if a.var.get_number_of_constraint() else D.ACT_NO_CNST)

    def full_next(self, model):
        if model.sys.modified:
            model.sys.solve()
        t = self._sync(model)
        return t.acts.next_occuring_event(with_latency=True)

    def full_update(self, model, delta):
        t = self._sync(model)
        t.acts.update_actions_state(D.MODEL_CM02, delta, SC.MAXMIN_PREC, SC.SURF_PREC)
        ids, evs = t.acts.events()
        self._back(model, t, ("remains", "max_duration", "latency"))
        t.shadow["penalty"][:] = t.acts.state()["penalty"]  # (act_update restores it when the latency is paid)
        return [(t.action[int(i)], int(e)) for i, e in zip(ids, evs)]
