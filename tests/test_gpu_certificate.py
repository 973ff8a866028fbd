"""The max-min certificate and the bottleneck witnesses computed on the device (cert_cnst / cert_var:
lmmhip_certificate, lmm_device_certificate, lmm_device_bottlenecks, DeviceBatch.certificate).

The yardstick is `model` below: a NumPy restatement of the pass over what the device itself holds — the flattened
system (lmmhip_flat_download), the values (lmmhip_get_values) and the usages (lmmhip_get_usage, whose bytes cert_cnst
reuses).  The level x * pen is one rounded fp64 product, a maximum has no rounding of its own, and the predicates of
lmm_cert.hpp are fixed expressions of single fp64 operations (the device code is compiled with -ffp-contract=off), so
the struct and the witness array have to EQUAL the model: max_excess by its bytes, the counts and the witnesses by
value.

Two statements of the detection cases are meant as follows (reasoning, not measurement):
  * halved bounds: a judged constraint that was saturated has U >= b (1 - prec), so U - b/2 >= b/2 - b prec > (b/2) prec
    for prec < 1/3: every formerly saturated judged constraint is infeasible.  An unsaturated one with U above half its
    bound is infeasible too, so n_infeasible is AT LEAST the number of formerly saturated judged constraints (asserted,
    with > 0), not always equal to it;
  * doubled bounds: no constraint is saturated any more (2b - U >= b (1 - prec) > 2 b prec), so no variable has a
    constraint for a witness; a variable at its own bound stays at it.  Hence n_unbottlenecked == n_judged_var -
    n_at_bound and every witness is negative: -2 for every judged variable that is not at its bound.
"""
import ctypes as ct
import struct

import numpy as np
import pytest

from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
STRESS = dict(penalty_mix=1, bounded_permille=100, fatpipe_permille=50)
FB = L.System.FAIR_BOTTLENECK
COUNTS = ("n_infeasible", "n_unbottlenecked", "n_judged_cnst", "n_judged_var", "n_at_bound")


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if L.device_count() == 0:
        pytest.fail("no HIP device visible: the GPU tests must run on the MI355X")


def p(a, t):
    return a.ctypes.data_as(ct.POINTER(t))


def ctx_flat(ctx):
    """The flattened system a device context holds (lmmhip_flat_download), as System.device_flat() returns it."""
    n = (L.I64 * 3)()
    L._check_hip(L.lib().lmmhip_flat_download(ctx, n, *([None] * 10)))
    nV, nC, nnz = n
    a = dict(var_ptr=np.zeros(nV + 1, np.uint32), csr_c=np.zeros(nnz, np.int32), csr_w=np.zeros(nnz),
             cnst_ptr=np.zeros(nC + 1, np.uint32), csc_v=np.zeros(nnz, np.int32), csc_w=np.zeros(nnz),
             pen=np.zeros(nV), vbound=np.zeros(nV), cbound=np.zeros(nC), cflags=np.zeros(nC, np.uint8))
    L._check_hip(L.lib().lmmhip_flat_download(ctx, n, *(x.ctypes.data for x in a.values())))
    return a


def ctx_values(ctx, n):
    x = np.empty(n, np.float64)
    L._check_hip(L.lib().lmmhip_get_values(ctx, p(x, ct.c_double)))
    return x


def ctx_usage(ctx, n):
    u = np.empty(n, np.float64)
    L._check_hip(L.lib().lmmhip_get_usage(ctx, p(u, ct.c_double)))
    return u


def model(f, x, u, prec, fair=False):
    """(lmmhip_cert as a dict, witness array) of the flattened system `f` under the values `x` and usages `u`."""
    nV, nC = len(x), len(u)
    cptr, vptr = f["cnst_ptr"].astype(np.int64), f["var_ptr"].astype(np.int64)
    pen, vb, b = f["pen"], f["vbound"], f["cbound"]
    with np.errstate(all="ignore"):
        # constraint half: top_c = max over the CSC segment of x * pen (0 for an empty one; a NaN level is skipped)
        top = np.zeros(nC)
        full = cptr[1:] > cptr[:-1]
        if full.any():
            lev = x[f["csc_v"]] * pen[f["csc_v"]]
            top[full] = np.fmax(0.0, np.fmax.reduceat(lev, cptr[:-1][full]))
        judged = b > b * prec
        infeasible = judged & (u - b > b * prec)
        sat = judged & ~(b - u > b * prec)
        ex = ((u - b) / b)[judged]
        worst = float(np.fmax.reduce(ex, initial=-1e300)) if len(ex) else -1e300
        cert = dict(max_excess=worst, n_infeasible=int(infeasible.sum()), n_unbottlenecked=-1,
                    n_judged_cnst=int(judged.sum()), n_judged_var=0, n_at_bound=0)
        wit = np.full(nV, L.WIT_NOT_JUDGED, np.int32)
        if fair:
            return cert, wit
        sattop = np.where(sat, top, np.inf)
        # variable half
        jv = (pen > 0) & (x > 0)
        tol = np.where(prec < 1e-9 * vb, 1e-9 * vb, prec)
        atb = jv & (vb > 0) & (np.abs(x - vb) <= tol)
        level = x * pen
        row = np.repeat(np.arange(nV), np.diff(vptr))
        carries = level[row] >= sattop[f["csr_c"]] * (1 - 1e-9)
        pos = np.flatnonzero(carries)  # ascending: np.unique's index is each row's first carrier in row order
        rows, first = np.unique(row[pos], return_index=True)
        wit[:] = L.WIT_NONE
        wit[rows] = f["csr_c"][pos[first]]
        wit[atb] = L.WIT_AT_BOUND
        wit[~jv] = L.WIT_NOT_JUDGED
    cert.update(n_unbottlenecked=int((wit == L.WIT_NONE).sum()), n_judged_var=int(jv.sum()), n_at_bound=int(atb.sum()))
    return cert, wit


def assert_equal(got, want, what=""):
    """The struct (max_excess by its bytes) and the witness array of `got` equal the model's `want`."""
    (gc, gw), (wc, ww) = got, want
    print(f"{what}: device {gc}")
    assert struct.pack("d", gc["max_excess"]) == struct.pack("d", wc["max_excess"]), (what, gc, wc)
    assert {k: gc[k] for k in COUNTS} == {k: wc[k] for k in COUNTS}, (what, gc, wc)
    assert gw.dtype == np.int32 and len(gw) == len(ww)
    bad = np.flatnonzero(gw != ww)
    assert len(bad) == 0, (what, len(bad), bad[:8], gw[bad[:8]], ww[bad[:8]])


def sys_model(s, prec=None):
    return model(s.device_flat(), s.device_values(), s.device_usage_dense(), L.get_precision() if prec is None else prec,
                 fair=s_kind(s) == FB)


def s_kind(s):
    return FB if s.last_engine() in (L.System.RAN_FB_ROUNDS, L.System.RAN_FB_BATCH) else L.System.MAXMIN


def cert_bytes(got):
    c, w = got
    return struct.pack("d5q", c["max_excess"], *(c[k] for k in COUNTS)) + w.tobytes()


# ---- 1: wave-stride and row-length edges, on the three global engines ----------------------------------------

DEGREES = (1, 2, 63, 64, 65, 128, 129, 1000)
ENGINES = {"persistent": (L.System.ENGINE_PERSISTENT, L.System.RAN_PERSISTENT),
           "rounds": (L.System.ENGINE_ROUNDS, L.System.RAN_ROUNDS),
           "frontier": (L.System.ENGINE_FRONTIER, L.System.RAN_FRONTIER)}


def build_a():
    """1000 variables, 16 constraints of degrees DEGREES, once SHARED and once FATPIPE; variable i lies on constraint
    k iff i < deg_k (rows of 2 .. 16 elements, around cert_var's lane / wave threshold of 8)."""
    rng = np.random.default_rng(20251)
    s = L.System(False)
    cs = []
    for fat in (False, True):
        for deg in DEGREES:
            c = s.constraint_new(None, float(rng.uniform(5.0, 50.0)) * (1 if deg < 100 else 10))
            if fat:
                c.unshare()
            cs.append((c, deg))
    for i in range(1000):
        pen = float(rng.choice([0.5, 1.0, 2.0]))
        bound = float(rng.uniform(0.001, 0.05)) if i % 10 == 0 else -1.0
        v = s.variable_new(None, pen, bound, len(cs))
        for c, deg in cs:
            if i < deg:
                s.expand(c, v, float(rng.uniform(0.1, 10.0)))
    return s


def build_rows(lengths, n_cnst, seed, vbound_hi=0.05):
    """n_cnst constraints (every 7th FATPIPE) and one variable per entry of `lengths`, on that many distinct
    constraints; a tenth of the variables bounded, below vbound_hi."""
    rng = np.random.default_rng(seed)
    s = L.System(False)
    cs = [s.constraint_new(None, float(rng.uniform(5.0, 50.0))) for _ in range(n_cnst)]
    for k in range(0, n_cnst, 7):
        cs[k].unshare()
    for i, n in enumerate(lengths):
        bound = float(rng.uniform(0.001, vbound_hi)) if i % 10 == 0 else -1.0
        v = s.variable_new(None, float(rng.choice([0.5, 1.0, 2.0])), bound, n)
        for k in rng.choice(n_cnst, n, replace=False):
            s.expand(cs[int(k)], v, float(rng.uniform(0.1, 10.0)))
    return s


B_ROWS = (1, 2, 63, 64, 65, 129, 300)
# (the row lengths around cert_var's own thresholds: a lane scans up to 8 elements, the wave 64 per step)
C_ROWS = (7, 8, 9, 16, 17)
BUILDERS = {
    "A": (build_a, 1000, (2, 4, 6, 8, 10, 12, 14, 16)),
    "B": (lambda: build_rows([n for n in B_ROWS for _ in range(2)] + [3] * 200, 300, 4242), 214, B_ROWS + (3,)),
    "C": (lambda: build_rows([n for n in C_ROWS for _ in range(6)], 40, 99, vbound_hi=0.002), 30, C_ROWS),
}


class Edges:
    def __init__(self, system, engine):
        want, ran = ENGINES[engine]
        build, self.n_var, self.rows = BUILDERS[system]
        self.s = s = build()
        s.set_engine(want)
        s.prepare()
        s.device_solve()
        # (a persistent launch that could not become co-resident is re-run by the round engine and says so)
        assert s.last_engine() == ran or (engine == "persistent" and s.engine_fallbacks() > 0)
        self.got = s.device_certificate_dense()


@pytest.fixture(scope="module", params=[(b, e) for b in BUILDERS for e in ENGINES], ids=lambda t: "-".join(t))
def edges(request):
    return Edges(*request.param)


def test_edges_equal_the_model_and_certify(edges):
    s = edges.s
    f = s.device_flat()
    assert len(f["pen"]) == edges.n_var
    assert set(np.diff(f["var_ptr"].astype(np.int64)).tolist()) == set(edges.rows)
    assert_equal(edges.got, sys_model(s), "edges")
    cert, wit = edges.got
    assert cert["n_infeasible"] == 0 and cert["n_unbottlenecked"] == 0 and cert["n_at_bound"] > 0
    assert cert["n_judged_var"] > 0.9 * edges.n_var and cert["n_judged_cnst"] == len(f["cbound"])
    assert np.count_nonzero(wit >= 0) + cert["n_at_bound"] == cert["n_judged_var"]
    assert s.device_certificate() == (cert["max_excess"], 0, 0)
    # counts only (no witness buffer), and a second call: the same bytes
    c2, none = L.ctx_certificate(s.device_ctx(), edges.n_var, L.get_precision(), witness=False)
    assert none is None and c2 == cert
    assert cert_bytes(s.device_certificate_dense()) == cert_bytes(edges.got)


# ---- 2: every engine class -----------------------------------------------------------------------------------

def stress_member(seed, kind=L.System.MAXMIN):
    s = L.System(False, kind)
    s.gen_synthetic(100, 600, 8, seed, **STRESS)
    return s


@pytest.mark.parametrize("kind,ran", [(M.DeviceBatch.MAXMIN, L.System.RAN_BATCH),
                                      (M.DeviceBatch.FAIR_BOTTLENECK, L.System.RAN_FB_BATCH)])
def test_batch_engines(kind, ran):
    b = M.DeviceBatch([stress_member(seed, kind) for seed in range(1, 9)], kind=kind)
    try:
        b.solve()
        assert b.last_engine() == ran
        got = b.certificate()
        fair = kind == M.DeviceBatch.FAIR_BOTTLENECK
        want = model(ctx_flat(b.ctx), b.values(), b.usage(), b.prec, fair=fair)
        assert_equal(got, want, "batch")
        cert, wit = got
        assert len(wit) == b.n_var > 4000 and cert["n_judged_cnst"] > 700
        if fair:
            assert cert["n_unbottlenecked"] == -1 and cert["n_judged_var"] == 0 and cert["n_at_bound"] == 0
            assert (wit == L.WIT_NOT_JUDGED).all()
        else:
            assert cert["n_infeasible"] == 0 and cert["n_unbottlenecked"] == 0 and cert["n_at_bound"] > 0
        assert cert_bytes(b.certificate()) == cert_bytes(got)
    finally:
        b.close()


def test_fair_bottleneck_round_engine():
    s = stress_member(1, FB)
    s.prepare()
    s.device_solve()
    assert s.last_engine() == L.System.RAN_FB_ROUNDS
    got = s.device_certificate_dense()
    assert_equal(got, sys_model(s), "FairBottleneck")
    cert, wit = got
    assert cert["n_unbottlenecked"] == -1 and cert["n_judged_var"] == 0 and cert["n_at_bound"] == 0
    assert cert["n_judged_cnst"] > 80 and (wit == L.WIT_NOT_JUDGED).all()
    assert s.device_certificate()[2] == -1
    vs, cs = s.device_bottlenecks()
    assert len(vs) == len(wit) and (cs == L.WIT_NOT_JUDGED).all()


# ---- 3: detection: the pass reads what HBM holds now ---------------------------------------------------------

def solved_a():
    s = build_a()
    s.prepare()
    s.device_solve()
    return s


def solved_r8s():
    s, _, _ = K.replay(L, K.engine_script("R8S", 0))
    s.prepare()
    s.device_solve()
    return s


@pytest.mark.parametrize("build", [solved_a, solved_r8s], ids=["A", "R8S"])
def test_detection(build):
    s = build()
    lib, ctx, prec = L.lib(), s.device_ctx(), L.get_precision()
    f0 = s.device_flat()
    x, u = s.device_values(), s.device_usage_dense()
    nV = len(x)
    cert0 = L.ctx_certificate(ctx, nV, prec)
    assert_equal(cert0, model(f0, x, u, prec), "solved")
    assert cert0[0]["n_infeasible"] == 0 and cert0[0]["n_unbottlenecked"] == 0
    b0, pen0 = f0["cbound"].copy(), f0["pen"].copy()
    sat0 = (b0 > b0 * prec) & ~(b0 - u > b0 * prec)

    def now(what):
        got = L.ctx_certificate(ctx, nV, prec)
        assert s.device_values().tobytes() == x.tobytes()  # nothing was solved again
        assert_equal(got, model(s.device_flat(), x, s.device_usage_dense(), prec), what)
        return got

    # halved bounds: every formerly saturated judged constraint is infeasible (module docstring)
    L._check_hip(lib.lmmhip_update_cnsts(ctx, p(np.ascontiguousarray(0.5 * b0), ct.c_double)))
    cert, _ = now("halved bounds")
    print(f"halved: {cert['n_infeasible']} infeasible, {int(sat0.sum())} formerly saturated (U > 0: "
          f"{int((sat0 & (u > 0)).sum())})")
    assert cert["n_infeasible"] >= int(sat0.sum()) > 0
    # doubled bounds: nothing is saturated, no variable has a constraint for a witness
    L._check_hip(lib.lmmhip_update_cnsts(ctx, p(np.ascontiguousarray(2.0 * b0), ct.c_double)))
    cert, wit = now("doubled bounds")
    assert cert["n_infeasible"] == 0 and cert["n_judged_var"] > cert["n_at_bound"]
    assert cert["n_unbottlenecked"] == cert["n_judged_var"] - cert["n_at_bound"]
    assert (wit < 0).all() and np.count_nonzero(wit == L.WIT_NONE) == cert["n_unbottlenecked"]
    assert cert["n_at_bound"] == cert0[0]["n_at_bound"]
    # the bounds back, every other penalty times 4: those variables' levels pass their constraints' tops ... and the
    # others no longer reach them
    L._check_hip(lib.lmmhip_update_cnsts(ctx, p(b0, ct.c_double)))
    pen = pen0.copy()
    pen[::2] *= 4.0
    L._check_hip(lib.lmmhip_update_vars(ctx, p(pen, ct.c_double), None))
    cert, _ = now("penalties")
    assert cert["n_infeasible"] == 0 and cert["n_unbottlenecked"] > 0
    # everything back: the original bytes
    L._check_hip(lib.lmmhip_update_vars(ctx, p(pen0, ct.c_double), None))
    assert cert_bytes(now("restored")) == cert_bytes(cert0)


# ---- 4: scripts through the System interface, resident and not, with no fetch --------------------------------

SCRIPTS = [("random", i) for i in range(20)] + [(shape, seed) for shape in ("R4", "R8", "R16", "R32", "R64", "WIDE", "R8S")
                                                for seed in K.ENGINE_SHAPES[shape][2]]


def script_ops(name, i):
    if name == "random":
        return K.random_script(i, conc_limits=(i % 2 == 0), frees=3, penalty_updates=4, bound_updates=4)
    return K.engine_script(name, i)


@pytest.mark.parametrize("resident", [True, False], ids=["resident", "host"])
@pytest.mark.parametrize("name,i", SCRIPTS, ids=[f"{n}{i}" for n, i in SCRIPTS])
def test_scripts_without_fetch(name, i, resident):
    s, cs, vs = K.replay(L, script_ops(name, i))
    s.set_resident(resident)
    s.prepare()
    s.device_solve()
    ex, ni, nu = s.device_certificate()  # no fetch
    assert (ni, nu) == (0, 0), (ex, ni, nu)
    got = s.device_certificate_dense()
    f, u = s.device_flat(), s.device_usage_dense()
    assert_equal(got, model(f, s.device_values(), u, L.get_precision()), f"{name} {i}")
    cert, wit = got
    assert cert["max_excess"] == ex and cert["n_judged_var"] > 0
    # the witnesses in host ids
    vids, cids = s.device_bottlenecks()
    dense_cids, _ = s.device_usage()  # (dense constraint -> id)
    assert len(vids) == len(wit) == s.last_stats()["n_var"] and len(set(vids.tolist())) == len(vids)
    assert set(vids.tolist()) <= {v.h for v in vs.values()}
    assert (cids[wit < 0] == wit[wit < 0]).all()
    assert (cids[wit >= 0] == dense_cids[wit[wit >= 0]]).all()
    vptr = f["var_ptr"].astype(np.int64)
    for d in np.flatnonzero(wit >= 0).tolist():
        assert wit[d] in f["csr_c"][vptr[d]:vptr[d + 1]], (d, wit[d])
    # after the fetch: the host walk's counts, and its worst excess within the usage sums' reordering bound
    s.fetch()
    hex_, hni, hnu = s.check_certificate()
    assert (hni, hnu) == (ni, nu)
    b = f["cbound"]
    jd = b > b * L.get_precision()
    n_max = int(np.diff(f["cnst_ptr"].astype(np.int64)).max())
    tol = 2 * n_max * EPS * float((u[jd] / b[jd]).max())
    print(f"max_excess device {ex!r} host {hex_!r} tolerance {tol:.3e}")
    assert abs(hex_ - ex) <= tol, (hex_, ex, tol)
    assert set(cids[cids >= 0].tolist()) <= set(s.flat_cnst_ids().tolist())


# ---- 5: selective, resident and not --------------------------------------------------------------------------

def build_halves(resident):
    """A selective system of two disconnected halves, each 20 constraints x 60 variables with 3 elements each."""
    rng = np.random.default_rng(777)
    s = L.System(True)
    s.set_resident(resident)
    halves = []
    for _ in range(2):
        cs = [s.constraint_new(None, float(rng.uniform(1.0, 20.0))) for _ in range(20)]
        cs[3].unshare()
        vs = []
        for j in range(60):
            v = s.variable_new(None, float(rng.choice([0.5, 1.0, 2.0])), 0.05 if j % 10 == 0 else -1.0, 3)
            for k in rng.choice(20, 3, replace=False):
                s.expand(cs[int(k)], v, float(rng.uniform(0.1, 2.0)))
            vs.append(v)
        halves.append((cs, vs))
    return s, halves


def selective_bottlenecks(resident):
    s, ((cs1, vs1), _) = build_halves(resident)
    assert s.resident() == resident
    s.solve()
    assert s.last_stats()["n_cnst"] == 40
    s.update_constraint_bound(cs1[5], 0.5 * cs1[5].get_bound())
    s.prepare()
    s.device_solve()
    assert s.device_certificate()[1:] == (0, 0)
    got = s.device_certificate_dense()
    assert_equal(got, sys_model(s), "selective")
    vids, cids = s.device_bottlenecks()
    assert 0 < len(vids) <= 60 and set(vids.tolist()) <= {v.h for v in vs1}
    assert (cids >= 0).any() and set(cids[cids >= 0].tolist()) <= {c.h for c in cs1}
    return vids, cids, got


def test_selective_resident_and_not():
    v_r, c_r, got_r = selective_bottlenecks(True)
    v_h, c_h, got_h = selective_bottlenecks(False)
    assert v_r.tobytes() == v_h.tobytes() and c_r.tobytes() == c_h.tobytes()
    assert cert_bytes(got_r) == cert_bytes(got_h)


# ---- 6: past the grid cap, many workgroups' parts folded -----------------------------------------------------

def test_past_the_grid_cap():
    """600,000 rows against 2048 workgroups of 256 threads, 20,000 constraints against 2048 x 4 waves."""
    s = L.System(False)
    s.gen_synthetic(20000, 600000, 3, 7, want_vars=False, **STRESS)
    s.prepare()
    s.device_solve()
    prec, ctx = L.get_precision(), s.device_ctx()
    f, x, u = s.device_flat(), s.device_values(), s.device_usage_dense()
    assert len(x) == 600000 and len(u) == 20000
    got = s.device_certificate_dense()
    assert_equal(got, model(f, x, u, prec), "solved")
    assert got[0]["n_infeasible"] == 0 and got[0]["n_unbottlenecked"] == 0 and got[0]["n_at_bound"] > 0
    assert cert_bytes(s.device_certificate_dense()) == cert_bytes(got)
    L._check_hip(L.lib().lmmhip_update_cnsts(ctx, p(np.ascontiguousarray(0.5 * f["cbound"]), ct.c_double)))
    half = s.device_certificate_dense()
    assert_equal(half, model(s.device_flat(), x, s.device_usage_dense(), prec), "halved bounds")
    assert half[0]["n_infeasible"] >= 1000
    assert cert_bytes(s.device_certificate_dense()) == cert_bytes(half)


# ---- 7: raw ABI edges ----------------------------------------------------------------------------------------

def test_raw_abi_edges():
    import torch

    lib, prec = L.lib(), L.get_precision()
    # v0 on c0 (4) and c1 (3, FATPIPE), v1 on c0; c2 (5) has no element
    var_ptr, cnst_idx = np.array([0, 2, 3], np.int64), np.array([0, 1, 0], np.int32)
    weight, pen, vbound = np.array([1.0, 2.0, 3.0]), np.ones(2), -np.ones(2)
    cbound, cflags = np.array([4.0, 3.0, 5.0]), np.array([0, 1, 0], np.uint8)
    ctx = ct.c_void_p()
    cert, wit = L.LmmhipCert(), np.full(2, 77, np.int32)
    L._check_hip(lib.lmmhip_ctx_create(torch.cuda.current_device(), ct.byref(ctx)))
    try:
        assert lib.lmmhip_certificate(ctx, prec, ct.byref(cert), p(wit, ct.c_int32)) == -4  # nothing uploaded
        L._check_hip(lib.lmmhip_upload(ctx, 2, 3, 3, p(var_ptr, ct.c_int64), p(cnst_idx, ct.c_int32),
                                       p(weight, ct.c_double), p(pen, ct.c_double), p(vbound, ct.c_double),
                                       p(cbound, ct.c_double), p(cflags, ct.c_uint8)))
        assert lib.lmmhip_certificate(ctx, prec, ct.byref(cert), p(wit, ct.c_int32)) == -4  # uploaded, not solved
        assert wit.tolist() == [77, 77]
        L._check_hip(lib.lmmhip_solve(ctx, 0, prec))
        assert lib.lmmhip_certificate(ctx, prec, None, p(wit, ct.c_int32)) == -3  # LMMHIP_E_ARG
        L._check_hip(lib.lmmhip_certificate(ctx, prec, ct.byref(cert), None))  # no witness buffer
        first = cert.as_dict()
        got = L.ctx_certificate(ctx, 2, prec)
        assert got[0] == first
        x, u = ctx_values(ctx, 2), ctx_usage(ctx, 3)
        assert_equal(got, model(ctx_flat(ctx), x, u, prec), "three constraints")
        # the empty constraint is judged, not infeasible, and not saturated: its excess is -1, it is no witness
        sat = np.empty(3, np.uint8)
        L._check_hip(lib.lmmhip_get_saturated(ctx, p(sat, ct.c_uint8)))
        assert first["n_judged_cnst"] == 3 and first["n_infeasible"] == 0 and u[2] == 0.0 and not sat[2]
        assert first["n_unbottlenecked"] == 0 and first["n_judged_var"] == 2 and first["n_at_bound"] == 0
        assert got[1].tolist() == [0, 0] and sat[0]
        # a zero bound is not judged: c0 leaves the count, and the variables lose their witness
        L._check_hip(lib.lmmhip_update_cnsts(ctx, p(np.array([0.0, 3.0, 5.0]), ct.c_double)))
        zero = L.ctx_certificate(ctx, 2, prec)
        assert_equal(zero, model(ctx_flat(ctx), x, u, prec), "zero bound")
        assert zero[0]["n_judged_cnst"] == 2 and zero[0]["n_infeasible"] == 0
    finally:
        lib.lmmhip_ctx_destroy(ctx)
