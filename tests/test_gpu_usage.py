"""Constraint usage computed on the device (mm_usage: lmmhip_get_usage, lmmhip_usage_device_ptr, lmm_device_usage).

U_c = Constraint::get_usage() (maxmin.cpp:948-961) of every constraint of the solved system, from the values the
device holds: the sum (FATPIPE: the max) of w * x over the constraint's flattened CSC segment.  Bounds used below:
  * FATPIPE: U_c == max(w * x) in float64, bit for bit (a maximum has no rounding of its own);
  * SHARED:  |U_c - fsum(w * x)| <= n_c * 2^-52 * fsum(w * x), n_c = the segment's length: the forward error of an
    fp64 sum of n_c non-negative rounded products in any order ((n_c - 1) u with u = 2^-53, first order), with a
    factor 2.  n_c = 1 gives equality;
  * against the oracle: sum_e w_e * max(ABS_TOL, REL_TOL * |x_e|) + n_c * 2^-52 * U, the project's value tolerance
    (tests/lmm_cases.py) carried through the sum, x_e and U the oracle's.
"""
import ctypes as ct
import math

import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -52
STRESS = dict(penalty_mix=1, bounded_permille=100, fatpipe_permille=50)
FB = L.System.FAIR_BOTTLENECK


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


def check_exact(u, f, x):
    """The bounds of the module docstring for usages `u` of the flattened system `f` (device arrays) under the
    device's values `x`.  Returns (SHARED constraints checked, FATPIPE ones, the largest SHARED error in units of
    2^-52 * fsum)."""
    assert u.dtype == np.float64 and len(u) == len(f["cbound"])
    nsh = nfat = 0
    worst = 0.0
    for d in range(len(u)):
        lo, hi = int(f["cnst_ptr"][d]), int(f["cnst_ptr"][d + 1])
        wx = f["csc_w"][lo:hi] * x[f["csc_v"][lo:hi]]
        if hi == lo:
            assert u[d] == 0.0, d
        elif f["cflags"][d] & 1:
            assert u[d] == wx.max(), (d, hi - lo, u[d], wx.max())
            nfat += 1
        else:
            ref = math.fsum(wx.tolist())
            err = abs(u[d] - ref)
            assert err <= (hi - lo) * EPS * ref, (d, hi - lo, u[d], ref, err)
            if ref > 0:
                worst = max(worst, err / (EPS * ref))
            nsh += 1
    return nsh, nfat, worst


# ---- 1-3: the wave-stride edges, on the three global engines -------------------------------------------------

DEGREES = (1, 2, 63, 64, 65, 128, 129, 1000)
ENGINES = {"persistent": (L.System.ENGINE_PERSISTENT, L.System.RAN_PERSISTENT),
           "rounds": (L.System.ENGINE_ROUNDS, L.System.RAN_ROUNDS),
           "frontier": (L.System.ENGINE_FRONTIER, L.System.RAN_FRONTIER)}


def build_edges():
    """1000 variables, 16 constraints of degrees DEGREES, once SHARED and once FATPIPE; variable i lies on constraint
    k iff i < deg_k: one lane, a full wave, one element into the second stride, several strides."""
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


class Edges:
    def __init__(self, engine):
        want, ran = ENGINES[engine]
        self.s = s = build_edges()
        s.set_engine(want)
        s.prepare()
        s.device_solve()
        # (a persistent launch that could not become co-resident is re-run by the round engine and says so)
        assert s.last_engine() == ran or (engine == "persistent" and s.engine_fallbacks() > 0)
        self.f = s.device_flat()
        self.x = s.device_values()
        self.u = s.device_usage_dense()


@pytest.fixture(scope="module", params=list(ENGINES))
def edges(request):
    return Edges(request.param)


def test_exact_against_device_values(edges):
    f, x, u = edges.f, edges.x, edges.u
    deg = np.diff(f["cnst_ptr"].astype(np.int64))
    assert sorted(deg.tolist()) == sorted(DEGREES * 2) and len(x) == 1000
    assert sorted(deg[(f["cflags"] & 1) == 1].tolist()) == sorted(DEGREES)
    assert np.count_nonzero(x > 0) > 900 and np.count_nonzero((f["vbound"] > 0) & (x == f["vbound"])) > 0
    nsh, nfat, worst = check_exact(u, f, x)
    print(f"SHARED {nsh}, FATPIPE {nfat}, largest SHARED error {worst:.3f} x 2^-52 fsum")
    assert (nsh, nfat) == (8, 8)


def test_consistent_with_saturated_set(edges):
    prec = L.get_precision()
    b = edges.f["cbound"]
    sat = edges.s.device_saturated()
    np.testing.assert_array_equal(sat, ~((b - edges.u) > b * prec))
    assert 0 < np.count_nonzero(sat) < len(sat)


def test_deterministic(edges):
    s = edges.s
    ref = edges.u.tobytes()
    assert s.device_usage_dense().tobytes() == ref
    assert s.device_usage_dense().tobytes() == ref
    ids, u = s.device_usage()
    assert u.tobytes() == ref and ids.dtype == np.int64
    s.device_solve()  # the same system solved again
    assert s.device_values().tobytes() == edges.x.tobytes()
    assert s.device_usage_dense().tobytes() == ref


# ---- 4: every engine class -----------------------------------------------------------------------------------

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
        u = b.usage()
        assert len(u) == b.n_cnst == 800
        nsh, nfat, worst = check_exact(u, ctx_flat(b.ctx), b.values())
        print(f"SHARED {nsh}, FATPIPE {nfat}, largest SHARED error {worst:.3f} x 2^-52 fsum")
        assert nsh > 700 and nfat > 8
        assert b.usage().tobytes() == u.tobytes()
    finally:
        b.close()


def test_fair_bottleneck_round_engine():
    s = stress_member(1, FB)
    s.prepare()
    s.device_solve()
    assert s.last_engine() == L.System.RAN_FB_ROUNDS
    u = s.device_usage_dense()
    nsh, nfat, worst = check_exact(u, s.device_flat(), s.device_values())
    print(f"SHARED {nsh}, FATPIPE {nfat}, largest SHARED error {worst:.3f} x 2^-52 fsum")
    assert nsh > 80 and nfat > 0
    ids, u2 = s.device_usage()
    assert u2.tobytes() == u.tobytes()
    assert ids.tolist() == s.flat_cnst_ids().tolist()


# ---- 5: against the oracle through the System interface, with no fetch ---------------------------------------

SCRIPT_KW = dict(frees=3, penalty_updates=4, bound_updates=4)


def oracle_tol(oc):
    """(tolerance, n_c) of an oracle constraint's usage: the value tolerance carried through the sum."""
    el = [(w, x) for _, w, x, en in oc.elements() if en and w > 0]
    n = len(el)
    assert n == oc.get_variable_amount()
    return sum(w * max(K.ABS_TOL, K.REL_TOL * abs(x)) for w, x in el) + n * EPS * oc.get_usage(), n


@pytest.mark.parametrize("resident", [True, False])
@pytest.mark.parametrize("i", range(20))
def test_scripts_against_oracle_without_fetch(i, resident):
    ops = K.random_script(i, conc_limits=(i % 2 == 0), **SCRIPT_KW)
    s, cs, _ = K.replay(L, ops)
    s.set_resident(resident)
    o, ocs, _ = K.replay(O, ops)
    s.prepare()
    s.device_solve()
    ids, u = s.device_usage()  # no fetch
    o.solve()
    key = {c.h: k for k, c in cs.items()}
    assert len(ids) == s.last_stats()["n_cnst"] > 0 and len(set(ids.tolist())) == len(ids)
    worst = 0.0
    for h, uc in zip(ids.tolist(), u.tolist()):
        oc = ocs[key[h]]
        tol, _ = oracle_tol(oc)
        assert abs(uc - oc.get_usage()) <= tol, (key[h], uc, oc.get_usage(), tol)
        worst = max(worst, abs(uc - oc.get_usage()))
    listed = [c.h for c in s.active_constraints()]
    assert set(ids.tolist()) <= set(listed)
    for h in set(listed) - set(ids.tolist()):
        assert ocs[key[h]].get_usage() == 0.0, key[h]
    print(f"script {i}: {len(ids)} of {len(listed)} listed constraints returned, worst |gpu - oracle| {worst:.3e}")
    s.fetch()
    for h, uc in zip(ids.tolist(), u.tolist()):
        c = cs[key[h]]
        host = c.get_usage()
        assert abs(uc - host) <= c.get_variable_amount() * EPS * host, (key[h], uc, host)


def test_before_any_solve():
    s, _, _ = K.replay(L, K.random_script(0, **SCRIPT_KW))
    with pytest.raises(L.LmmError, match="no device solve"):
        s.device_usage()
    s.prepare()
    with pytest.raises(L.LmmError, match="no device solve"):
        s.device_usage()


# ---- 6: selective and resident -------------------------------------------------------------------------------

def build_halves(resident):
    """A selective system of two disconnected halves, each 20 constraints x 60 variables with 3 elements each."""
    rng = np.random.default_rng(777)
    s = L.System(True)
    s.set_resident(resident)
    halves = []
    for _ in range(2):
        cs = [s.constraint_new(None, float(rng.uniform(1.0, 20.0))) for _ in range(20)]
        cs[3].unshare()
        for j in range(60):
            v = s.variable_new(None, float(rng.choice([0.5, 1.0, 2.0])), 0.05 if j % 10 == 0 else -1.0, 3)
            for k in rng.choice(20, 3, replace=False):
                s.expand(cs[int(k)], v, float(rng.uniform(0.1, 2.0)))
        halves.append(cs)
    return s, halves


def selective_usage(resident):
    s, (first, second) = build_halves(resident)
    assert s.resident() == resident
    s.solve()
    assert s.last_stats()["n_cnst"] == 40
    s.update_constraint_bound(first[5], 0.5 * first[5].get_bound())
    s.prepare()
    s.device_solve()
    ids, u = s.device_usage()
    assert 0 < len(ids) <= 20 and set(ids.tolist()) <= {c.h for c in first}
    assert first[5].h in ids.tolist()
    s.fetch()
    by_h = {c.h: c for c in first}
    for h, uc in zip(ids.tolist(), u.tolist()):
        host = by_h[h].get_usage()
        assert abs(uc - host) <= by_h[h].get_variable_amount() * EPS * host, (h, uc, host)
    return ids, u


def test_selective_resident_and_not():
    ids_r, u_r = selective_usage(True)
    ids_h, u_h = selective_usage(False)
    assert ids_r.tobytes() == ids_h.tobytes()
    assert u_r.tobytes() == u_h.tobytes()


# ---- 7: raw ABI edges ----------------------------------------------------------------------------------------

def hip_runtime():
    """The HIP runtime this process already runs on (loaded with torch / liblmm_amd.so), by its mapped path."""
    L.lib()
    with open("/proc/self/maps") as maps:
        paths = sorted({ln.split()[-1] for ln in maps if "libamdhip64.so" in ln})
    assert len(paths) == 1, paths
    return ct.CDLL(paths[0])


def test_raw_abi_edges():
    import torch

    lib, hip = L.lib(), hip_runtime()
    hip.hipStreamCreate.argtypes = [ct.POINTER(ct.c_void_p)]
    hip.hipStreamSynchronize.argtypes = [ct.c_void_p]
    hip.hipStreamDestroy.argtypes = [ct.c_void_p]
    hip.hipMemcpy.argtypes = [ct.c_void_p, ct.c_void_p, ct.c_size_t, ct.c_int]
    D2H = 2  # hipMemcpyDeviceToHost
    # v0 on c0 (4) and c1 (3, FATPIPE), v1 on c0; c2 (5) has no element
    var_ptr, cnst_idx = np.array([0, 2, 3], np.int64), np.array([0, 1, 0], np.int32)
    weight, pen, vbound = np.array([1.0, 2.0, 3.0]), np.ones(2), -np.ones(2)
    cbound, cflags = np.array([4.0, 3.0, 5.0]), np.array([0, 1, 0], np.uint8)
    ctx, stream = ct.c_void_p(), ct.c_void_p()
    L._check_hip(lib.lmmhip_ctx_create(torch.cuda.current_device(), ct.byref(ctx)))
    try:
        assert hip.hipStreamCreate(ct.byref(stream)) == 0
        L._check_hip(lib.lmmhip_ctx_set_stream(ctx, stream))
        u = np.full(3, np.nan)
        assert lib.lmmhip_get_usage(ctx, p(u, ct.c_double)) == -4  # LMMHIP_E_STATE: nothing uploaded
        L._check_hip(lib.lmmhip_upload(ctx, 2, 3, 3, p(var_ptr, ct.c_int64), p(cnst_idx, ct.c_int32),
                                       p(weight, ct.c_double), p(pen, ct.c_double), p(vbound, ct.c_double),
                                       p(cbound, ct.c_double), p(cflags, ct.c_uint8)))
        dptr = ct.c_void_p()
        assert lib.lmmhip_get_usage(ctx, p(u, ct.c_double)) == -4  # uploaded, not solved
        assert lib.lmmhip_usage_device_ptr(ctx, ct.byref(dptr)) == -4
        L._check_hip(lib.lmmhip_solve(ctx, 0, L.get_precision()))
        assert lib.lmmhip_get_usage(ctx, None) == -3  # LMMHIP_E_ARG
        L._check_hip(lib.lmmhip_get_usage(ctx, p(u, ct.c_double)))
        x = np.full(2, np.nan)
        L._check_hip(lib.lmmhip_get_values(ctx, p(x, ct.c_double)))
        assert u[2] == 0.0
        assert u[0] == 1.0 * x[0] + 3.0 * x[1] and u[1] == 2.0 * x[0] and x[0] > 0 and x[1] > 0
        n = L.I64(-1)
        L._check_hip(lib.lmmhip_get_touched_cnsts(ctx, None, 0, ct.byref(n)))  # size query
        assert n.value == 3
        ids = np.full(3, -1, np.int32)
        assert lib.lmmhip_get_touched_cnsts(ctx, p(ids, ct.c_int32), 2, ct.byref(n)) == -3  # cap below the count
        L._check_hip(lib.lmmhip_get_touched_cnsts(ctx, p(ids, ct.c_int32), 3, ct.byref(n)))
        assert ids.tolist() == [0, 1, 2] and n.value == 3
        L._check_hip(lib.lmmhip_usage_device_ptr(ctx, ct.byref(dptr)))
        assert dptr.value
        assert hip.hipStreamSynchronize(stream) == 0
        d = np.full(3, np.nan)
        assert hip.hipMemcpy(d.ctypes.data, dptr, d.nbytes, D2H) == 0
        assert d.tobytes() == u.tobytes()
        L._check_hip(lib.lmmhip_ctx_use_own_stream(ctx))
    finally:
        lib.lmmhip_ctx_destroy(ctx)
        if stream:
            hip.hipStreamDestroy(stream)
