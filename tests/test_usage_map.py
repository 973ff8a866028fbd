"""The dense constraint -> constraint id map of the host flatten (lmm_flat_export_cnsts, System.flat_cnst_ids): the
ids lmm_device_usage reports its usages under.  Host only: the flatten is compared with the system's own records
and with the oracle built by the same script (CPU)."""
import numpy as np
import pytest

from oracle import pyoracle as O
from simgrid_amd import lmm as L
from simgrid_amd import multi as M
from tests import lmm_cases as K

SCRIPT_KW = dict(frees=3, penalty_updates=4, bound_updates=4)


def check_map(i, kind):
    ops = K.random_script(i, conc_limits=(i % 2 == 0), **SCRIPT_KW)
    s, cs, _ = K.replay(L, ops, kind=kind)
    o, ocs, _ = K.replay(O, ops, kind=kind)
    ids = s.flat_cnst_ids()
    f = M.export_flat(s)
    assert ids.dtype == np.int64 and len(ids) == len(f.cbound) > 0
    assert len(set(ids.tolist())) == len(ids)
    by_h = {c.h: (k, c) for k, c in cs.items()}
    for d, h in enumerate(ids.tolist()):
        c = by_h[h][1]
        assert f.cbound[d] == c.get_bound(), (d, h)
        assert bool(f.cflags[d] & 1) == (not c.is_shared()), (d, h)
    assert len(f.cnst_idx) > 0 and int(f.cnst_idx.max()) < len(ids) and int(f.cnst_idx.min()) >= 0
    # every flattened constraint is one the oracle holds active with an enabled element of weight > 0
    okey = {c.h: k for k, c in ocs.items()}
    used = {okey[c.h] for c in o.active_constraints() if c.get_variable_amount() > 0}
    assert {by_h[h][0] for h in ids.tolist()} <= used
    # ... and, listed in the order of the active set, the flatten keeps that order
    order = {c.h: n for n, c in enumerate(s.active_constraints())}
    pos = [order[h] for h in ids.tolist()]
    assert pos == sorted(pos)


@pytest.mark.parametrize("i", range(20))
def test_maxmin_scripts(i):
    check_map(i, L.System.MAXMIN)


def test_fair_bottleneck_script():
    check_map(3, L.System.FAIR_BOTTLENECK)


def test_capacity_is_checked():
    s, _, _ = K.replay(L, K.random_script(1, **SCRIPT_KW))
    n = len(s.flat_cnst_ids())
    buf = np.zeros(n, np.int64)
    assert L.lib().lmm_flat_export_cnsts(s.h, buf.ctypes.data_as(L.PI64), n - 1) == -1
    assert "cap" in L.lib().lmm_last_error().decode()
    assert L.lib().lmm_flat_export_cnsts(s.h, buf.ctypes.data_as(L.PI64), n) == 0
    assert buf.tolist() == s.flat_cnst_ids().tolist()
