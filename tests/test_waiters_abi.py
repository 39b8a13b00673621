"""Device-resident waiters at the C boundary (include/laspj.h "resident variables":
laspj_var_wait / _recheck / _recheck_many / _wait_cancel / _waiter_count / _waiter_at),
without a GPU: the entry points exist and reject null handles, and the random scenario the
GPU test replays (tests/waiters_model.py) is not vacuous on the reference model of
read/6 and reply_to_all/3 (lasp_core.erl:331-364, 765-825)."""

import ctypes as C

import pytest

from lasp_amd import _lib

import waiters_model as wm


@pytest.fixture(scope="module")
def lib():
    from lasp_amd import build
    build.build()
    return _lib.load()


def test_waiter_entry_points_reject_null_handles(lib):
    met, verd, found = C.c_int32(), C.c_int32(), C.c_int32()
    n32, left, strict = C.c_uint32(), C.c_uint32(), C.c_int32()
    wid, ln, p = C.c_uint64(), C.c_uint64(), C.c_void_p()
    ids = (C.c_uint64 * 4)()
    nmet = (C.c_uint32 * 1)()
    verds = (C.c_int32 * 1)()
    vars_ = (C.c_void_p * 1)()
    assert lib.laspj_var_wait(None, b"\x83j", 2, 0, 7, C.byref(met), C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_var_recheck(None, ids, 4, C.byref(n32), C.byref(left),
                                 C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_var_recheck_many(None, 1, vars_, ids, 4, nmet, verds) == _lib.E_INVAL
    assert lib.laspj_var_wait_cancel(None, 7, C.byref(found)) == _lib.E_INVAL
    assert lib.laspj_var_waiter_count(None, C.byref(n32)) == _lib.E_INVAL
    assert lib.laspj_var_waiter_at(None, 0, C.byref(wid), C.byref(strict), C.byref(p),
                                   C.byref(ln)) == _lib.E_INVAL
    assert lib.laspj_abi_version() == 2           # additive: the version stands


def test_reply_model_order():
    """reply_to_all replies in list order and keeps the rest in order (`StillWaiting0 ++
    [H]`, lasp_core.erl:765-825); a met threshold is not registered (:331-364)."""
    m = wm.ReplyModel("gset")
    assert m.wait([], False, 1) is True and m.waiting == []
    assert m.wait([], True, 1) is False                 # {strict, []} of new()
    assert m.wait([1], False, 2) is False
    assert m.wait([5], False, 3) is False
    assert m.wait([1, 2], False, 2) is False            # the same id twice
    m.value = [1, 2]
    fired, flags = m.write()
    assert fired == [1, 2, 2] and flags == [True, True, False, True]
    assert [w[0] for w in m.waiting] == [3]
    assert m.cancel(9) is False and m.cancel(3) is True and m.waiting == []


@pytest.mark.parametrize("kind", ["orset", "gset"])
def test_scenario_is_not_vacuous(kind):
    s = wm.Scenario(wm.SEEDS[kind], kind).run(300)
    c = s.counts
    assert sum(c["fired_later"].values()) >= 30, c
    assert sum(c["survived"].values()) >= 30, c
    assert sum(c["met_at_wait"].values()) >= 10, c
    for cls in c.values():
        assert cls[False] > 0 and cls[True] > 0, c      # strict and non-strict in each
    assert s.gap_writes >= 1
    assert s.empty_rechecks >= 1 and s.rechecks > s.empty_rechecks
    assert s.cancels[True] >= 1 and s.cancels[False] >= 1
