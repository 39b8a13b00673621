"""Blocking reads on list-valued variables without a GPU (include/laspj.h "list-valued resident
variables": laspj_lvar_wait / _recheck / _intersection_recheck / _wait_cancel / _waiter_count /
_waiter_at): the model of read/6 and reply_to_all/3 on list values (lasp_core.erl:331-364,
765-825; lasp_lattice.erl:72-75, 153-161, 235-253) is pinned on literals, the random scenario
the GPU test replays is not vacuous on it, and the entry points exist and reject null
handles."""

import ctypes as C

import pytest

from lasp_amd import _lib

import lvar_waiters_model as lwm

NAMES = ("laspj_lvar_wait", "laspj_lvar_recheck", "laspj_lvar_intersection_recheck",
         "laspj_lvar_wait_cancel", "laspj_lvar_waiter_count", "laspj_lvar_waiter_at")


@pytest.mark.parametrize("name,value,threshold,strict,met", lwm.LITERALS,
                         ids=[x[0] for x in lwm.LITERALS])
def test_literals(name, value, threshold, strict, met):
    m = lwm.ListReplyModel()
    m.value = value
    assert m.met(strict, threshold) is met
    # read/6: met -> nothing kept; unmet -> appended, and a write of the same value keeps it
    assert m.wait(threshold, strict, 7) is met
    assert m.listing() == ([] if met else [(7, strict, lwm.tb(threshold))])
    assert m.write() == ([], [] if met else [False])


def test_reply_order_on_lists():
    """reply_to_all replies in list order and keeps the unmet entries in order
    (`StillWaiting0 ++ [H]`, lasp_core.erl:765-825)."""
    m = lwm.ListReplyModel()
    a, b = (1, [(b"x", False)]), (2, [(b"y", False)])
    assert m.wait([a], False, 1) is False
    assert m.wait([b], False, 2) is False
    assert m.wait([a], True, 3) is False
    assert m.wait([a, b], True, 1) is False               # the same id twice
    m.value = [a]
    fired, flags = m.write()
    # {strict, [a]} on [a]: nothing changed and no new element
    assert fired == [1] and flags == [True, False, False, False]
    m.value = [b, a]
    fired, flags = m.write()
    assert fired == [2, 3] and flags == [True, True, False]     # [a] < [b, a] by length/1
    assert [w[0] for w in m.waiting] == [1]
    assert m.cancel(9) is False and m.cancel(1) is True and m.waiting == []


def test_scenario_is_not_vacuous():
    s = lwm.ListScenario(lwm.SEED).run()
    c = s.counts
    for name in ("met_at_wait", "fired_later", "survived"):
        assert c[name][False] >= 5 and c[name][True] >= 5, c     # strict and non-strict alike
    assert s.gap_writes >= 1
    assert s.empty_rechecks >= 1 and s.rechecks > s.empty_rechecks
    assert s.cancels[True] >= 1
    assert s.status[lwm.WRITTEN] >= 10 and s.status[lwm.NOOP] >= 1, s.status


@pytest.fixture(scope="module")
def lib():
    from lasp_amd import build
    build.build()
    return _lib.load()


def test_entry_points_are_declared_exported_and_bound(lib):
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                            "include", "laspj.h")).read()
    for name in NAMES:
        assert ("int %s(" % name) in hdr, name
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name


def test_entry_points_reject_null_handles(lib):
    met, verd, found, st = C.c_int32(), C.c_int32(), C.c_int32(), C.c_int32()
    n32, left, strict = C.c_uint32(), C.c_uint32(), C.c_int32()
    wid, ln, p = C.c_uint64(), C.c_uint64(), C.c_void_p()
    ids = (C.c_uint64 * 4)()
    assert lib.laspj_lvar_wait(None, b"\x83j", 2, 0, 7, C.byref(met),
                               C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_recheck(None, ids, 4, C.byref(n32), C.byref(left),
                                  C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_intersection_recheck(None, None, None, C.byref(st), ids, 4,
                                               C.byref(n32), C.byref(left),
                                               C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_lvar_wait_cancel(None, 7, C.byref(found)) == _lib.E_INVAL
    assert lib.laspj_lvar_waiter_count(None, C.byref(n32)) == _lib.E_INVAL
    assert lib.laspj_lvar_waiter_at(None, 0, C.byref(wid), C.byref(strict), C.byref(p),
                                    C.byref(ln)) == _lib.E_INVAL
    assert lib.laspj_abi_version() == 2           # additive: the version stands
