"""Blocking reads on list-valued resident variables (include/laspj.h "list-valued resident
variables": laspj_lvar_wait / _recheck / _intersection_recheck / _wait_cancel / _waiter_count /
_waiter_at; the check pass k_lw_* of lasp_amd/csrc/laspj_lists.hip) against
tests/lvar_waiters_model.py: met, the fired ids in list order, the count left, the waiter
listing and the value after every step, and the device passes each call took."""

import ctypes as C
import types

import pytest

import lvar_waiters_model as lwm
import lvars_model as lm
import update4_model as um
from oracle.terms import Atom

OK, FALLBACK = 0, 1
NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
A = Atom
tb = lwm.tb
TILE = 256            # kLwTile: threshold entries per work item of the check launch

pytestmark = pytest.mark.gpu


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def _trio(ctx):
    l = ctx.var("orset")
    return types.SimpleNamespace(l=l, r=l.replica(), out=ctx.list_var(l))


def _passes(ctx):
    return lambda: ctx.nif_stats()["device_passes"]


def tok(k: int) -> bytes:
    return k.to_bytes(4, "big") + bytes(16)


def add(var, e, t):
    verd, res, _err, _minted = var.update(tb((A("add_by_token"), t, e)))
    assert (verd, res) == (OK, 0), (e, t)


def listing(ws):
    return [(i, s, tb(th)) for i, s, th in ws]


def test_random_scenario():
    ctx = _ctx()
    try:
        s = lwm.ListScenario(lwm.SEED, _trio(ctx), _passes(ctx)).run()
        assert s.fused >= 5 and s.status[WRITTEN] >= 10
    finally:
        ctx.close()


# ---- tile and wave edges -----------------------------------------------------------------
SIZES = [1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1, 0]


def _edge_waiters(n, W):
    """W thresholds of SIZES entries in turn over the keys of an n-entry value, each unmet
    until its own gate entry {5000 + k, [gate]} is in the value; every other one strict, its
    gate token's flag flipped so that the strict read sees a change."""
    ws = []
    for k in range(W):
        size, strict = SIZES[k % len(SIZES)], k % 2 == 1
        if size == 0:
            ws.append((k + 1, True, []))            # {strict, []}: met by any non-empty value
            continue
        body = [(i % n, [(tok(i % n), False)]) for i in range(size - 1)]
        ws.append((k + 1, strict, body + [(5000 + k, [(tok(5000 + k), strict)])]))
    return ws


def _edge_value(n, sel):
    """the n-entry value with the gate entries of the waiters in sel: before it (the keyfind
    table is then offset) for an odd count, after it otherwise"""
    base = [(e, [(tok(e), False)]) for e in range(n)]
    gates = [(5000 + k, [(tok(5000 + k), False)]) for k in sel]
    return gates + base if len(sel) % 2 else base + gates


@pytest.mark.parametrize("n", [1, 2049])
@pytest.mark.parametrize("W", [1, 2, 63, 64, 65, 130])
def test_tile_and_wave_edges(n, W):
    """Thresholds of 0, 1, tile-1, tile, tile+1 and 2 tile+1 entries in one recheck, over 1 to
    130 waiters (the item search, the finish block's stride and the descriptor upload cross
    their boundaries), against a value of 1 and of 2049 entries; only the last, only the
    first, alternate waiters or none are met."""
    ctx = _ctx()
    passes = _passes(ctx)
    try:
        peer = ctx.var("orset")
        out = ctx.list_var(peer)
        ws = _edge_waiters(n, W)
        gated = [k for k in range(W) if ws[k][2]]
        patterns = {"last": gated[-1:], "first": gated[:1], "alternate": gated[::2], "none": []}
        for name, sel in patterns.items():
            where = (n, W, name)
            assert out.write(tb([])) == OK
            for wid, strict, th in ws:
                assert out.wait(tb(th), strict, wid) == (OK, False), where
            assert out.waiters() == listing(ws), where
            value = _edge_value(n, sel)
            # by construction: a gated waiter is met exactly when its gate is in the value,
            # {strict, []} by any value; the clause-by-clause model agrees where it is cheap
            want = [(k in sel) if ws[k][2] else True for k in range(W)]
            if n == 1:
                for k in range(0, W, 7):
                    assert want[k] == lm.threshold(value, ws[k][2], ws[k][1]), (where, k)
            assert out.write(tb(value)) == OK
            p0 = passes()
            verd, fired, left = out.recheck(cap=W)
            assert passes() - p0 == 1, where
            assert verd == OK, where
            assert fired == [ws[k][0] for k in range(W) if want[k]], where
            rest = [ws[k] for k in range(W) if not want[k]]
            assert left == len(rest) and out.waiters() == listing(rest), where
            assert out.read() == (OK, tb(value)), where
            for wid, _s, _th in rest:
                assert out.cancel(wid) is True
            p0 = passes()
            assert out.recheck() == (OK, [], 0) and passes() == p0, where   # no device work
    finally:
        ctx.close()


# ---- literals ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,value,threshold,strict,met", lwm.LITERALS,
                         ids=[x[0] for x in lwm.LITERALS])
def test_literals(name, value, threshold, strict, met):
    """Each literal twice: read/6 on the value as written (laspj_lvar_etf_write keeps repeated
    and descending keys resident), and registered on [] and decided by the re-check pass."""
    ctx = _ctx()
    try:
        peer = ctx.var("orset")
        out = ctx.list_var(peer)
        assert out.write(tb(value)) == OK
        assert out.wait(tb(threshold), strict, 7) == (OK, met)
        want = [] if met else [(7, strict, tb(threshold))]
        assert out.waiters() == want
        assert out.recheck() == (OK, [], len(want))           # the value has not changed
        assert out.waiters() == want
        out.cancel(7)
        # through the check pass
        assert out.write(tb([])) == OK
        on_empty = lm.threshold([], threshold, strict)
        assert out.wait(tb(threshold), strict, 9) == (OK, on_empty)
        assert out.write(tb(value)) == OK
        if on_empty:
            assert out.recheck() == (OK, [], 0)
        else:
            assert out.recheck() == ((OK, [9], 0) if met else (OK, [], 1))
        assert out.read() == (OK, tb(value))
    finally:
        ctx.close()


# ---- token runs --------------------------------------------------------------------------
def test_token_runs():
    """Thresholds with runs of 1, 2, 63 and 64 tokens under one key, and the `Cx ++ Cy` run of
    a real intersection: registered on [], decided when the re-run writes."""
    ctx = _ctx()
    try:
        d = _trio(ctx)
        lt = [tok(100 + k) for k in range(32)]
        rt = [tok(200 + k) for k in range(32)]
        for k in range(32):
            add(d.l, 5, lt[k])
            add(d.r, 5, rt[k])
        add(d.l, 9, tok(1))
        add(d.r, 9, tok(2))
        lval = [(5, [(t, False) for t in lt]), (9, [(tok(1), False)])]
        rval = [(5, [(t, False) for t in rt]), (9, [(tok(2), False)])]
        st, new = lm.intersection(lval, rval, [])
        run = dict(new)[5]
        assert st == WRITTEN and len(run) == 64 and run[:32] == [(t, False) for t in lt]
        m = lwm.ListReplyModel()
        wid = 0
        for n in (1, 2, 63, 64):
            for th in ([(5, run[:n])], [(5, run[64 - n:])], [(5, run[:n][::-1])],
                       [(5, [(t, True) for t, _f in run[:n]])]):
                for strict in (False, True):
                    wid += 1
                    assert m.wait(th, strict, wid) is False
                    assert d.out.wait(tb(th), strict, wid) == (OK, False), (n, strict)
            if n == 2:
                # two that stay (a key the value never gets), between those that fire
                for strict in (False, True):
                    wid += 1
                    th = [(5, run[:2]), (7, [(tok(7), False)])]
                    assert m.wait(th, strict, wid) is False
                    assert d.out.wait(tb(th), strict, wid) == (OK, False)
        m.value = new
        fired, _flags = m.write()
        assert len(fired) == wid - 2 and [w[0] for w in m.waiting] == [17, 18]
        got = d.out.intersection_recheck(d.l, d.r, cap=wid)
        assert got == (OK, WRITTEN, fired, len(m.waiting))
        assert d.out.waiters() == m.listing()
        assert d.out.read() == (OK, tb(new))
    finally:
        ctx.close()


# ---- cap overflow ------------------------------------------------------------------------
def _raw_recheck(out, cap):
    ids = (C.c_uint64 * max(cap, 1))()
    nmet, left, verd = C.c_uint32(), C.c_uint32(), C.c_int32()
    assert out.L.laspj_lvar_recheck(out.h, ids, cap, C.byref(nmet), C.byref(left),
                                    C.byref(verd)) == 0
    return verd.value, nmet.value, left.value, (list(ids[:nmet.value]) if nmet.value <= cap else [])


def _raw_fused(out, l, r, cap):
    ids = (C.c_uint64 * max(cap, 1))()
    st, nmet, left, verd = C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_int32()
    assert out.L.laspj_lvar_intersection_recheck(out.h, l.h, r.h, C.byref(st), ids, cap,
                                                 C.byref(nmet), C.byref(left),
                                                 C.byref(verd)) == 0
    return verd.value, st.value, nmet.value, left.value, (list(ids[:nmet.value]) if nmet.value <= cap else [])


def test_cap_overflow():
    ctx = _ctx()
    try:
        d = _trio(ctx)
        add(d.l, 1, tok(1))
        add(d.r, 1, tok(2))
        ths = [[(1, [(tok(1), False)])], [(1, [(tok(2), False)])], [(7, [(tok(3), False)])],
               [(1, [(tok(1), False), (tok(2), False)])]]
        for out in (d.out, ctx.list_var(d.l)):
            for k, th in enumerate(ths):
                assert out.wait(tb(th), False, 10 + k) == (OK, False)
        # the fused call: written, three met, room for two: nothing removed
        assert _raw_fused(d.out, d.l, d.r, 2) == (OK, WRITTEN, 3, 4, [])
        assert len(d.out.waiters()) == 4
        assert _raw_recheck(d.out, 2) == (OK, 3, 4, [])
        assert _raw_recheck(d.out, 3) == (OK, 3, 1, [10, 11, 13])
        assert d.out.waiters() == listing([(12, False, ths[2])])
        # the same through recheck alone
        assert out.intersection(d.l, d.r) == (OK, WRITTEN)
        assert _raw_recheck(out, 0) == (OK, 3, 4, [])
        assert _raw_recheck(out, 2) == (OK, 3, 4, [])
        assert out.recheck(cap=2) == (OK, [10, 11, 13], 1)
    finally:
        ctx.close()


# ---- the fused re-run ----------------------------------------------------------------------
def test_fused_rerun_equals_the_two_calls():
    """A twin pair over one l and r: laspj_lvar_intersection_recheck on one,
    laspj_lvar_intersection then laspj_lvar_recheck on the other, item for item through
    WRITTEN, NOOP and REFUSED, one device pass against two in the ascending steady state, and
    the same answers after a descending foreign bind sends the re-run down the merge path."""
    ctx = _ctx()
    passes = _passes(ctx)
    try:
        d = _trio(ctx)
        twin = ctx.list_var(d.l)
        m = lwm.ListReplyModel()
        lval, rval = [], []
        nid = [0]
        seen = {NOOP: 0, WRITTEN: 0, REFUSED: 0}

        def wait(th, strict):
            nid[0] += 1
            met = m.wait(th, strict, nid[0])
            for out in (d.out, twin):
                assert out.wait(tb(th), strict, nid[0]) == (OK, met), (th, strict)

        def upd(left, e, t):
            nonlocal lval, rval
            add(d.l if left else d.r, e, t)
            cur = lval if left else rval
            new = um.update4("orset", (A("add_by_token"), t, e), cur, [])[1]
            if left:
                lval = new
            else:
                rval = new

        def rerun(steady):
            st, new = lm.intersection(lval, rval, m.value)
            seen[st] += 1
            nwait = len(m.waiting)
            fired = []
            if st == WRITTEN:
                m.value = new
                fired, _flags = m.write()
            p0 = passes()
            got = d.out.intersection_recheck(d.l, d.r, cap=8)
            p1 = passes()
            assert twin.intersection(d.l, d.r) == (OK, st)
            two = twin.recheck(cap=8) if st == WRITTEN else (OK, [], nwait)
            p2 = passes()
            assert got == (OK, st, fired, len(m.waiting)), (got, st, fired)
            assert two == (OK, fired, len(m.waiting))
            assert d.out.waiters() == twin.waiters() == m.listing()
            assert d.out.read() == twin.read() == (OK, tb(m.value))
            if steady and st == WRITTEN and nwait:
                assert (p1 - p0, p2 - p1) == (1, 2)
            return st

        for e in range(6):
            upd(True, e, tok(10 + e))
        for e in range(3, 9):
            upd(False, e, tok(20 + e))
        wait([(4, [(tok(14), False)])], False)
        wait([(4, [(tok(14), False), (tok(24), False)])], True)
        wait([(8, [(tok(28), False)])], False)            # 8 is not in l yet
        wait([], True)
        assert rerun(False) == WRITTEN                    # the first write: from []
        assert rerun(True) == NOOP
        # steady re-runs: one more element, one more token, a waiter on each
        for k in range(4):
            e = 6 + k % 3
            wait(lm.bind(m.value, lm.acc_value(
                um.update4("orset", (A("add_by_token"), tok(40 + k), e), lval, [])[1],
                rval))[1], k % 2 == 0)
            wait([(e, [(tok(40 + k), False)])], False)
            upd(True, e, tok(40 + k))
            assert rerun(True) == WRITTEN
            # (NOOP, or WRITTEN again where the merge as written differs from AccValue: the
            # model decides)
            rerun(True)
        # a descending foreign bind on both: not_asc, the merge path from here on
        foreign = [(A("z"), [(b"t1", False)]), (7, [(tok(41), True)]), (3, [(tok(23), False)])]
        st, new = lm.bind(m.value, foreign)
        for out in (d.out, twin):
            assert out.bind(tb(foreign)) == (OK, st)
        if st == WRITTEN:
            m.value = new
            fired, _flags = m.write()
            for out in (d.out, twin):
                assert out.recheck(cap=8) == (OK, fired, len(m.waiting))
        for k in range(3):
            wait([(2, [(tok(60 + k), False)])], k == 1)
            upd(True, 2, tok(60 + k))
            upd(False, 2, tok(70 + k))
            rerun(False)
        # a value the merge does not inflate: REFUSED, nothing fires
        # (orddict:merge walks the value's descending keys as if they ascended: the merge
        # meets key 1 first with AccValue's tokens only, and keyfind takes that first match)
        upd(False, 1, tok(81))
        refused0 = [(2, [(tok(90), False)]), (1, [(tok(91), False)])]
        for out in (d.out, twin):
            assert out.write(tb(refused0)) == OK
        m.value = refused0
        fired, _flags = m.write()
        for out in (d.out, twin):
            assert out.recheck(cap=8) == (OK, fired, len(m.waiting))
        wait([(1, [(tok(99), False)])], False)
        assert rerun(False) == REFUSED
        assert seen[WRITTEN] >= 6 and seen[NOOP] >= 1 and seen[REFUSED] == 1, seen
    finally:
        ctx.close()


# ---- lifecycle ---------------------------------------------------------------------------
def test_lifecycle_growth_reset_widening_cancel():
    ctx = _ctx()
    try:
        d = _trio(ctx)
        m = lwm.ListReplyModel()
        for e in range(5):
            add(d.l, e, tok(e))
            add(d.r, e, tok(100 + e))
        lval = [(e, [(tok(e), False)]) for e in range(5)]
        rval = [(e, [(tok(100 + e), False)]) for e in range(5)]
        st, m.value = lm.intersection(lval, rval, [])
        assert d.out.intersection_recheck(d.l, d.r) == (OK, WRITTEN, [], 0)

        def wait(th, strict, wid):
            met = m.wait(th, strict, wid)
            assert d.out.wait(tb(th), strict, wid) == (OK, met)

        def written(value):
            m.value = value
            fired, _flags = m.write()
            assert d.out.recheck() == (OK, fired, len(m.waiting))
            assert d.out.waiters() == m.listing()
            return fired

        # cancelling the middle one of three
        wait([(50, [(tok(50), False)])], False, 1)
        wait([(51, [(tok(51), False)])], True, 2)
        wait([(52, [(tok(52), False)])], False, 3)
        assert d.out.cancel(2) is True and m.cancel(2) is True
        assert d.out.cancel(2) is False
        assert d.out.waiters() == m.listing() and len(m.waiting) == 2
        # growth: a never-seen element registered between wait and recheck
        wait([(A("new"), [(tok(7), False)])], False, 4)
        add(d.l, A("grown"), tok(8))
        add(d.r, A("grown"), tok(9))
        add(d.l, A("new"), tok(7))
        add(d.r, A("new"), tok(10))
        lval += [(A("grown"), [(tok(8), False)]), (A("new"), [(tok(7), False)])]
        rval += [(A("grown"), [(tok(9), False)]), (A("new"), [(tok(10), False)])]
        st, new = lm.intersection(lval, rval, m.value)
        assert st == WRITTEN
        m.value = new
        fired, _flags = m.write()
        assert fired == [4]
        assert d.out.intersection_recheck(d.l, d.r) == (OK, WRITTEN, [4], 2)
        # a dictionary reset between wait and recheck: the waiters are walked back in, their
        # ids and order kept
        wait([(0, [(tok(0), False), (tok(100), False)]), (60, [(tok(60), False)])], False, 5)
        wait(m.value, True, 6)
        before = d.out.waiters()
        ctx.nif_reset()
        assert not d.out.resident and d.out.waiters() == before == m.listing()
        assert d.out.recheck() == (OK, [], 4)
        assert d.out.resident and d.out.waiters() == before
        assert written_via_write(d.out, m, m.value + [(60, [(tok(60), False)])]) == [5, 6]
        ctx.nif_reset()
        assert d.out.wait(tb([(50, [(tok(50), False)])]), True, 8) == (OK, False)
        m.wait([(50, [(tok(50), False)])], True, 8)
        assert d.out.waiters() == m.listing()
        assert written_via_write(d.out, m, m.value + [(50, [(tok(50), True)])]) == [1, 8]
        # an element's 65th token: the namespace goes wide — FALLBACK, nothing fires, the
        # waiters intact
        before = d.out.waiters()
        value = d.out.read()
        for k in range(66):
            add(d.l, 3, tok(3000 + k))
        assert ctx.nif_stats()["namespaces_widened"] >= 1
        assert d.out.recheck() == (FALLBACK, [], 1)
        assert d.out.intersection_recheck(d.l, d.r) == (FALLBACK, NOOP, [], 1)
        assert d.out.wait(tb([]), True, 9) == (FALLBACK, None)
        assert d.out.waiters() == before == m.listing() and d.out.read() == value
        assert d.out.cancel(3) is True and d.out.waiters() == []
    finally:
        ctx.close()


def written_via_write(out, m, value):
    """write/4 of value, then reply_to_all: the fired ids (asserted against the model)"""
    assert out.write(tb(value)) == OK
    m.value = value
    fired, _flags = m.write()
    assert out.recheck() == (OK, fired, len(m.waiting))
    assert out.waiters() == m.listing()
    return fired


def test_peer_or_context_gone_first():
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        peer = ctx.var("orset")
        out = ctx.list_var(peer)
        th = [(1, [(b"a", False)])]
        assert out.wait(tb(th), False, 1) == (OK, False)
        peer.close()                                      # the namespace is shared-owned
        assert out.wait(tb(th), True, 2) == (OK, False)
        assert out.write(tb(th)) == OK
        assert out.recheck() == (OK, [1], 1)
        out.close()                                       # with a waiter left
        l = ctx.var("orset")
        out = ctx.list_var(l)
        assert out.wait(tb(th), False, 3) == (OK, False)
    finally:
        ctx.close()
    # the context went first: every call answers E_INVAL, destroy still frees
    for call in (lambda: out.wait(tb([]), True, 4), out.recheck, out.waiters,
                 lambda: out.cancel(3), lambda: out.intersection_recheck(l, l)):
        with pytest.raises(_lib.LaspjError) as ex:
            call()
        assert ex.value.status == _lib.E_INVAL
    out.close()
    l.close()


def test_every_fallback_cause_leaves_value_and_waiters():
    ctx = _ctx()
    try:
        d = _trio(ctx)
        add(d.l, 1, tok(1))
        add(d.r, 1, tok(2))
        assert d.out.intersection(d.l, d.r) == (OK, WRITTEN)
        th = [(2, [(tok(3), False)])]
        assert d.out.wait(tb(th), False, 1) == (OK, False)
        value, ws = d.out.read(), d.out.waiters()
        n0 = ctx.nif_stats()["dict_elements"]
        f0 = ctx.nif_stats()["fallbacks"]
        # images the walk refuses: nothing registered, the walk's registrations undone
        for bad in (tb([1, 2, 3]), tb([(77, [b"t"])]), tb([(78, [(b"t", 3)])]), tb(A("x")),
                    tb([(79, [(bytes([k]), False) for k in range(65)])])):
            assert d.out.wait(bad, False, 2) == (FALLBACK, None)
            assert d.out.wait(bad, True, 2) == (FALLBACK, None)
            assert d.out.read() == value and d.out.waiters() == ws
        assert ctx.nif_stats()["dict_elements"] == n0
        # inputs the intersection does not take: its own FALLBACK, nothing checked
        other = ctx.var("orset")
        g = ctx.var("gset")
        for a, b in ((other, d.r), (d.l, other), (g, d.r), (d.l, g)):
            assert d.out.intersection_recheck(a, b) == (FALLBACK, NOOP, [], 1)
            assert d.out.read() == value and d.out.waiters() == ws
        # the value held on the host by a write the walk refused
        bad = tb([1, 2, 3])
        assert d.out.write(bad) == FALLBACK and not d.out.resident
        assert d.out.wait(tb(th), False, 3) == (FALLBACK, None)
        assert d.out.recheck() == (FALLBACK, [], 1)
        assert d.out.intersection_recheck(d.l, d.r) == (FALLBACK, NOOP, [], 1)
        assert d.out.read() == (OK, bad) and d.out.waiters() == ws
        assert ctx.nif_stats()["fallbacks"] >= f0 + 17
        # until the next write
        assert d.out.write(tb(th)) == OK
        assert d.out.recheck() == (OK, [1], 0)
    finally:
        ctx.close()
