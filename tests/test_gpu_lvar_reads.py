"""Lazy threads and one-pass reads on list-valued resident variables (include/laspj.h
"list-valued resident variables": laspj_lvar_wait_needed / _read / _read_any / _lazy_count /
_lazy_at / _lazy_cancel; the pass k_lr_* of lasp_amd/csrc/laspj_lists.hip) against
tests/lvar_reads_model.py: every answer, the lazy and waiter listings and the value after
every step, and the device passes a call took.

A lazy threshold of [] cannot be registered through the ABI — wait_needed/6's own first clause
answers it (every value inflates [], and {strict, []} that would register is the FALLBACK
case) — so the pass's current of no entries is covered by a value of [] instead."""

import ctypes as C
import types

import pytest

import lvar_reads_model as rm
import lvars_model as lm
from oracle.terms import Atom

OK, FALLBACK = 0, 1
NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
A = Atom
tb = rm.tb
TILE = 256            # kLwTile: threshold entries per work item of the check launch

pytestmark = pytest.mark.gpu


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def _quad(ctx):
    from lasp_amd import engine
    l = ctx.var("orset")
    return types.SimpleNamespace(l=l, r=l.replica(), out=ctx.list_var(l), out2=ctx.list_var(l),
                                 read_any=engine.list_read_any)


def _passes(ctx):
    return lambda: ctx.nif_stats()["device_passes"]


def tok(k: int) -> bytes:
    return k.to_bytes(4, "big") + bytes(16)


def add(var, e, t):
    verd, res, _err, _minted = var.update(tb((A("add_by_token"), t, e)))
    assert (verd, res) == (OK, 0), (e, t)


def base(n, first=0):
    return [(e, [(tok(e), False)]) for e in range(first, first + n)]


GATE = [(9000, [(tok(9000), False)])]


class Both:
    """a list variable and its model, every answer asserted"""

    def __init__(self, out):
        self.d, self.m, self.next = out, rm.ListDv(), 1

    def id(self):
        self.next += 1
        return self.next - 1

    def check(self):
        assert self.d.lazy() == self.m.lazy_listing()
        assert self.d.waiters() == self.m.listing()

    def write(self, v):
        assert self.d.write(tb(v)) == OK
        self.m.wrote(v)
        fired, _flags = self.m.write()
        assert self.d.lazy() == []
        assert self.d.recheck(cap=64) == (OK, fired, len(self.m.waiting))
        self.check()

    def wait_needed(self, th, strict=False):
        i = self.id()
        want = self.m.wait_needed(th, strict, i)
        assert self.d.wait_needed(tb(th), strict, i) is want, (strict, len(th))
        self.check()
        return want

    def read(self, th, strict=False, cap=16):
        i = self.id()
        want = self.m.read(th, strict, i)
        got = self.d.read(tb(th), strict, i, cap)
        assert got == want, (got, want, strict, len(th))
        self.check()
        return want

    def readers_leave(self):
        for wid in [w[0] for w in self.m.waiting]:
            assert self.m.cancel(wid) and self.d.cancel(wid) is True


def test_random_scenario():
    ctx = _ctx()
    try:
        s = rm.ListReadScenario(rm.SEED, _quad(ctx), _passes(ctx)).run()
        assert s.c["fired_reads"] >= 10 and s.c["any_twice_removed"] >= 1, s.c
    finally:
        ctx.close()


# ---- shapes ------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    """one variable for the threshold sizes: a value of 600 entries"""
    ctx = _ctx()
    b = Both(ctx.list_var(ctx.var("orset")))
    b.write(base(600))
    yield b
    ctx.close()


@pytest.mark.parametrize("n", [0, 1, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_threshold_sizes(sized, n):
    """Read thresholds of 0, 1, 255, 256, 257 and 513 entries (the check launch's tile edges,
    finish's no-item case) against a value of 600 entries and two lazy thresholds, one of them
    longer than the value: met and unmet, strict and plain."""
    b = sized
    b.readers_leave()
    b.write(base(600))
    long_id, short_id = b.next, b.next + 1
    assert b.wait_needed(base(600) + GATE) is False          # 601 entries: its table is larger
    assert b.wait_needed(base(300) + GATE) is False
    th = base(n)
    assert b.read(th, False) == (True, [long_id, short_id] if n <= 300 else [long_id])
    assert b.read(th, True) == (True, [long_id, short_id] if n <= 300 else [long_id])
    if n:
        gated = base(n - 1) + GATE                           # its last entry: past a tile edge
        want = b.read(gated, n % 2 == 1)
        assert want == (False, [long_id, short_id] if n - 1 <= 300 else [long_id])
        assert b.m.lazy == ([] if n - 1 <= 300 else [b.m.lazy[0]])
        assert b.wait_needed(base(5) + GATE) is True         # a waiter is there (:739-741)


def test_lazy_list_sizes_and_an_empty_value():
    """Lazy thresholds of 1, 3, 255, 256 and 257 entries on one variable whose value is [] (a
    current of no entries), then under a value shorter than each of them: finish's stride, the
    binary searches over both item tables, strict reads against an equal lazy threshold."""
    ctx = _ctx()
    try:
        b = Both(ctx.list_var(ctx.var("orset")))
        sizes = [1, 3, TILE - 1, TILE, TILE + 1]
        for value in ([], [(9001, [(tok(9001), False)])]):
            b.readers_leave()
            b.write(value)
            ids = [b.next + k for k in range(len(sizes))]
            for s in sizes:
                assert b.wait_needed(base(s)) is False
            assert b.read([], False) == (True, ids)
            assert b.read([], True) == (bool(value), ids)
            if not value:
                b.readers_leave()
                for s in sizes:
                    assert b.wait_needed(base(s)) is False
                ids = [z[0] for z in b.m.lazy]
            assert b.read(value + base(1), False) == (False, ids if not value else [])
            b.readers_leave()
            if not b.m.lazy:
                for s in sizes:
                    assert b.wait_needed(base(s)) is False
            ids = [z[0] for z in b.m.lazy]
            assert b.read(base(TILE), True) == (False, ids[4:])      # 256 equals: not strict
            assert b.read(base(TILE), False) == (False, ids[3:4])
            assert b.read(base(4), False) == (False, ids[2:3])
            assert [len(z[1]) for z in b.m.lazy] == [1, 3]
            assert b.read(base(1), True) == (False, ids[1:2])
            assert b.read(base(1), True) == (False, [])
            assert b.read(base(1), False) == (False, ids[0:1])
            assert b.m.lazy == []
    finally:
        ctx.close()


def test_first_match_order_and_flags():
    ctx = _ctx()
    try:
        b = Both(ctx.list_var(ctx.var("orset")))
        ta, tc, t0, t1 = tok(1), tok(2), tok(3), tok(4)
        # keyfind's first match: only a later duplicate holds c, in the value and in the lazy
        b.write([(5, [(ta, False)]), (5, [(ta, False), (tc, False)])])
        lazy = [(5, [(ta, False)]), (3, [(t0, False)]), (5, [(ta, False), (tc, False)])]
        lid = b.next
        assert b.wait_needed(lazy) is False
        assert b.read([(5, [(tc, False)])], False) == (False, [])
        b.readers_leave()
        assert b.read([(5, [(ta, False)])], False) == (True, [lid])
        assert b.read([(5, [(ta, False)]), (5, [(ta, False)])], True) == (False, [lid])
        # a run in another order and a flipped flag under a strict read
        b.readers_leave()
        b.write([(1, [(t0, False), (t1, False)])])
        lazy = [(1, [(t0, False), (t1, False)]), (2, [(tc, False)])]
        lid = b.next
        assert b.wait_needed(lazy) is False
        assert b.read(lazy, True) == (False, [])                         # equal: not strict
        b.readers_leave()
        assert b.read(lazy, False) == (False, [lid])
        b.readers_leave()
        lid = b.next
        assert b.wait_needed(lazy) is False
        swapped = [(1, [(t1, False), (t0, False)]), (2, [(tc, False)])]
        flipped = [(1, [(t0, False), (t1, True)]), (2, [(tc, False)])]
        assert b.read([(1, [(t1, False), (t0, False)])], True) == (True, [lid])
        for th in (swapped, flipped):
            assert b.read(th, True) == (False, [lid])
            b.readers_leave()
            lid = b.next
            assert b.wait_needed(lazy) is False
    finally:
        ctx.close()


def test_cap_rule():
    """more fired than cap: nothing is changed, *nlazy says the room; the second call answers"""
    ctx = _ctx()
    try:
        out = ctx.list_var(ctx.var("orset"))
        b = Both(out)
        for k in range(5):
            assert b.wait_needed(base(2 + k)) is False
        th = tb(base(2))
        ids = (C.c_uint64 * 8)()
        met, verd, nl, still = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
        for cap in (2, 0):
            assert out.L.laspj_lvar_read(out.h, th, len(th), 0, 77, C.byref(met), ids, cap,
                                         C.byref(nl), C.byref(still), C.byref(verd)) == 0
            assert (verd.value, nl.value, still.value) == (OK, 5, 5)
            b.check()
        assert b.read(base(2), False, cap=5) == (False, [1, 2, 3, 4, 5])
        assert out.lazy() == [] and len(out.waiters()) == 1
        # read_any: the same rule over the reads' sum
        b.readers_leave()
        for k in range(3):
            assert b.wait_needed(base(2 + k)) is False
        from lasp_amd import engine
        want = rm.read_any([(b.m, base(2), False), (b.m, base(1), True)], 99)
        assert engine.list_read_any([(out, tb(base(2)), False), (out, tb(base(1)), True)], 99,
                                    cap=1) == want
        assert want[0] == -1 and len(want[1][0]) == 3
        b.check()
    finally:
        ctx.close()


# ---- device passes -----------------------------------------------------------------------
@pytest.mark.parametrize("L", [0, 1, 16])
def test_a_read_is_one_pass(L):
    ctx = _ctx()
    passes = _passes(ctx)
    try:
        d = _quad(ctx)
        b, b2 = Both(d.out), Both(d.out2)
        b.write(base(60))                                # (every term below is registered here)
        b.write(base(40))
        b2.write(base(7, 20))
        for k in range(L):
            assert b.wait_needed(base(41 + k)) is False
        assert b2.wait_needed(base(9, 20)) is False
        for th, strict in ((base(30), False), (base(45), True), (base(41 + L), False)):
            p0 = passes()
            b.read(th, strict)                           # every term is registered already
            assert passes() - p0 == 1, (L, len(th))
        # a read_any of four reads: one pass
        reads = [(b, base(50), False), (b2, base(8, 20), True), (b, base(44), False),
                 (b2, base(3, 20), False)]
        want = rm.read_any([(x.m, th, s) for x, th, s in reads], 500)
        p0 = passes()
        got = d.read_any([(x.d, tb(th), s) for x, th, s in reads], 500)
        assert passes() - p0 == 1
        assert got == want and want[0] == 3
        b.check()
        b2.check()
    finally:
        ctx.close()


def test_unseen_terms_take_no_more_passes_than_wait():
    ctx = _ctx()
    passes = _passes(ctx)
    try:
        out, twin = ctx.list_var(ctx.var("orset")), ctx.list_var(ctx.var("orset"))
        for v in (out, twin):
            assert v.write(tb(base(20))) == OK
        assert out.wait_needed(tb(base(21)), False, 1) is False
        th = tb(base(20) + [(A("unseen"), [(tok(77), False)])])
        p0 = passes()
        assert out.read(th, False, 2) == (False, [])
        p1 = passes()
        assert twin.wait(th, False, 2) == (OK, False)
        assert p1 - p0 <= passes() - p1
    finally:
        ctx.close()


# ---- lifecycle ---------------------------------------------------------------------------
def test_reset_widening_host_held_and_strict_wait_needed():
    ctx = _ctx()
    try:
        d = _quad(ctx)
        b = Both(d.out)
        b.write(base(5))
        # wait_needed(strict = 1) that would register: FALLBACK, nothing kept
        f0 = ctx.nif_stats()["fallbacks"]
        assert b.wait_needed(base(6), True) is None
        assert ctx.nif_stats()["fallbacks"] == f0 + 1 and d.out.lazy() == []
        assert b.wait_needed(base(3), True) is True              # met: answered, strict or not
        assert b.wait_needed(base(6)) is False
        assert b.wait_needed(base(4) + [(A("k"), [(tok(50), False)])]) is False
        before = d.out.lazy()
        # a dictionary reset: the lazy entries are walked back in at the next call and fire
        ctx.nif_reset()
        assert not d.out.resident and d.out.lazy() == before
        first = b.m.lazy[0][0]
        assert b.read(base(6), False) == (False, [first])
        assert d.out.resident
        ctx.nif_reset()
        b.readers_leave()
        assert b.wait_needed(base(7)) is False
        assert b.read(base(2), True) == (True, [z[0] for z in b.m.lazy])
        # a host-held value: FALLBACK, the listing intact
        before = d.out.lazy()
        bad = tb([1, 2, 3])
        held = ctx.list_var(d.l)
        assert held.write(bad) == FALLBACK and not held.resident
        assert held.wait_needed(tb(base(1)), False, 9) is None
        assert held.read(tb(base(1)), False, 9) == (None, [])
        assert d.read_any([(d.out, tb(base(1)), False), (held, tb(base(1)), False)], 9) == \
            (None, [])
        assert held.lazy() == [] and d.out.lazy() == before
        # an element's 65th token: the namespace goes wide — FALLBACK, the listing intact
        for k in range(66):
            add(d.l, 3, tok(3000 + k))
        assert ctx.nif_stats()["namespaces_widened"] >= 1
        assert d.out.read(tb(base(1)), False, 10) == (None, [])
        assert d.out.wait_needed(tb(base(9)), False, 11) is None
        assert d.read_any([(d.out, tb(base(1)), False)], 12) == (None, [])
        assert d.out.lazy() == before and d.out.waiters() == b.m.listing()
        assert d.out.lazy_cancel(before[0][0]) is True and len(d.out.lazy()) == len(before) - 1
    finally:
        ctx.close()


def test_every_write_empties_the_lazy_list():
    ctx = _ctx()
    try:
        d = _quad(ctx)
        out = d.out
        far = tb(base(3, 700))

        def lazy_again(v=out):
            if not v.lazy():
                assert v.wait_needed(far, False, 1) is False
            return v.lazy()

        add(d.l, 1, tok(1))
        add(d.r, 1, tok(2))
        assert len(lazy_again()) == 1
        assert out.intersection(d.l, d.r) == (OK, WRITTEN) and out.lazy() == []
        kept = lazy_again()
        assert out.intersection(d.l, d.r) == (OK, NOOP) and out.lazy() == kept
        assert out.intersection_recheck(d.l, d.r)[:2] == (OK, NOOP) and out.lazy() == kept
        add(d.l, 2, tok(3))
        add(d.r, 2, tok(4))
        assert out.intersection_recheck(d.l, d.r)[:2] == (OK, WRITTEN) and out.lazy() == []
        kept = lazy_again()
        assert out.bind(out.read()[1]) == (OK, NOOP) and out.lazy() == kept
        assert out.bind(tb([(8, [(tok(8), False)])])) == (OK, WRITTEN) and out.lazy() == []
        lazy_again()
        assert out.write(tb(lm.REFUSED_VALUE0)) == OK and out.lazy() == []
        kept = lazy_again()
        assert out.bind(tb(lm.REFUSED_VALUE)) == (OK, REFUSED) and out.lazy() == kept
        # a map run and a fold run into list variables of their own
        for make, fun in ((ctx.map, lambda x: x), (ctx.fold, lambda x: [x])):
            inv = ctx.var("orset")
            lv = ctx.list_var(inv)
            p = make(inv, lv)
            add(inv, 1, tok(1))
            assert len(lazy_again(lv)) == 1
            assert p.step(fun) == (OK, WRITTEN, 0) and lv.lazy() == []
            kept = lazy_again(lv)
            assert p.step(fun) == (OK, NOOP, 0) and lv.lazy() == kept
    finally:
        ctx.close()
