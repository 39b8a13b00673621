"""Lazy threads and one-pass reads (include/laspj.h: laspj_var_read / _read_any /
_wait_needed / _lazy_count / _lazy_at / _lazy_cancel; lasp_amd/csrc/laspj_reads.hip
k_read_check) against the reference model of read/6, read_any/3, wait_needed/6, write/4 and
reply_to_all (lasp_core.erl:331-420, 730-758, 765-844) in tests/reads_model.py.  Every answer
is compared exactly: met / found, the fired lazy ids and their order, and the waiter and lazy
lists through laspj_var_waiter_at / laspj_var_lazy_at; after a bind laspj_var_recheck must
fire the waiters laspj_var_read made.

The kernel's wave item is one tile of kReadTile = 128 16-byte units of one read — 128 element
slots of a narrow OR-Set (one {p, r} pair each), 256 bitmap words of a G-Set (two each, an
odd last word a unit's first half) — and a wave takes a read's currents (the value, then its
lazy thresholds) in chunks of kReadChunk = 16, four loads ahead: 16 lazy threads are 17
currents, two chunks.
"""

import ctypes as C

import pytest

from oracle import orset as oorset
from oracle.terms import Atom, exact_eq

import reads_model as rm
import waiters_model as wm
from reads_model import FALLBACK, OK, Dv, ReferenceRaises, tb

A = Atom
pytestmark = pytest.mark.gpu
TILE = 128            # kReadTile (laspj_internal.h)


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def T(k, salt=0):
    return bytes([salt]) + k.to_bytes(4, "big") + b"\x55" * 15


def st(ks, salt=0):
    """an OR-Set state: elements ks, one token each"""
    return [(k, [(T(k, salt), False)]) for k in ks]


def plus(state, k, salt, removed=False):
    """state with one more token on element k"""
    return oorset.merge(state, [(k, [(T(k, salt), removed)])])


class Both:
    """a resident variable and the model of its #dv, kept in step; every answer of the
    device is asserted against the model's, and both lists after every call"""

    def __init__(self, ctx, kind, var=None):
        self.kind, self.ctx = kind, ctx
        self.v = var if var is not None else ctx.var(kind)
        self.m = Dv(kind)

    def same_lists(self, where=None):
        assert self.v.waiters() == self.m.waiting_listing(), where
        assert self.v.lazy() == self.m.lazy_listing(), where

    def read(self, th, strict, rid, cap=16):
        want = self.m.read(th, strict, rid)
        assert self.v.read(self.m.image(th), strict, rid, cap=cap) == want, (rid, strict)
        self.same_lists((rid, strict))
        return want

    def wait_needed(self, th, strict, wid):
        want = self.m.wait_needed(th, strict, wid)
        assert self.v.wait_needed(self.m.image(th), strict, wid) is want, (wid, strict)
        self.same_lists(wid)
        return want

    def written(self, value):
        """the model's write/4 behind a WRITTEN / UPDATE_OK answer, then the re-check"""
        fired = self.m.write(value)
        assert self.v.recheck() == (OK, fired, len(self.m.waiting))
        self.same_lists()
        return fired

    def bind(self, state):
        noop = exact_eq(state, self.m.value)
        assert self.v.bind(tb(state)) == (OK, 0 if noop else 1)
        if noop:
            self.same_lists()           # Value0 =:= Value: nothing is written
            return []
        return self.written(wm.merge(self.kind, self.m.value, state))

    def update(self, op):
        verd, res, _err, minted = self.v.update(tb(op))
        want = wm.oracle_update(self.kind, op, self.m.value, minted)
        assert (verd, res) == (OK, 0) and want[0] == "ok", op
        return self.written(want[1])


def _edges(n):
    return sorted({0, n - 1} | {p for t in (1, 2) for p in (t * TILE - 1, t * TILE) if p < n})


# ---------------------------------------------------------------- element slots

def _orset_var(ctx, n, p):
    """n element slots, one token each; lazy threads that differ from the read's threshold
    T = V + token b on p in one cell: 10 equal, 11 the same tokens with b's removed flag
    set, 12 lacks b on p (another token on the other edge instead), 13 only element p"""
    b = Both(ctx, "orset")
    b.bind(st(range(n)))
    V = b.m.value
    q = 0 if p else n - 1
    assert b.wait_needed(plus(V, p, 1), False, 10) is False
    assert b.wait_needed(plus(V, p, 1, removed=True), False, 11) is False
    assert b.wait_needed(plus(V, q, 2), False, 12) is False
    assert b.wait_needed(plus(st([p]), p, 1), False, 13) is False
    return b, V


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1])
def test_orset_shapes_single_cell_decides(n):
    """The deciding cell sits first, last or on a tile edge.  Non-strict: `violation` alone
    (12 lacks the token; 13 lacks every other element when n > 1).  Strict: `changed` (11's
    removed flag, `Ids =/= Ids1`) and n_previous < n_current (a one-element threshold
    against 10, whose common cell is equal)."""
    ctx = _ctx()
    try:
        for p in _edges(n):
            b, V = _orset_var(ctx, n, p)
            one = n == 1
            assert b.read(plus(V, p, 1), False, 1) == (False, [10, 11, 13] if one else [10, 11])
            assert b.bind([(p, [(T(p, 1), False)])]) == [1]
            b, V = _orset_var(ctx, n, p)
            assert b.read(plus(V, p, 1), True, 2) == (False, [11])
            b.v.close()
            b, V = _orset_var(ctx, n, p)
            # {p: [a, b]} -> 10: no cell differs; strictly so only through the counts
            assert b.read(plus(st([p]), p, 1), True, 3) == (False, [11] if one else [10, 11])
            assert b.read(V, False, 4) == (True, [10, 12, 13] if one else [12])
            # (a one-element value equal to the strict threshold does not meet it)
            assert b.bind([(p, [(T(p, 1), False)])]) == ([] if one else [3])
            b.v.close()
    finally:
        ctx.close()


# G-Set bitmap words: the OR-Set shapes' word counts (2 n), and the same counts of words,
# whose odd ones end in half a unit
GSET_WORDS = sorted({w for n in (1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 2 * TILE + 1)
                     for w in (n, 2 * n)})


@pytest.mark.parametrize("words", GSET_WORDS)
def test_gset_shapes_single_bit_decides(words):
    """E = 64 * words elements known to the namespace (a replica holds them, so their slots
    are their ranks); the value lacks the edge elements: bits 0, 63, 64, the tile's edge,
    the last word's first and last.  Lazy thread 100 + i wants everything but edge i, 99
    wants everything: for the read of everything one bit decides each of them; for the
    read of everything but edge 0, that bit decides thread 100."""
    ctx = _ctx()
    try:
        n = 64 * words
        peer = ctx.var("gset")
        full = list(range(n))
        assert peer.write(tb(full)) == OK
        pos = sorted({0, 63, n - 64, n - 1} | {p for p in (64, 128 * TILE - 1, 128 * TILE) if p < n})
        V = [k for k in full if k not in pos]
        lacking = [[k for k in full if k != p] for p in pos]
        every = [100 + i for i in range(len(pos))]
        b = Both(ctx, "gset", var=peer.replica())
        b.bind(V)
        for i, th in enumerate(lacking):
            assert b.wait_needed(th, False, 100 + i) is False
        assert b.wait_needed(full, False, 99) is False
        assert b.read(V, False, 1) == (True, every + [99])     # met: they all stay
        assert b.read(full, False, 2) == (False, [99])
        assert b.read(lacking[0], True, 3) == (False, [])      # equal to 100: not strictly
        assert b.read(lacking[0], False, 4) == (False, [100])
        assert b.read(V, True, 5) == (False, every[1:])
        assert b.v.lazy() == []
        assert b.bind(pos[1:]) == [4, 5]       # the value equals 3's threshold: not strictly
        assert b.bind(pos[:1]) == [2, 3]
        assert b.v.waiters() == []
    finally:
        ctx.close()


# ---------------------------------------------------------------- wide namespaces

def test_wide_namespace():
    """An element of 65 tokens widens the namespace (cells of two {p, r} pairs): lazy threads
    registered before it (their cells are re-laid) and after it, reads strict and not."""
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        toks = sorted(T(k) for k in range(66))
        few = [(1, [(t, False) for t in toks[:5]]), (2, [(T(2), False)])]
        b.bind(few)
        assert b.wait_needed(plus(few, 2, 1), False, 10) is False       # narrow cells
        assert b.wait_needed(plus(few, 1, 9), False, 11) is False
        w0 = ctx.nif_stats()["namespaces_widened"]
        r = b.v.replica()
        assert r.write(tb([(1, [(t, False) for t in toks[:65]])])) == OK
        assert ctx.nif_stats()["namespaces_widened"] == w0 + 1
        many = [(1, [(t, False) for t in toks[:65]]), (2, [(T(2), False)])]
        only = [(1, [(t, False) for t in toks[:65]])]
        assert b.wait_needed(many, False, 12) is False                   # wide cells
        assert b.wait_needed([(1, [(t, k == 64) for k, t in enumerate(toks[:65])])], False, 13) is False
        assert b.wait_needed([(1, [(t, False) for t in toks])], False, 14) is False
        assert b.read(few, False, 1) == (True, [10, 11, 12])
        # the second pair of element 1's cell decides: 10 and 11 lack its tokens; 13 differs
        # from `only` in token 64's removed flag alone, 14 in token 65, 12 in element 2
        assert b.read(only, True, 3) == (False, [12, 13, 14])
        assert b.wait_needed(many, False, 15) is True                    # somebody reads
        assert b.read(few, True, 2) == (False, [10, 11])
        assert b.v.lazy() == []
        assert b.bind(many) == [3, 2]
        assert b.v.read() == (OK, tb(b.m.value))
    finally:
        ctx.close()


# ---------------------------------------------------------------- lazy threads per variable

def _lazy_var(ctx, nl):
    """100 elements; lazy thread j by j % 4: 0 equal to T = V + b on 50, 1 the same with b's
    removed flag set, 2 a superset of T, 3 lacks b on 50"""
    b = Both(ctx, "orset")
    b.bind(st(range(100)))
    V = b.m.value
    Tq = plus(V, 50, 1)
    for j in range(nl):
        th = [Tq, plus(V, 50, 1, removed=True), plus(Tq, 60 + j, 2), plus(V, 60 + j, 2)][j % 4]
        assert b.wait_needed(th, False, 1000 + j) is False
    return b, V, Tq


@pytest.mark.parametrize("nl", [0, 1, 3, 4, 5, 16, 17])
def test_lazy_thread_counts(nl):
    """0 .. 17 lazy threads: one and two chunks of 16 currents (the value is the first),
    every remainder of the unroll of 4.  violation, changed and n_previous < n_current each
    decide: 3 never fires for T; 0 fires unless strict; 1 and 2 always; a one-element
    strict threshold fires 0 by the element counts alone."""
    ctx = _ctx()
    try:
        ids = lambda ks: [1000 + j for j in range(nl) if j % 4 in ks]   # noqa: E731
        b, V, Tq = _lazy_var(ctx, nl)
        p0 = ctx.nif_stats()["device_passes"]
        assert b.read(Tq, False, 1, cap=32) == (False, ids((0, 1, 2)))
        if nl:                                  # (T's terms are known: the lazy threads hold them)
            assert ctx.nif_stats()["device_passes"] - p0 == 1   # decode and check: one pass
        assert [i for i, _ in b.v.lazy()] == ids((3,))
        b, V, Tq = _lazy_var(ctx, nl)
        assert b.read(Tq, True, 2, cap=32) == (False, ids((1, 2)))
        b, V, Tq = _lazy_var(ctx, nl)
        assert b.read(V, True, 3, cap=32) == (False, ids((0, 1, 2, 3)))
        b, V, Tq = _lazy_var(ctx, nl)
        assert b.read(plus(st([50]), 50, 1), True, 4, cap=32) == (False, ids((0, 1, 2)))
        assert b.read(V, False, 5, cap=32) == (True, ids((3,)))
        assert b.read(V, False, 6, cap=32) == (True, ids((3,)))  # met: the entries stayed
        assert b.bind(Tq) == [4]
        assert b.v.lazy() == []
    finally:
        ctx.close()


# ---------------------------------------------------------------- read_any

def _pool(ctx):
    """nine variables of their own namespaces, OR-Sets and G-Sets alternating, each with
    two lazy threads: 10 k wants one more element / token, 10 k + 1 two more"""
    out = []
    for k in range(9):
        if k % 2 == 0:
            b = Both(ctx, "orset")
            b.bind(st(range(3 + 40 * k), k))
            nxt = [plus(b.m.value, 0, 100 + k), plus(plus(b.m.value, 0, 100 + k), 1, 100 + k)]
        else:
            b = Both(ctx, "gset")
            b.bind(list(range(5 + 700 * k)))
            nxt = [wm.merge("gset", b.m.value, [-1]), wm.merge("gset", b.m.value, [-2, -1])]
        assert b.wait_needed(nxt[0], False, 10 * k) is False
        assert b.wait_needed(nxt[1], False, 10 * k + 1) is False
        b.nxt = nxt
        out.append(b)
    return out


def _read_any(pool, picks, rid):
    """picks: (variable index, threshold, strict); device against model, lists compared"""
    from lasp_amd import engine
    want = rm.read_any([(pool[k].m, th, s) for k, th, s in picks], rid)
    got = engine.read_any([(pool[k].v, tb(th), s) for k, th, s in picks], rid)
    assert got == want, (rid, got, want)
    for k in {k for k, _t, _s in picks}:
        pool[k].same_lists((rid, k))
    return want


@pytest.mark.parametrize("n,met_at", [(1, 0), (1, None), (2, 0), (2, 1), (2, None), (3, 1),
                                      (3, 2), (3, None), (17, 0), (17, 8), (17, 16), (17, None)])
def test_read_any_positions(n, met_at):
    """1, 2, 3 and 17 reads with the met read first, in the middle, last and absent; OR-Sets
    and G-Sets of different namespaces in one call; 17 reads name variables twice."""
    ctx = _ctx()
    try:
        pool = _pool(ctx)
        picks = []
        for i in range(n):
            k = i % 9
            b = pool[k]
            # unmet: the variable's first lazy threshold (fires 10 k, strictly 10 k + 1)
            picks.append((k, b.m.value if i == met_at else b.nxt[0], i % 3 == 2 and i != met_at))
        p0 = ctx.nif_stats()["device_passes"]
        found, fired = _read_any(pool, picks, 7000 + n)
        kinds = {pool[k].kind for k, _t, _s in picks}
        assert ctx.nif_stats()["device_passes"] - p0 == len(kinds)     # one pass per kind
        assert found == (-1 if met_at is None else met_at)
        assert any(fired[:1])
        # the waiters read_any left are served by the re-check
        for k in sorted({k for k, _t, _s in picks}):
            b = pool[k]
            nw = len(b.m.waiting)
            assert len(b.bind(b.nxt[1])) == nw
    finally:
        ctx.close()


def test_read_any_names_one_variable_twice():
    ctx = _ctx()
    try:
        pool = _pool(ctx)
        a = pool[0]
        picks = [(0, a.nxt[0], False), (1, pool[1].nxt[1], True), (0, a.nxt[1], False),
                 (0, a.m.value, False), (2, pool[2].m.value, False)]
        found, fired = _read_any(pool, picks, 5)
        assert (found, fired) == (3, [[0, 1], [], [], [], []])
        assert [w[0] for w in a.v.waiters()] == [5, 5] and a.v.lazy() == []
        assert pool[2].v.waiters() == [] and len(pool[2].v.lazy()) == 2
        assert a.bind(a.nxt[1]) == [5, 5]
    finally:
        ctx.close()


# ---------------------------------------------------------------- FALLBACK and errors

def test_fallback_and_errors():
    from lasp_amd import _lib, engine
    ctx, other = _ctx(), _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind(st(range(5)))
        V = b.m.value
        cnt = ctx.var("gcounter")
        # a counter: laspj_var_wait remains its read
        assert cnt.wait_needed(tb(3), False, 1) is None
        assert cnt.read(tb(3), False, 1) == (None, [])
        assert cnt.lazy() == [] and cnt.lazy_cancel(1) is False
        assert engine.read_any([(b.v, tb(plus(V, 0, 1)), False), (cnt, tb(3), False)], 9) == (None, [])
        b.same_lists()
        # strict wait_needed: met, or somebody reading -> at once; would register -> FALLBACK
        assert b.wait_needed(st([0]), True, 2) is True
        copy = Dv("orset")
        copy.value = V
        assert copy.wait_needed(V, True, 2) is False
        with pytest.raises(ReferenceRaises):
            copy.read(V, False, 3)                 # what the entry would have done (:798)
        f0 = ctx.nif_stats()["fallbacks"]
        assert b.v.wait_needed(tb(V), True, 2) is None
        assert ctx.nif_stats()["fallbacks"] == f0 + 1
        b.same_lists()
        assert b.read(plus(V, 0, 1), False, 3) == (False, [])
        assert b.wait_needed(V, True, 4) is True   # waiting_threads is non-empty (:739-741)
        assert b.bind(plus(V, 0, 1)) == [3]
        # cap too small: nothing changes, the count comes back
        V = b.m.value
        for j in range(3):
            assert b.wait_needed(plus(V, j, 2), False, 20 + j) is False
        ids, met, verd = (C.c_uint64 * 2)(), C.c_int32(), C.c_int32()
        nl, still = C.c_uint32(), C.c_uint32()
        img = tb(V)
        assert ctx.L.laspj_var_read(b.v.h, img, len(img), 1, 8, C.byref(met), ids, 2,
                                    C.byref(nl), C.byref(still), C.byref(verd)) == 0
        assert (verd.value, nl.value, still.value) == (OK, 3, 3)
        b.same_lists()                             # no waiter, three lazy threads
        assert b.read(V, True, 8, cap=2) == (False, [20, 21, 22])       # asks again with room
        assert b.v.cancel(8) is True
        b.m.waiting = []
        # read_any, the same: three fire in all, room for two
        for j in range(3):
            assert b.wait_needed(plus(V, j, 2), False, 30 + j) is False
        vs = (C.c_void_p * 1)(b.v.h.value)
        pv, nv, sv = (C.c_char_p * 1)(img), (C.c_uint64 * 1)(len(img)), (C.c_int32 * 1)(1)
        nls, found = (C.c_uint32 * 1)(), C.c_int32()
        assert ctx.L.laspj_var_read_any(ctx.h, 1, vs, pv, nv, sv, 8, C.byref(found), ids, 2, nls,
                                        C.byref(verd)) == 0
        assert (verd.value, nls[0], found.value) == (OK, 3, -1)
        b.same_lists()
        # a variable of another context
        o = other.var("orset")
        vs2 = (C.c_void_p * 2)(b.v.h.value, o.h.value)
        pv2, nv2 = (C.c_char_p * 2)(img, img), (C.c_uint64 * 2)(len(img), len(img))
        sv2, nl2 = (C.c_int32 * 2)(0, 0), (C.c_uint32 * 2)()
        assert ctx.L.laspj_var_read_any(ctx.h, 2, vs2, pv2, nv2, sv2, 8, C.byref(found), ids, 2,
                                        nl2, C.byref(verd)) == _lib.E_INVAL
        b.same_lists()
        # a host-held value (an element past 64 tokens whose token images differ in length)
        toks = sorted([T(k) for k in range(64)] + [T(64) + b"xy"])
        assert b.v.write(tb([(1, [(t, False) for t in toks])])) == FALLBACK and not b.v.resident
        assert b.v.lazy() == []                    # write/4 dropped them
        assert b.v.read(tb([]), False, 9) == (None, [])
        assert b.v.wait_needed(tb(V), False, 9) is None
        c = Both(ctx, "gset")
        assert engine.read_any([(c.v, tb([1]), False), (b.v, tb([]), False)], 9) == (None, [])
        assert c.v.waiters() == [] and b.v.waiters() == []
        # a threshold the namespace cannot represent (no ordset in term order)
        assert c.v.read(tb([5, 1]), False, 9) == (None, [])
        assert c.v.wait_needed(tb([5, 1]), False, 9) is None
        assert c.v.waiters() == [] and c.v.lazy() == []
    finally:
        other.close()
        ctx.close()


# ---------------------------------------------------------------- lifecycle

def test_lazy_list_follows_growth_and_reset():
    """lazy threads registered when the namespace had 10 element slots are read after it
    grew past two tiles (the slots they do not cover are absent), and across
    laspj_nif_reset (written out and decoded again beside the value)"""
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind(st(range(10)))
        V = b.m.value
        assert b.wait_needed(plus(V, 3, 1), False, 1) is False
        assert b.wait_needed(plus(V, 9, 1), False, 2) is False
        assert b.wait_needed(st(range(11)), False, 3) is False
        r = b.v.replica()
        assert r.bind(tb(st(range(2 * TILE + 20)))) == (OK, 1)          # the namespace grows
        assert b.read(plus(V, 3, 1), False, 10) == (False, [1])
        s0 = ctx.nif_stats()
        ctx.nif_reset()
        s1 = ctx.nif_stats()
        # b's value, its waiter, its two lazy thresholds, the replica
        assert s1["vars_spilled"] - s0["vars_spilled"] == 5
        b.same_lists()
        assert b.read(st(range(11)), True, 11) == (False, [])
        assert b.read(st(range(10)), True, 12) == (False, [2, 3])
        assert b.bind(st(range(11))) == [12]
        ctx.nif_reset()
        assert b.bind(plus(V, 3, 1)) == [10, 11]
        assert b.v.waiters() == []
    finally:
        ctx.close()


def test_written_calls_empty_the_lazy_list():
    """write/4 builds a fresh #dv (:842-843): a WRITTEN bind, UPDATE_OK, a WRITTEN union and
    filter run and laspj_var_etf_write drop the lazy threads; a NOOP bind keeps them"""
    ctx = _ctx()
    try:
        def fresh():
            b = Both(ctx, "orset")
            b.bind(st(range(6)))
            assert b.wait_needed(plus(b.m.value, 1, 1), False, 1) is False
            assert b.wait_needed(plus(b.m.value, 2, 1), False, 2) is False
            return b
        b = fresh()
        b.bind(b.m.value)                                   # Value0 =:= Value
        assert [i for i, _ in b.v.lazy()] == [1, 2]
        b.bind(plus(b.m.value, 5, 3))
        assert b.v.lazy() == []
        b = fresh()
        b.update((A("add"), 77))
        assert b.v.lazy() == []
        b = fresh()
        assert b.v.write(tb(st(range(3)))) == OK
        assert b.v.lazy() == []
        # union: out = l U r over replicas of one namespace
        b = fresh()
        l, r = b.v.replica(), b.v.replica()
        assert l.write(tb(b.m.value)) == OK and r.write(tb(b.m.value)) == OK
        assert b.v.union(l, r) == (OK, 0) and len(b.v.lazy()) == 2
        assert r.write(tb(st(range(7)))) == OK               # an element l does not hold
        assert b.v.union(l, r) == (OK, 1) and b.v.lazy() == []
        # a filter process writing into out
        b = fresh()
        src = b.v.replica()
        assert src.write(tb(plus(b.m.value, 4, 8))) == OK
        f = ctx.filter(src, b.v)
        verd, status, pend = f.step(lambda _x: True)
        assert (verd, status, pend) == (OK, 1, 0) and b.v.lazy() == []
        f.close()
        # a G-Set intersection writing into out
        g = Both(ctx, "gset")
        g.bind([1, 2])
        assert g.wait_needed([1, 2, 3], False, 1) is False
        gl, gr = g.v.replica(), g.v.replica()
        assert gl.write(tb([1, 2, 3, 4])) == OK and gr.write(tb([3, 4, 5])) == OK
        assert g.v.intersection(gl, gr) == (OK, 1) and g.v.lazy() == []
    finally:
        ctx.close()


def test_destroy_with_live_lazy_threads():
    ctx = _ctx()
    b = Both(ctx, "orset")
    c = Both(ctx, "gset")
    b.bind(st([1]))
    assert b.wait_needed(st([1, 2]), False, 1) is False
    assert b.read(st([2]), False, 2) == (False, [1])
    assert b.wait_needed(st([1, 3]), False, 3) is True
    b.m.waiting, _ = [], b.v.cancel(2)
    assert b.wait_needed(st([1, 3]), False, 3) is False
    assert c.wait_needed([4], False, 1) is False
    assert b.v.lazy_cancel(12345) is False
    b.v.close()                     # the variable first, with its lazy threads
    ctx.close()                     # then the context, with c's
    c.v.close()


# ---------------------------------------------------------------- equivalence

@pytest.mark.parametrize("kind", ["orset", "gset"])
def test_read_equals_wait_without_lazy_threads(kind):
    """twin variables, one read through laspj_var_read and one through laspj_var_wait: the
    same met, verdict and waiter list after every call, and the same re-check"""
    ctx = _ctx()
    try:
        a, w = ctx.var(kind), ctx.var(kind)
        if kind == "orset":
            V = st(range(70))
            ths = [[], V, V[:3], plus(V, 69, 1), plus(V[:2], 0, 1, removed=True), st([500]),
                   [(0, [(T(0), True)])], st(range(69)), plus(V, 0, 5)]
            more = plus(plus(V, 69, 1), 0, 5)
        else:
            V = list(range(200))
            ths = [[], V, V[:3], V + [900], [901], V[5:], [A("x")], V + [A("x")]]
            more = V + [900, A("x")]
        wid = 0
        for value in ([], V):
            if value:
                assert a.bind(tb(value)) == w.bind(tb(value)) == (OK, 1)
            for th in ths:
                for strict in (False, True):
                    wid += 1
                    verd, met = w.wait(tb(th), strict, wid)
                    assert a.read(tb(th), strict, wid) == ((met if verd == OK else None), [])
                    assert a.waiters() == w.waiters(), (wid, strict)
            assert a.recheck(cap=64) == w.recheck(cap=64)
        assert a.bind(tb(more)) == w.bind(tb(more)) == (OK, 1)
        got = a.recheck(cap=64)
        assert got == w.recheck(cap=64) and got[1]
        assert a.waiters() == w.waiters()
    finally:
        ctx.close()
