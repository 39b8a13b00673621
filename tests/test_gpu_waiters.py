"""Device-resident waiters (include/laspj.h: laspj_var_wait / _recheck / _recheck_many /
_wait_cancel / _waiter_count / _waiter_at; lasp_amd/csrc/laspj_nif_waiters.hip k_waiter_check)
against the reference model of read/6 and reply_to_all/3 (lasp_core.erl:331-364, 765-825)
in tests/waiters_model.py.  Oracle values are kept as tests/test_gpu_nif_update.py keeps
them: oorset.update replayed with the device-minted tokens, oorset.merge for binds.

The kernel's wave tile is kWaitTile = 128 16-byte units of the value: 128 element slots of
a narrow OR-Set (one {p, r} pair each), 128 x 128 = 16384 elements of a G-Set (two bitmap
words each); a wave takes kWaitChunk = 16 waiters, so 64 / 65 waiters are four chunks / four
and one.
"""

import pytest

from oracle import orset as oorset
from oracle.terms import Atom, exact_eq

import waiters_model as wm
from waiters_model import FALLBACK, OK, tb

A = Atom
pytestmark = pytest.mark.gpu
TILE = 128            # kWaitTile (laspj_nif_waiters.hip)


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def T(k, salt=0):
    return bytes([salt]) + k.to_bytes(4, "big") + b"\x55" * 15


class Both:
    """a resident variable and the model of its value and waiting_threads, kept in step;
    every answer of the device is asserted against the model's"""

    def __init__(self, ctx, kind, var=None):
        self.kind, self.ctx = kind, ctx
        self.v = var if var is not None else ctx.var(kind)
        self.m = wm.ReplyModel(kind)

    def wait(self, th, strict, wid):
        met = self.m.wait(th, strict, wid)
        assert self.v.wait(tb(th), strict, wid) == (OK, met), (wid, strict)
        return met

    def bind(self, state):
        noop = exact_eq(state, self.m.value)
        assert self.v.bind(tb(state)) == (OK, 0 if noop else 1)
        self.m.value = wm.merge(self.kind, self.m.value, state)

    def update(self, op):
        verd, res, _err, minted = self.v.update(tb(op))
        want = wm.oracle_update(self.kind, op, self.m.value, minted)
        assert (verd, res) == (OK, 0 if want[0] == "ok" else 1), op
        if want[0] == "ok":
            self.m.value = want[1]

    def recheck(self):
        fired, _flags = self.m.write()
        assert self.v.recheck() == (OK, fired, len(self.m.waiting))
        assert self.v.waiters() == self.m.listing()
        return fired


@pytest.mark.parametrize("kind", ["orset", "gset"])
def test_random_scenario_matches_reply_to_all(kind):
    """300 random steps (tests/waiters_model.py, the seed whose run the CPU test shows is
    not vacuous): after every WRITTEN / UPDATE_OK laspj_var_recheck answers the model's ids
    in the model's order, the waiters left are the model's, wait's met is threshold_met;
    one device pass per re-check with waiters and none without; no reset, no FALLBACK."""
    ctx = _ctx()
    try:
        var = ctx.var(kind)
        s = wm.Scenario(wm.SEEDS[kind], kind, dev=var,
                        passes=lambda: ctx.nif_stats()["device_passes"]).run(300)
        c = s.counts
        assert all(cls[False] > 0 and cls[True] > 0 for cls in c.values()), c
        assert s.empty_rechecks >= 1 and s.rechecks > s.empty_rechecks
        st = ctx.nif_stats()
        assert st["dict_resets"] == 0 and st["fallbacks"] == 0
    finally:
        ctx.close()


def test_strict_waiter_fires_on_removal_only():
    """A {strict, Cur} waiter does not fire on a no-op bind and fires on {remove, E}: the
    ids differ by their removed flag (`Ids =/= Ids1`, lasp_lattice.erl:235-253); the
    non-strict waiter for the same state was met at registration (:153-161)."""
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind([(k, [(T(k), False)]) for k in range(5)])
        cur = b.m.value
        assert b.wait(cur, False, 1) is True
        assert b.wait(cur, True, 2) is False
        b.bind(cur)                                   # Value0 =:= Value
        assert b.recheck() == []
        b.update((A("remove"), 3))
        assert b.recheck() == [2]
        assert b.v.waiters() == []
    finally:
        ctx.close()


def _edges(n):
    return sorted({0, n - 1} | {p for t in (1, 2, 3) for p in (t * TILE - 1, t * TILE) if p < n})


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1])
def test_orset_shapes_single_cell_decides(n):
    """n elements; the only violating cell (a threshold token the value lacks) and the only
    changed cell (a {strict, Cur} waiter) sit first, last, or on a tile edge."""
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind([(k, [(T(k), False)]) for k in range(n)])
        assert b.recheck() == []
        pos = _edges(n)
        for i, p in enumerate(pos):
            th = oorset.merge(b.m.value, [(p, [(T(p, 1), False)])])
            assert b.wait(th, False, 100 + i) is False
        assert b.wait(b.m.value, True, 99) is False
        for i, p in enumerate(pos):
            b.bind([(p, [(T(p, 1), False)])])
            assert b.recheck() == [100 + i, 99]
            assert b.wait(b.m.value, True, 99) is False
        assert [w[0] for w in b.v.waiters()] == [99]
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, TILE - 1, TILE, TILE + 1, 3 * TILE + 1,
                               TILE * TILE])
def test_gset_shapes_single_bit_decides(n):
    """The same for G-Sets (words of 64 elements, units of 128, a tile of 16384): the
    elements at the edges are known to the namespace (a replica holds them, so their slots
    are their ranks) and missing from the value; each arrives alone."""
    ctx = _ctx()
    try:
        peer = ctx.var("gset")
        full = list(range(n))
        assert peer.write(tb(full)) == OK
        pos = sorted(set(_edges(n)) | {p for p in (63, 64) if p < n})
        b = Both(ctx, "gset", var=peer.replica())
        if len(pos) < n:
            b.bind([k for k in full if k not in pos])
        assert b.recheck() == []
        for i, p in enumerate(pos):
            assert b.wait(wm.merge("gset", b.m.value, [p]), False, 100 + i) is False
        assert b.wait(b.m.value, True, 99) is False
        for i, p in enumerate(pos):
            b.bind([p])
            assert b.recheck() == [100 + i, 99]
            assert b.wait(b.m.value, True, 99) is False
        assert b.v.read() == (OK, tb(full))
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", ["orset", "gset"])
def test_new_value_and_grown_namespace(kind):
    """new() with a {strict, []} waiter; a [] threshold is met at once; a waiter registered
    when the namespace had 10 elements is re-checked after it grew past three tiles (an
    OR-Set's; a G-Set's 6144 elements are 48 units of its one tile) — the slots it does
    not cover are absent."""
    ctx = _ctx()
    try:
        b = Both(ctx, kind)
        assert b.wait([], False, 1) is True
        assert b.wait([], True, 2) is False
        assert b.recheck() == []
        st = (lambda ks, s=0: [(k, [(T(k, s), False)]) for k in ks]) if kind == "orset" else \
            (lambda ks, s=0: list(ks))
        b.bind(st(range(10)))
        assert b.recheck() == [2]
        later = st([3], 1) if kind == "orset" else [9000]
        assert b.wait(wm.merge(kind, b.m.value, later), False, 3) is False
        assert b.wait(b.m.value, True, 4) is False
        n = 3 * TILE + 20 if kind == "orset" else 3 * TILE * TILE // 8
        b.bind(st(range(10, n)))
        assert b.recheck() == [4]
        b.bind(later)
        assert b.recheck() == [3]
    finally:
        ctx.close()


@pytest.mark.parametrize("nw", [0, 1, 64, 65])
def test_waiter_counts_on_one_variable(nw):
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind([(k, [(T(k), False)]) for k in range(100)])
        for w in range(nw):
            th = oorset.merge(b.m.value[:w % 7], [(w, [(T(w, 1 + w % 3), False)])])
            assert b.wait(th, w % 2 == 1, w) is False
        b.bind([(w, [(T(w, 1), False)]) for w in range(100)])
        p0 = ctx.nif_stats()["device_passes"]
        fired = b.recheck()
        assert fired == [w for w in range(nw) if w % 3 == 0]
        # (NifVar.recheck starts with room for 16 ids and asks once more when more are met)
        want = 0 if not nw else 2 if len(fired) > 16 else 1
        assert ctx.nif_stats()["device_passes"] - p0 == want
        b.bind([(w, [(T(w, 2), False), (T(w, 3), False)]) for w in range(100)])
        assert b.recheck() == [w for w in range(nw) if w % 3 != 0]
    finally:
        ctx.close()


def test_wide_namespace():
    """70 adds of one element across two replicas widen the namespace (cells of k {p, r}
    pairs); waiters registered before and after it, strict and not."""
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        r = Both(ctx, "orset", var=b.v.replica())
        for _ in range(5):
            b.update((A("add"), 1))
            r.update((A("add"), 1))
        b.update((A("add"), 2))
        w0 = ctx.nif_stats()["namespaces_widened"]
        assert b.wait(r.m.value, False, 1) is False           # the replica's tokens
        assert b.wait(b.m.value, True, 2) is False
        assert b.wait(wm.merge("orset", b.m.value, r.m.value), True, 3) is False
        for _ in range(30):
            b.update((A("add"), 1))
            r.update((A("add"), 1))
        assert ctx.nif_stats()["namespaces_widened"] == w0 + 1
        assert b.recheck() == [2]
        assert b.wait(r.m.value, False, 4) is False
        assert b.wait(b.m.value, True, 5) is False
        assert b.wait(b.m.value[:1], False, 6) is True
        b.bind(r.m.value)
        assert b.recheck() == [1, 3, 4, 5]
        assert b.wait(b.m.value, True, 7) is False
        b.update((A("remove"), 1))
        assert b.recheck() == [7]
        assert b.v.read() == (OK, tb(b.m.value))
    finally:
        ctx.close()


def _prepare_set(ctx):
    """8 variables of different sizes; [1] and [6] have no waiters, [0] holds new()"""
    sizes = [0, 1, 5, 64, 130, 300, 40, 7]
    out = []
    for i, n in enumerate(sizes):
        b = Both(ctx, "orset")
        if n:
            b.bind([(k, [(T(k, i), False)]) for k in range(n)])
        if i not in (1, 6):
            assert b.wait(b.m.value, True, 10 * i) is False
            assert b.wait([(0, [(T(0, 100 + i), False)])], False, 10 * i + 1) is False
            assert b.wait([(n, [(T(n, i), False)])], i % 2 == 0, 10 * i + 2) is False
        out.append(b)
    return out, sizes


def test_recheck_many_equals_recheck_per_variable():
    ctx = _ctx()
    try:
        sa, sizes = _prepare_set(ctx)
        sb, _ = _prepare_set(ctx)
        for bs in (sa, sb):
            pairs, states = [], []
            for i, b in enumerate(bs):
                # written: [0] (from new()), [2], [4], [5], [6]; no-ops: the others
                st = [(sizes[i], [(T(sizes[i], i), False)])] if i in (0, 2, 4, 5, 6) else b.m.value
                states.append(st)
                pairs.append((b.v, tb(st)))
            want = [(OK, 0 if exact_eq(st, b.m.value) else 1) for st, b in zip(states, bs)]
            assert ctx.var_bind_many(pairs) == want
            for st, b in zip(states, bs):
                b.m.value = wm.merge("orset", b.m.value, st)
        p0 = ctx.nif_stats()["device_passes"]
        got = ctx.var_recheck_many([b.v for b in sa], cap=64)
        assert ctx.nif_stats()["device_passes"] - p0 == 1
        model = [b.m.write()[0] for b in sa]
        assert got == [(OK, ids) for ids in model]
        assert [bool(ids) for _v, ids in got] == [True, False, True, False, True, True, False,
                                                   False]
        assert got[2] == (OK, [20, 22])
        assert [b.v.waiters() for b in sa] == [b.m.listing() for b in sa]
        assert [b.recheck() for b in sb] == model
        # too little room: nothing is removed, the count says how much to come back with
        assert sa[3].wait(sa[3].m.value, False, 77) is True
        import ctypes as C
        vs = (C.c_void_p * 2)(sa[0].v.h.value, sa[3].v.h.value)
        for b in (sa[0], sa[3]):
            b.update((A("add"), 1))
        ids, nmet, verd = (C.c_uint64 * 1)(), (C.c_uint32 * 2)(), (C.c_int32 * 2)()
        assert ctx.L.laspj_var_recheck_many(ctx.h, 2, vs, ids, 1, nmet, verd) == 0
        assert list(nmet) == [1, 1] and list(verd) == [OK, OK]
        assert sa[3].v.waiters() == sa[3].m.listing() and sa[0].v.waiters() == sa[0].m.listing()
        assert sa[3].recheck() == [30] and sa[0].recheck() == [2]
    finally:
        ctx.close()


def test_waiters_survive_reset():
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind([(k, [(T(k), False)]) for k in range(200)])
        assert b.wait(oorset.merge(b.m.value, [(7, [(T(7, 1), False)])]), False, 1) is False
        assert b.wait(b.m.value, True, 2) is False
        assert b.wait([(999, [(T(999), False)])], False, 3) is False
        s0 = ctx.nif_stats()
        ctx.nif_reset()
        s1 = ctx.nif_stats()
        assert s1["vars_spilled"] - s0["vars_spilled"] == 4       # the value, three thresholds
        assert b.v.waiters() == b.m.listing()
        assert b.recheck() == []
        assert ctx.nif_stats()["vars_hydrated"] - s1["vars_hydrated"] == 4
        b.bind([(7, [(T(7, 1), False)])])
        assert b.recheck() == [1, 2]
        ctx.nif_reset()
        b.bind([(999, [(T(999), False)])])
        assert b.recheck() == [3]
    finally:
        ctx.close()


def test_host_held_value_answers_fallback_and_keeps_waiters():
    ctx = _ctx()
    try:
        b = Both(ctx, "orset")
        b.bind([(2, [(T(2), False)])])
        assert b.wait([(1, [(T(0), False)])], False, 1) is False
        assert b.wait([(5, [(T(5), False)])], False, 2) is False
        assert b.wait([(1, [(T(0), False)]), (2, [(T(2), False)])], True, 3) is False
        assert b.v.cancel(12345) is False
        # an element past 64 tokens whose token images differ in length: held on the host
        toks = sorted([T(k) for k in range(64)] + [T(64) + b"xy"])
        big = [(1, [(t, False) for t in toks])]
        assert b.v.write(tb(big)) == FALLBACK and not b.v.resident
        assert b.v.wait(tb([]), False, 9) == (FALLBACK, None)
        assert b.v.recheck() == (FALLBACK, [], 3)
        assert b.v.waiters() == b.m.listing()
        small = [(1, [(T(0), True)]), (2, [(T(2), False)])]
        assert b.v.write(tb(small)) == OK
        b.m.value = small
        assert b.recheck() == [1, 3]
        assert b.v.cancel(2) is True and b.v.waiters() == []
    finally:
        ctx.close()


def test_destroy_with_live_waiters():
    ctx = _ctx()
    b = Both(ctx, "orset")
    c = Both(ctx, "gset")
    b.bind([(1, [(T(1), False)])])
    assert b.wait([(2, [(T(2), False)])], False, 1) is False
    assert b.wait(b.m.value, True, 2) is False
    assert c.wait([4], False, 1) is False
    b.v.close()                     # the variable first, with its waiters
    ctx.close()                     # then the context, with c's
    c.v.close()
