"""riak_dt_gcounter variables resident on the device (include/laspj.h: LASPJ_KIND_GCOUNTER
through laspj_var_*; lasp_amd/csrc/laspj_counters.hip) against tests/counters_model.py:
oracle/core.py's _GCounter for values, oracle.lattice.threshold_met for thresholds,
reply_to_all (lasp_core.erl:765-825) for the waiting list.

The kernels' widths (laspj_counters.hip): one wave of LANES = 64 lanes per variable; a row
is summed S = 128 slots per iteration (two counts per lane); an image's pairs are gathered 64
per iteration; V = 4 variables per 256-thread block; W = 64 waiters per ballot step (one
mask word).  k_gc_incr gives one variable a whole block: 4 x S slots per iteration and
four ballot steps side by side, so 4 W + 1 waiters wrap it once.  A row starts at ROW0 = 64
slots and doubles.

Thresholds through threshold / wait: a refused *value* image passed as a threshold is a list
or an atom, which lasp_lattice.erl:87-90 compares as a term above every number: never met,
and a waiter on it is kept and never fires (the issue's own rule for non-numbers); only an
image that is no term at all (truncated) answers FALLBACK there.  FALLBACK for threshold /
wait over a refused value is checked on a variable that holds one (written, host-held).
"""

import ctypes as C
import random

import pytest

import counters_model as cm
from counters_model import A, FALLBACK, M64, NOOP, OK, WRITTEN, tb
from lasp_amd import _lib
from lasp_amd import gcounter as dg
from oracle import lattice as olat

pytestmark = pytest.mark.gpu
LANES, S, V, W, ROW0 = 64, 128, 4, 64, 64


@pytest.fixture()
def ctx():
    from lasp_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


def fires(th, strict):
    """a waiter a kernel can fire (plan T): the others are decided on the host"""
    return dg.threshold_plan(th, strict)[1] is not None


class Rep:
    """a counter variable and its model in step: every device answer is asserted against
    the model's, and every call against the device passes it may take"""

    def __init__(self, ctx, var=None):
        self.ctx = ctx
        self.v = var if var is not None else ctx.var("gcounter")
        self.m = cm.CounterModel()
        self.row = False          # a pass has given the variable its row
        self.checked = True       # the waiters were checked against the current value

    def replica(self):
        return Rep(self.ctx, self.v.replica())

    def _passes(self):
        return self.ctx.nif_stats()["device_passes"]

    def _expect(self, p0, n):
        assert self._passes() - p0 == n, (self._passes() - p0, n)

    def live(self):
        return any(fires(th, s) for _i, s, th in self.m.waiting)

    def increment(self, op, actor, fused):
        p0 = self._passes()
        self.m.increment(op, actor)
        if fused:
            fired = self.m.reply()
            assert self.v.increment(tb(op), tb(actor), cap=16) == (OK, fired, len(self.m.waiting))
            self.checked = True
        else:
            assert self.v.increment(tb(op), tb(actor)) == (OK,)
            self.checked = False
            fired = None
        self.row = True
        self._expect(p0, 1)
        return fired

    def bind(self, c):
        p0 = self._passes()
        st = self.m.bind(c)
        assert self.v.bind(tb(c)) == (OK, st)
        self.row = self.checked = True
        self._expect(p0, 1)
        return st

    def write(self, c):
        p0 = self._passes()
        self.m.value = list(c)
        assert self.v.write(tb(c)) == OK
        self.row, self.checked = True, False
        self._expect(p0, 1)

    def recheck(self, cap=16):
        p0 = self._passes()
        need = 0 if self.checked or not self.live() else 1
        fired = self.m.reply()
        assert self.v.recheck(cap) == (OK, fired, len(self.m.waiting))
        self.checked = True
        self.row = self.row or bool(need)
        self._expect(p0, need)
        return fired

    def wait(self, th, strict, wid):
        p0 = self._passes()
        met = self.m.wait(th, strict, wid)
        assert self.v.wait(tb(th), strict, wid) == (OK, met), (th, strict)
        if fires(th, strict):
            self.row = self.checked = True
        self._expect(p0, 1 if fires(th, strict) else 0)
        return met

    def cancel(self, wid):
        found = self.m.cancel(wid)
        assert self.v.cancel(wid) == found
        return found

    def check(self):
        p0 = self._passes()
        assert self.v.read() == (OK, tb(self.m.value))
        self._expect(p0, 1 if self.row else 0)
        assert self.v.value() == (OK, tb(cm.total(self.m.value)))
        self.row = self.checked = True
        assert self.v.waiters() == self.m.listing()
        assert self.v.resident


def test_random_ad_counter_scenario(ctx):
    """300 steps over 3 replicas of one counter and 5 actors: increment (both op forms, with
    and without the fused re-check), bind of another replica's read, wait, cancel, write."""
    rng = random.Random(20260)
    base = Rep(ctx)
    reps = [base, base.replica(), base.replica()]
    actors = [A("c1"), A("c2"), 7, b"client", (1, A("n"))]
    seen = {k: set() for k in ("fused", "plain", "op", "bind", "wait", "cancel", "write")}
    wid = 0
    for step in range(300):
        r = rng.choice(reps)
        kind = rng.choice(["incr", "incr", "incr", "bind", "bind", "wait", "wait", "cancel",
                           "write"])
        if kind == "incr":
            op = A("increment") if rng.random() < 0.5 else (A("increment"), rng.randint(1, 3))
            seen["op"].add(isinstance(op, tuple))
            if rng.random() < 0.6:
                seen["fused"].add(bool(r.increment(op, rng.choice(actors), True)))
            else:
                r.increment(op, rng.choice(actors), False)
                seen["plain"].add(bool(r.recheck()) if rng.random() < 0.7 else None)
        elif kind == "bind":
            o = rng.choice(reps)
            verd, img = o.v.read()
            assert (verd, img) == (OK, tb(o.m.value))
            seen["bind"].add(r.bind(o.m.value))
            r.recheck()
        elif kind == "wait":
            sm = cm.total(r.m.value)
            th = rng.choice([sm - 1, sm, sm + 1, sm + 2, sm + 4, sm + 2.5, 0, -1, [],
                             sm + 6, float(sm + 3)])
            wid += 1
            seen["wait"].add(r.wait(th, rng.random() < 0.4, wid))
        elif kind == "cancel":
            ids = [w[0] for w in r.m.waiting]
            seen["cancel"].add(r.cancel(rng.choice(ids) if ids and rng.random() < 0.7 else 9999))
        else:
            o = rng.choice(reps)
            r.write(o.m.value)
            seen["write"].add(bool(r.recheck()))
        if step % 25 == 0:
            for x in reps:
                x.check()
    for x in reps:
        x.check()
    assert seen["fused"] == {True, False} and seen["plain"] >= {True, False}, seen
    assert seen["op"] == {True, False} and seen["bind"] == {NOOP, WRITTEN}, seen
    assert seen["wait"] == {True, False} and seen["cancel"] == {True, False}, seen
    assert seen["write"] == {True, False}, seen
    st = ctx.nif_stats()
    assert st["fallbacks"] == 0 and st["dict_elements"] == len(actors)


def counter(n, base=1):
    return [(k, base + k) for k in range(n)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, S - 1, S, S + 1, 3 * S + 1])
def test_row_shapes(ctx, n):
    """`=:=` and the max over rows around the pair step (64) and the row step S: the only
    pair that differs first, last or on a step edge; one actor more or fewer; a sum that only
    the last slot completes."""
    r = Rep(ctx)
    # (odd actors first: slots are not in term order)
    if n > 1:
        assert r.bind([p for p in counter(n) if p[0] % 2]) == WRITTEN
    assert r.bind(counter(n)) == WRITTEN
    assert r.bind(counter(n)) == NOOP
    edges = sorted({0, n - 1} | {e for e in (63, 64, 65, S - 1, S, S + 1, 2 * S, 3 * S) if e < n})
    for e in edges:
        lower = [(a, c - 1 if a == e and c > 1 else c) for a, c in r.m.value]
        if lower != r.m.value:
            # not =:=, though the max leaves the row as it was: written, as the reference
            before = list(r.m.value)
            assert r.bind(lower) == WRITTEN and r.m.value == before
        higher = [(a, c + 5 if a == e else c) for a, c in r.m.value]
        assert r.bind(higher) == WRITTEN
        assert r.bind(higher) == NOOP
    r.check()
    # one actor fewer (the rest equal), one more
    assert r.bind(r.m.value[:-1]) == WRITTEN
    assert r.bind(r.m.value[1:]) == WRITTEN
    assert r.bind(r.m.value + [(n, 1 << 40)]) == WRITTEN
    assert r.bind(r.m.value) == NOOP
    r.check()
    # the last slot (2^40) completes the sum
    tot = cm.total(r.m.value)
    assert r.v.threshold(tb(tot)) == (OK, True)
    assert r.v.threshold(tb(tot - 1), True) == (OK, True)
    assert r.v.threshold(tb(tot), True) == (OK, False)
    assert r.v.threshold(tb(tot - (1 << 40) + 1)) == (OK, True)
    assert r.v.threshold(tb(tot + 1)) == (OK, False)


def test_growth_past_each_doubling(ctx):
    """actors arrive one per call past ROW0 and 2 ROW0; a replica stays small until an image
    names a late actor; earlier counts survive every copy"""
    a = Rep(ctx)
    b = a.replica()
    b.bind(counter(3, 100))
    for k in range(2 * ROW0 + 3):
        if k % 2:
            a.increment((A("increment"), k + 1), k, fused=False)
        else:
            a.bind(a.m.value + [(k, k + 1)] if k else [(0, 1)])
        if k in (ROW0 - 1, ROW0, ROW0 + 1, 2 * ROW0 - 1, 2 * ROW0, 2 * ROW0 + 1):
            a.check()
            b.check()           # (its row is shorter than its namespace)
    assert a.m.value[0] == (0, 1) and len(a.m.value) == 2 * ROW0 + 3
    a.check()
    # the replica goes from ROW0 slots straight past two doublings
    assert b.bind([(2 * ROW0 + 2, 9)]) == WRITTEN
    b.check()
    assert b.bind(a.m.value) == WRITTEN
    assert b.m.value[:3] == [(0, 100), (1, 101), (2, 102)]
    b.check()
    assert ctx.nif_stats()["fallbacks"] == 0


@pytest.mark.parametrize("n", [1, 2, V - 1, V, V + 1, 65])
def test_bind_many_is_one_pass(ctx, n):
    """n counters of mixed row lengths (1 and 3 S + 1 side by side), namespaces, waiters and
    outcomes in one launch; every status and fired id is the model's"""
    base = Rep(ctx)
    reps, binds = [], []
    for i in range(n):
        r = base.replica() if i % 3 == 1 else Rep(ctx)
        big = i % 4 == 1 or (n == 1)
        state = counter(3 * S + 1) if big and i < 6 else [(A("x"), i + 1)]
        r.bind(state)
        if i % 2 == 0:
            tot = cm.total(state)
            for j, th in enumerate([tot + 1, tot + 50, tot + 2.5, []]):
                r.wait(th, j % 2 == 1, 1000 * i + j)
        if i % 3 == 0:
            img = list(state)                                   # NOOP
        elif big and i < 6:
            img = state[:-1] + [(3 * S, state[-1][1] + 7)]      # the last slot alone moves
        else:
            img = [(A("x"), i + 3), (A("y"), 1)]
        reps.append(r)
        binds.append(img)
    p0 = ctx.nif_stats()["device_passes"]
    got = ctx.var_bind_many([(r.v, tb(img)) for r, img in zip(reps, binds)])
    assert got == [(OK, r.m.bind(img)) for r, img in zip(reps, binds)]
    assert ctx.nif_stats()["device_passes"] - p0 == 1
    assert {s for _v, s in got} == ({NOOP} if n == 1 else {NOOP, WRITTEN})
    # the re-check is answered from that pass
    fired = ctx.var_recheck_many([r.v for r in reps], cap=4)
    assert fired == [(OK, r.m.reply()) for r in reps]
    assert ctx.nif_stats()["device_passes"] - p0 == 1
    assert n < 3 or any(f for _v, f in fired)
    for r in reps[:6]:
        r.row = r.checked = True
        r.check()


def test_bind_many_refuses_a_set_beside_counters(ctx):
    a, b = Rep(ctx), Rep(ctx)
    a.bind(counter(2))
    o = ctx.var("orset")
    with pytest.raises(_lib.LaspjError) as e:
        ctx.var_bind_many([(a.v, tb(counter(3))), (o, tb([])), (b.v, tb(counter(1)))])
    assert e.value.status == _lib.E_KIND
    a.check()
    b.check()
    assert o.read() == (OK, tb([]))


def met_pattern(k, pattern):
    if pattern == "first":
        return [i == 0 for i in range(k)]
    if pattern == "last":
        return [i == k - 1 for i in range(k)]
    if pattern == "alternating":
        return [i % 2 == 0 for i in range(k)]
    return [True] * k


@pytest.mark.parametrize("pattern", ["first", "last", "alternating", "all"])
@pytest.mark.parametrize("k", [0, 1, W - 1, W, W + 1, 4 * W + 1])
def test_waiter_counts(ctx, k, pattern):
    """k waiters around the ballot step, the met ones first, last, alternating and all, fired
    by the fused increment (a block: four steps side by side) and by the re-check (a wave)"""
    for fused in (True, False):
        r = Rep(ctx)
        r.bind([(A("a"), 10)])
        met = met_pattern(k, pattern)
        for i in range(k):
            assert r.wait(11 if met[i] else 1000 + i, i % 3 == 0 and not met[i], i + 1) is False
        never = r.wait([], False, 5000)                       # kept, never fires
        assert never is False
        p0 = ctx.nif_stats()["device_passes"]
        if fused:
            r.m.increment(A("increment"), A("b"))
            want = r.m.reply()
            assert r.v.increment(tb(A("increment")), tb(A("b")), cap=k + 1) == \
                (OK, want, len(r.m.waiting))
        else:
            r.increment(A("increment"), A("b"), fused=False)
            want = [i + 1 for i in range(k) if met[i]]
            if len(want) > 1:
                # too little room: the count needed, and nothing removed
                ids = (C.c_uint64 * len(want))()
                nmet, left, verd = C.c_uint32(), C.c_uint32(), C.c_int32()
                assert ctx.L.laspj_var_recheck(r.v.h, ids, len(want) - 1, C.byref(nmet),
                                               C.byref(left), C.byref(verd)) == 0
                assert (nmet.value, left.value, verd.value) == (len(want), k + 1, OK)
                assert r.v.waiters() == r.m.listing()
                r.checked = True
            assert r.recheck(cap=max(len(want), 1)) == want
        assert want == [i + 1 for i in range(k) if met[i]]
        assert ctx.nif_stats()["device_passes"] - p0 == (1 if fused or not k else 2)
        assert r.v.waiters() == r.m.listing() and r.m.waiting[-1][0] == 5000


def test_fused_increment_with_little_room(ctx):
    """more met than cap: the increment is applied once, nothing is removed, nmet says how
    much room to come back with"""
    r = Rep(ctx)
    for i in range(5):
        r.wait(1, False, i + 1)
    ids = (C.c_uint64 * 2)()
    nmet, left, verd = C.c_uint32(), C.c_uint32(), C.c_int32()
    op, actor = tb(A("increment")), tb(A("a"))
    assert ctx.L.laspj_var_etf_increment(r.v.h, op, len(op), actor, len(actor), ids, 2,
                                         C.byref(nmet), C.byref(left), C.byref(verd)) == 0
    assert (nmet.value, left.value, verd.value) == (5, 5, OK)
    r.m.increment(A("increment"), A("a"))
    r.row = True
    assert r.recheck(cap=5) == [1, 2, 3, 4, 5]
    r.check()


def test_recheck_many_over_counters_and_a_set(ctx):
    a, b = Rep(ctx), Rep(ctx)
    o = ctx.var("orset")
    assert o.update(tb((A("add"), 1)))[:2] == (OK, 0)
    seen = o.read()[1]
    assert o.wait(seen, True, 77) == (OK, False)              # a strict inflation of it
    a.wait(2, False, 1)
    a.wait(9, False, 2)
    b.wait(1, True, 3)
    a.increment((A("increment"), 2), A("x"), fused=False)
    b.increment((A("increment"), 2), A("x"), fused=False)
    assert o.update(tb((A("add"), 2)))[:2] == (OK, 0)
    # too little room over all of them: nothing leaves, on either side
    vs = (C.c_void_p * 3)(a.v.h.value, o.h.value, b.v.h.value)
    ids, nmet, verd = (C.c_uint64 * 4)(), (C.c_uint32 * 3)(), (C.c_int32 * 3)()
    assert ctx.L.laspj_var_recheck_many(ctx.h, 3, vs, ids, 2, nmet, verd) == 0
    assert list(nmet) == [1, 1, 1] and list(verd) == [OK, OK, OK]
    assert len(a.v.waiters()) == 2 and len(o.waiters()) == 1 and len(b.v.waiters()) == 1
    assert ctx.var_recheck_many([a.v, o, b.v], cap=3) == [(OK, [1]), (OK, [77]), (OK, [3])]
    a.m.reply()
    b.m.reply()
    assert a.v.waiters() == a.m.listing() and o.waiters() == [] and b.v.waiters() == []
    # counters alone, and a set alone, still answer
    assert ctx.var_recheck_many([b.v, a.v]) == [(OK, []), (OK, [])]
    assert ctx.var_recheck_many([o]) == [(OK, [])]


@pytest.mark.parametrize("name", sorted(cm.REFUSED) + ["equal_terms", "truncated"])
def test_refused_input(ctx, name):
    r = Rep(ctx)
    r.bind([(1, 4), (A("a"), 1)])
    r.wait(9, False, 1)
    img = {"equal_terms": tb([(1.0, 2), (A("q"), 1)]),
           "truncated": tb(cm.VALID[2])[:-9]}.get(name) or cm.REFUSED[name]
    size = ctx.nif_stats()["dict_elements"]
    f0 = ctx.nif_stats()["fallbacks"]
    assert r.v.bind(img) == (FALLBACK, 0)
    assert ctx.var_bind_many([(r.v, img)]) == [(FALLBACK, 0)]
    assert ctx.nif_stats()["fallbacks"] - f0 == 2
    if name == "truncated":
        assert r.v.threshold(img) == (FALLBACK, None)
        assert r.v.wait(img, False, 2) == (FALLBACK, None)
    else:
        # a term that is no number: above every sum (lasp_lattice.erl:87-90)
        assert r.v.threshold(img) == (OK, False)
    assert ctx.nif_stats()["dict_elements"] == size
    r.check()
    # write/4 holds the image on the host; the variable then answers FALLBACK
    assert r.v.write(img) == FALLBACK
    assert not r.v.resident
    assert r.v.read() == (OK, img)
    assert r.v.value() == (FALLBACK, None)
    assert r.v.threshold(tb(1)) == (FALLBACK, None)
    assert r.v.wait(tb(1), False, 3) == (FALLBACK, None)
    assert r.v.bind(tb([(1, 9)])) == (FALLBACK, 0)
    assert r.v.increment(tb(A("increment")), tb(1)) == (FALLBACK,)
    assert r.v.increment(tb(A("increment")), tb(1), cap=4)[0] == FALLBACK
    assert r.v.recheck()[0] == FALLBACK
    assert r.v.waiters() == r.m.listing()
    assert ctx.nif_stats()["dict_elements"] == size
    # a representable write brings it back
    r.write([(1, 9)])
    r.check()
    assert r.recheck() == [1]


def test_refused_operations(ctx):
    r = Rep(ctx)
    r.bind([(A("a"), M64), (A("b"), 1)])
    size = ctx.nif_stats()["dict_elements"]
    for op in [(A("increment"), 0), (A("increment"), -3), (A("decrement"), 1), A("decrement"),
               (A("increment"), 1 << 64), (A("increment"), 1.0), (A("increment"), 1, 2)]:
        assert r.v.increment(tb(op), tb(A("fresh"))) == (FALLBACK,), op
        assert r.v.increment(tb(op), tb(A("fresh")), cap=4)[0] == FALLBACK, op
    # a count that would pass 2^64 - 1, with and without the fused re-check
    assert r.v.increment(tb(A("increment")), tb(A("a"))) == (FALLBACK,)
    assert r.v.increment(tb((A("increment"), 5)), tb(A("a")), cap=4)[0] == FALLBACK
    # an actor `==` to a registered one under another image
    r2 = Rep(ctx)
    r2.bind([(1, 1)])
    assert r2.v.increment(tb(A("increment")), tb(1.0)) == (FALLBACK,)
    r2.check()
    assert ctx.nif_stats()["dict_elements"] == size + 1
    # the sum wraps at 2^64 (b's own count does not)
    r.increment(A("increment"), A("b"), fused=True)
    r.check()
    assert cm.total(r.m.value) == 1
    # update/3 without its Actor and union/7 are the reference's to run
    assert r.v.update(tb((A("add"), 1)))[0] == FALLBACK
    assert r.v.union(r.v, r.v) == (FALLBACK, 0)
    r.check()
    o = ctx.var("orset")
    with pytest.raises(_lib.LaspjError):
        o.increment(tb(A("increment")), tb(A("a")))


def test_unknown_kind_is_an_error(ctx):
    with pytest.raises(ValueError):
        ctx.var("gcounters")


def test_lattice_kats_through_the_variable(ctx):
    """lasp_lattice.erl:386-443's A1 / A2 / A3 / B1 / B2, as far as a threshold read says
    them: the threshold is value(Prev), so `Prev =< Cur` in value — which holds for the
    concurrent pair {A2, B2} too, where is_lattice_inflation compares per actor and says no."""
    a1, b1 = [], []
    a2 = cm.GC.update(A("increment"), A("a"), a1)[1]
    a3 = cm.GC.update(A("increment"), A("a"), a2)[1]
    b2 = cm.GC.update(A("increment"), A("b"), b1)[1]
    cases = [(a1, b1, True, False), (a2, b1, False, False), (a1, a2, True, True),
             (b1, a2, True, True), (a2, b2, True, False), (a2, a2, True, False),
             (a2, a3, True, True)]
    for prev, cur, ge, gt in cases:
        r = Rep(ctx)
        r.bind(cur)
        th = cm.total(prev)
        assert olat.threshold_met(cm.TYPE, cur, th) == ge
        assert olat.threshold_met(cm.TYPE, cur, ("strict", th)) == gt
        assert r.v.threshold(tb(th)) == (OK, ge)
        assert r.v.threshold(tb(th), True) == (OK, gt)
    # merge of the concurrent pair: both actors, value 2
    r = Rep(ctx)
    r.bind(a2)
    assert r.bind(b2) == WRITTEN and r.m.value == [(A("a"), 1), (A("b"), 1)]
    r.check()


def test_counters_survive_a_dictionary_reset(ctx):
    a = Rep(ctx)
    b = a.replica()
    a.bind(counter(70))
    b.bind([(3, 50)])
    a.wait(cm.total(a.m.value) + 1, False, 1)
    ctx.nif_reset()
    assert a.v.read() == (OK, tb(a.m.value))
    assert a.increment(A("increment"), 200, fused=True) == [1]
    assert b.v.read() == (OK, tb(b.m.value))
    b.bind(a.m.value)
    a.row = b.row = True
    a.check()
    b.check()
