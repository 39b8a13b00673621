"""Resident filter processes and the resident G-Set intersection (include/laspj.h "resident
filter processes"; lasp_amd/csrc/laspj_process.hip, laspj_nif_process.hip) against filters_model:
filter/6 (lasp_core.erl:681-712) re-run over device variables with the fun's results kept
in two device bitmaps, and intersection/7's G-Set branch (:569-576).  Every case compares
the output variable's image with the model's bind of the oracle's body."""

import random

import pytest

import filters_model as fm
import update4_model as um
from oracle import etf as oetf
from oracle.terms import Atom, exact_eq

OK, FALLBACK = 0, 1
NOOP, WRITTEN = fm.NOOP, fm.WRITTEN
A = Atom

pytestmark = pytest.mark.gpu


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def _status(exc) -> int:
    return exc.value.status


def upd(var, cur, op, type_="lasp_orset"):
    """update/4 on the device variable and, with the tokens it minted, on the model
    (tests/update4_model.py: update/3, then the bind's merge with cur)."""
    verd, res, _err, minted = var.update(tb(op))
    assert verd == OK, op
    want = um.update4(type_, op, cur, minted)
    assert (res == 0) == (want[0] == "ok"), op
    return want[1] if want[0] == "ok" else cur


class Proc:
    """A device filter beside its model; `fun` is recorded call by call."""

    def __init__(self, ctx, type_, in_var, out_var, pred):
        self.type_, self.in_var, self.out_var = type_, in_var, out_var
        self.calls = []
        self.pred = pred
        self.f = ctx.filter(in_var, out_var)
        self.m = fm.FilterModel(type_, pred)
        self.out = []

    def fun(self, v):
        self.calls.append(v)
        return self.pred(v)

    def step(self, value, where=None):
        """NifFilter.step against the model's: status, the arguments Function got (exactly
        the unseen held elements, in term order) and out's image."""
        want_args = self.m.args(value)
        n0 = len(self.calls)
        verd, st, pend = self.f.step(self.fun)
        assert (verd, pend) == (OK, 0), where
        got = self.calls[n0:]
        assert len(got) == len(want_args) and all(exact_eq(a, b) for a, b in zip(got, want_args)), where
        want_st, _first, self.out = self.m.step(value, self.out)
        assert st == want_st, where
        assert self.out_var.read() == (OK, tb(self.out)), where
        return st

    def run(self, value, where=None):
        """One laspj_filter_run against the model's."""
        want_st, want_pend, self.out = self.m.run(value, self.out)
        assert self.f.run() == (OK, want_st, want_pend), where
        return want_st, want_pend

    def feed(self, value):
        """args -> Function -> results for the pending elements, both sides."""
        verd, img, n = self.f.args()
        want = self.m.args(value)
        got = oetf.binary_to_term(img)
        assert verd == OK and n == len(want)
        assert len(got) == n and all(exact_eq(a, b) for a, b in zip(got, want))
        self.f.results(tb([self.fun(a) for a in got]))
        self.m.evaluate(value)
        return n


def test_orset_filter_matches_model():
    """40 random {add, E} / {remove, E} on in, a re-run after each: narrow cells, then a
    namespace widened by 70 tokens on one element (two pairs per cell)."""
    ctx = _ctx()
    try:
        rng = random.Random(101)
        for wide in (False, True):
            inv = ctx.var("orset")
            cur = []
            if wide:
                for _ in range(70):
                    cur = upd(inv, cur, (A("add"), 7))
                assert ctx.nif_stats()["namespaces_widened"] >= 1
            p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
            for k in range(40):
                e = rng.randrange(40)
                cur = upd(inv, cur, (A("add"), e) if rng.random() < 0.7 else (A("remove"), e))
                if k % 2 == 0:
                    # the pending count of the first run, then the loop by hand
                    st, pend = p.run(cur, (wide, k))
                    if pend:
                        assert st == NOOP and p.out_var.read() == (OK, tb(p.out))
                        assert p.feed(cur) == pend
                        p.run(cur, (wide, k))
                    assert p.out_var.read() == (OK, tb(p.out)), (wide, k)
                else:
                    p.step(cur, (wide, k))
            # Function was called once per element over the whole run
            assert len(p.calls) == len(set(p.calls)) == len(p.m.results) == len(cur)
            assert len(p.out) > 0
    finally:
        ctx.close()


def test_tombstoned_elements_are_kept():
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        cur = upd(inv, [], (A("add"), 3))
        cur = upd(inv, cur, (A("add"), 4))
        cur = upd(inv, cur, (A("remove"), 3))
        assert p.step(cur) == WRITTEN
        tok = cur[0][1][0][0]
        assert p.out == [(3, [(tok, True)])]
        assert p.out_var.read() == (OK, tb([(3, [(tok, True)])]))
        assert p.out_var.value() == (OK, tb([]))
    finally:
        ctx.close()


def _orset_shape(ctx, n, sparse):
    """in over a namespace of n element slots (slot k = element k): all held, or — sparse —
    every third absent (the slots come from a second replica's state) and some tombstoned."""
    full = ctx.var("orset")
    state = upd(full, [], (A("add_all"), list(range(n))))
    inv = full.replica()
    if not sparse:
        assert inv.bind(tb(state)) == (OK, 1)
        return inv, state, full
    cur = [ent for ent in state if ent[0] % 3 != 1 or ent[0] == n - 1]
    assert inv.bind(tb(cur))[0] == OK
    for e in [x[0] for x in cur][::5]:
        if e != n - 1:
            cur = upd(inv, cur, (A("remove"), e))
    return inv, cur, full


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130, 256, 257, 300])
def test_orset_wave_and_block_boundaries(n):
    """Held-element counts on both sides of a wave (64) and a block (256), dense and sparse,
    with a predicate that keeps the last slot: out bit for bit."""
    ctx = _ctx()
    try:
        for sparse in (False, True):
            inv, cur, _full = _orset_shape(ctx, n, sparse)
            p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e == n - 1 or e % 2 == 0)
            st, pend = p.run(cur, (n, sparse))
            assert (st, pend) == (NOOP, len(cur))
            assert p.step(cur, (n, sparse)) == WRITTEN
            assert any(ent[0] == n - 1 for ent in p.out)
            assert p.run(cur, (n, sparse)) == (NOOP, 0)
            # one more token on the last slot: written again, nothing pending
            cur = upd(inv, cur, (A("add"), n - 1))
            assert p.step(cur, (n, sparse)) == WRITTEN
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [64, 65, 16385])
def test_gset_word_and_block_boundaries(n):
    """G-Sets of one bitmap word, two, and 257 (a word in a second block; one {add_all, ...})."""
    ctx = _ctx()
    try:
        inv = ctx.var("gset")
        cur = upd(inv, [], (A("add_all"), list(range(n))), "lasp_gset")
        assert len(cur) == n
        p = Proc(ctx, "lasp_gset", inv, inv.replica(), lambda e: e == n - 1 or e % 2 == 0)
        assert p.run(cur, n) == (NOOP, n)
        assert p.step(cur, n) == WRITTEN
        assert p.out[-1] == n - 1 and len(p.calls) == n
        assert p.run(cur, n) == (NOOP, 0)
    finally:
        ctx.close()


def test_status_rule():
    """bind/3's `Value0 =:= AccValue`: a strict superset in out answers WRITTEN every time and
    stays as it is; out exactly AccValue answers NOOP; out == in."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        cur = upd(inv, [], (A("add_all"), list(range(10))))
        sup = inv.replica()
        assert sup.bind(tb(cur)) == (OK, 1)
        p = Proc(ctx, "lasp_orset", inv, sup, lambda e: e % 3 == 0)
        p.out = cur
        assert p.step(cur) == WRITTEN and p.out == cur
        assert p.run(cur) == (WRITTEN, 0) and p.out == cur
        assert sup.read() == (OK, tb(cur))
        q = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        assert q.step(cur) == WRITTEN
        assert q.run(cur) == (NOOP, 0)
        assert [e for e, _t in q.out] == [0, 3, 6, 9]
        # out == in: in is a strict superset of its own filtered value
        s = Proc(ctx, "lasp_orset", inv, inv, lambda e: e % 3 == 0)
        s.out = cur
        assert s.step(cur) == WRITTEN and s.run(cur) == (WRITTEN, 0)
        assert inv.read() == (OK, tb(cur))
        # and a G-Set onto itself with everything kept: equal, NOOP
        g = ctx.var("gset")
        gcur = upd(g, [], (A("add_all"), [1, 2, 3]), "lasp_gset")
        t = Proc(ctx, "lasp_gset", g, g, lambda e: True)
        t.out = gcur
        assert t.step(gcur) == NOOP
    finally:
        ctx.close()


def test_pending_leaves_out_untouched():
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        cur = upd(inv, [], (A("add_all"), [0, 1, 3]))
        p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        assert p.step(cur) == WRITTEN
        before = p.out_var.read()
        cur = upd(inv, cur, (A("add"), 3))          # an evaluated, kept element changes
        cur = upd(inv, cur, (A("add"), 9))          # and a new one arrives
        assert p.run(cur) == (NOOP, 1)
        assert p.out_var.read() == before
        assert p.feed(cur) == 1
        assert p.run(cur) == (WRITTEN, 0)
        assert [(e, len(t)) for e, t in p.out] == [(0, 1), (3, 2), (9, 1)]
        assert p.out_var.read() == (OK, tb(p.out))
    finally:
        ctx.close()


def test_results_errors():
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        cur = upd(inv, [], (A("add_all"), [0, 1, 2]))
        p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        with pytest.raises(_lib.LaspjError) as ex:
            p.f.results(tb([True]))                   # nothing outstanding yet
        assert _status(ex) == _lib.E_INVAL
        assert p.run(cur) == (NOOP, 3)
        assert p.f.args()[2] == 3
        for bad in ([True, False], [True] * 4, []):
            with pytest.raises(_lib.LaspjError) as ex:
                p.f.results(tb(bad))
            assert _status(ex) == _lib.E_INVAL
        assert p.run(cur) == (NOOP, 3)              # nothing was recorded
        assert p.feed(cur) == 3
        with pytest.raises(_lib.LaspjError) as ex:
            p.f.results(tb([True, False, False]))     # the list was used up
        assert _status(ex) == _lib.E_INVAL
        assert p.run(cur) == (WRITTEN, 0)
        assert p.out_var.read() == (OK, tb(p.out))
        assert p.f.args() == (OK, tb([]), 0)        # nothing pending: the image of []
        p.f.results(tb([]))
    finally:
        ctx.close()


def test_gset_pair_elements():
    """A G-Set element that is a 2-tuple gives its first component as the argument; two
    elements with one first component get an answer each."""
    ctx = _ctx()
    try:
        inv = ctx.var("gset")
        elems = [(A("a"), 1), (A("a"), 2), (A("b"), 1), 5]
        cur = upd(inv, [], (A("add_all"), elems), "lasp_gset")
        p = Proc(ctx, "lasp_gset", inv, inv.replica(), lambda v: v == A("a"))
        assert p.run(cur) == (NOOP, 4)
        verd, img, n = p.f.args()
        assert (verd, n) == (OK, 4)
        assert oetf.binary_to_term(img) == p.m.args(cur) == [5, A("a"), A("a"), A("b")]
        # (answers no pure fun would give: each element keeps its own)
        answers = [False, True, False, True]
        p.f.results(tb(answers))
        for e, r in zip(p.m.pending(cur), answers):
            p.m.results[tb(e)] = r
        assert p.run(cur) == (WRITTEN, 0)
        assert p.out == [(A("a"), 1), (A("b"), 1)]
        assert p.out_var.read() == (OK, tb(p.out))
        # and through step with a pure fun
        q = Proc(ctx, "lasp_gset", inv, inv.replica(), lambda v: v == A("a"))
        assert q.step(cur) == WRITTEN and q.out == [(A("a"), 1), (A("a"), 2)]
    finally:
        ctx.close()


def test_lifecycle_reset_growth_host_held_destroy():
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        other = inv.replica()
        cur = upd(inv, [], (A("add_all"), list(range(20))))
        p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        assert p.step(cur) == WRITTEN
        # growth: elements only another replica holds are nobody's pending
        upd(other, [], (A("add_all"), list(range(100, 400))))
        assert p.run(cur) == (NOOP, 0)
        cur = upd(inv, cur, (A("add"), 21))
        assert p.run(cur) == (NOOP, 1)
        assert p.feed(cur) == 1 and p.run(cur) == (WRITTEN, 0)
        # an argument list outstanding across a dictionary reset is dropped
        cur = upd(inv, cur, (A("add"), 22))
        assert p.run(cur) == (NOOP, 1) and p.f.args()[2] == 1
        h0 = ctx.nif_stats()["vars_hydrated"]
        ctx.nif_reset()
        p.m.reset()
        p.f.results(tb([True]))                       # OK, nothing recorded
        assert p.run(cur) == (NOOP, len(cur))       # every held element pending again
        assert ctx.nif_stats()["vars_hydrated"] > h0
        assert p.step(cur) == NOOP                  # out already holds AccValue
        cur = upd(inv, cur, (A("add"), 24))
        assert p.step(cur) == WRITTEN
        # a host-held in: FALLBACK, out as it was
        toks = sorted([bytes([k]) * 20 for k in range(64)] + [bytes([64]) * 20 + b"xy"])
        assert inv.write(tb([(1, [(t, False) for t in toks])])) == FALLBACK and not inv.resident
        fb0 = ctx.nif_stats()["fallbacks"]
        assert p.f.run()[0] == FALLBACK
        assert p.f.args()[0] == FALLBACK
        assert ctx.nif_stats()["fallbacks"] == fb0 + 2
        assert p.out_var.read() == (OK, tb(p.out))
        # in destroyed first: the filter is dead, not dangling
        inv.close()
        with pytest.raises(_lib.LaspjError) as ex:
            p.f.run()
        assert _status(ex) == _lib.E_INVAL
        with pytest.raises(_lib.LaspjError) as ex:
            ctx.filter_run_many([p.f])
        assert _status(ex) == _lib.E_INVAL
        p.f.close()
    finally:
        ctx.close()


def test_run_many():
    """Five filters in one pass — two OR-Set filters on one in, one over a wide namespace,
    two G-Set — some pending, some ready; one device pass per call."""
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        a = ctx.var("orset")
        acur = upd(a, [], (A("add_all"), list(range(70))))
        w = ctx.var("orset")
        wcur = []
        for _ in range(70):
            wcur = upd(w, wcur, (A("add"), 7))
        wcur = upd(w, wcur, (A("add_all"), list(range(30))))
        assert ctx.nif_stats()["namespaces_widened"] >= 1
        g = ctx.var("gset")
        gcur = upd(g, [], (A("add_all"), list(range(100))), "lasp_gset")
        h = ctx.var("gset")
        hcur = upd(h, [], (A("add_all"), [A("x"), A("y"), 3]), "lasp_gset")
        ps = [Proc(ctx, "lasp_orset", a, a.replica(), lambda e: e % 3 == 0),
              Proc(ctx, "lasp_orset", a, a.replica(), lambda e: e % 2 == 1),
              Proc(ctx, "lasp_orset", w, w.replica(), lambda e: e % 5 == 0),
              Proc(ctx, "lasp_gset", g, g.replica(), lambda e: e % 4 == 0),
              Proc(ctx, "lasp_gset", h, h.replica(), lambda e: e == A("x"))]
        curs = [acur, acur, wcur, gcur, hcur]

        def many(where):
            p0 = ctx.nif_stats()["device_passes"]
            got = ctx.filter_run_many([p.f for p in ps])
            assert ctx.nif_stats()["device_passes"] == p0 + 1, where
            for k, p in enumerate(ps):
                st, pend, p.out = p.m.run(curs[k], p.out)
                assert got[k] == (OK, st, pend), (where, k)
            for k, p in enumerate(ps):
                assert p.out_var.read() == (OK, tb(p.out)), (where, k)
            return got

        # filters 1 and 3 ready, the rest pending
        ps[1].step(acur)
        ps[3].step(gcur)
        acur = curs[0] = curs[1] = upd(a, acur, (A("remove"), 5))
        got = many("mixed")
        assert [x[2] for x in got] == [70, 0, 30, 0, 3]
        assert got[1][1] == WRITTEN and got[3][1] == NOOP
        for k in (0, 2, 4):
            ps[k].feed(curs[k])
        got = many("ready")
        assert [x[1:] for x in got] == [(WRITTEN, 0), (NOOP, 0), (WRITTEN, 0), (NOOP, 0),
                                        (WRITTEN, 0)]
        assert [x[1:] for x in many("again")] == [(NOOP, 0)] * 5
        # two filters binding one out would race
        clash = ctx.filter(a, ps[0].out_var)
        with pytest.raises(_lib.LaspjError) as ex:
            ctx.filter_run_many([ps[0].f, clash])
        assert _status(ex) == _lib.E_INVAL
        with pytest.raises(_lib.LaspjError) as ex:
            ctx.filter_run_many([ps[0].f, ps[0].f])
        assert _status(ex) == _lib.E_INVAL
    finally:
        ctx.close()


def test_waiter_on_out_fires_from_recheck_after_written():
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        cur = upd(inv, [], (A("add"), 3))
        assert p.out_var.wait(tb(cur), False, 11) == (OK, False)
        assert p.out_var.recheck() == (OK, [], 1)
        assert p.run(cur) == (NOOP, 1)
        assert p.out_var.recheck() == (OK, [], 1)
        assert p.step(cur) == WRITTEN
        assert len(p.out_var.waiters()) == 1        # the run itself answers nobody
        assert p.out_var.recheck() == (OK, [11], 0)
    finally:
        ctx.close()


def test_gset_intersection_matches_model():
    ctx = _ctx()
    try:
        rng = random.Random(202)
        l = ctx.var("gset")
        r, out = l.replica(), l.replica()
        vs = {"l": l, "r": r}
        cur = {"l": [], "r": [], "out": []}
        written = 0
        for k in range(30):
            name = rng.choice(("l", "r"))
            e = rng.randrange(200) if k else 199
            cur[name] = upd(vs[name], cur[name], (A("add"), e), "lasp_gset")
            if k == 0:
                cur["r"] = upd(r, cur["r"], (A("add_all"), [199, 64, 63, 0]), "lasp_gset")
                cur["l"] = upd(l, cur["l"], (A("add_all"), [199, 64, 63, 128]), "lasp_gset")
            st, cur["out"] = fm.intersection(cur["l"], cur["r"], cur["out"])
            assert out.intersection(l, r) == (OK, st), k
            assert out.read() == (OK, tb(cur["out"])), k
            written += st
        assert written >= 1 and len(cur["out"]) >= 3
        st, cur["l"] = fm.intersection(cur["l"], cur["r"], cur["l"])
        assert l.intersection(l, r) == (OK, st)
        assert l.read() == (OK, tb(cur["l"]))
        # the bodies this path does not take: out as it was
        before = out.read()
        assert out.intersection(l, ctx.var("gset"))[0] == FALLBACK         # two namespaces
        o1 = ctx.var("orset")
        assert o1.intersection(o1, o1.replica())[0] == FALLBACK             # OR-Sets
        c = ctx.var("gcounter")
        assert c.intersection(l, r)[0] == FALLBACK                          # a counter
        upd(r, cur["r"], (A("add"), (A("x"), A("y"))), "lasp_gset")
        assert out.intersection(l, r)[0] == FALLBACK                        # a 2-tuple element
        assert out.read() == before
    finally:
        ctx.close()


def test_filter_create_errors():
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        o, g, c = ctx.var("orset"), ctx.var("gset"), ctx.var("gcounter")
        for pair, want in (((o, g), _lib.E_KIND), ((c, c), _lib.E_KIND), ((o, c), _lib.E_KIND),
                           ((o, ctx.var("orset")), _lib.E_UNSUPPORTED),
                           ((g, ctx.var("gset")), _lib.E_UNSUPPORTED)):
            with pytest.raises(_lib.LaspjError) as ex:
                ctx.filter(*pair)
            assert _status(ex) == want
        ctx.filter(o, o.replica()).close()
        ctx.filter(g, g).close()
    finally:
        ctx.close()


def test_readd_by_a_removed_token_is_no_new_input():
    """update/4 is update/3 then the bind's merge (lasp_core.erl:283-312): an add_by_token by
    a token in holds removed, and a remove then an add_by_token of an element's only token
    in one call, leave in as it was — the re-run answers what the model answers, a no-op,
    and out reads as before."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        tok = lambda k: bytes([k]) * 20                  # noqa: E731
        value = []
        for e in range(7):
            value = upd(inv, value, (A("add_by_token"), tok(e), e))
        value = upd(inv, value, (A("remove"), 3))
        p = Proc(ctx, "lasp_orset", inv, inv.replica(), lambda e: e % 3 == 0)
        assert p.step(value) == WRITTEN
        before = p.out_var.read()
        assert before == (OK, tb([(0, [(tok(0), False)]), (3, [(tok(3), True)]),
                                  (6, [(tok(6), False)])]))
        for op in ((A("add_by_token"), tok(3), 3),
                   (A("update"), [(A("remove"), 6), (A("add_by_token"), tok(6), 6)])):
            assert upd(inv, value, op) == value
            assert inv.read() == (OK, tb(value)), op
            assert p.run(value, op) == (NOOP, 0)
            assert p.out_var.read() == before, op
    finally:
        ctx.close()
