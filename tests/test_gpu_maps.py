"""Resident map processes (include/laspj.h "resident map processes"; lasp_amd/csrc/
laspj_lvars.hip k_lm_count / k_lm_write, laspj_nif_maps.hip) against tests/maps_model.py:
map/6's body (lasp_core.erl:641-667) re-run from a resident OR-Set's cells and bound with
bind/3 (:291-312) into a list-valued variable.  Every case compares status, pending and
verdict, the decoded out.read() (list order, token order, flags) and laspj_lvar_counts with
the model."""

import random

import pytest

import lvars_model as lm
import maps_model as mm
import update4_model as um
from oracle import etf as oetf
from oracle.terms import Atom

OK, FALLBACK = 0, 1
NOOP, WRITTEN, REFUSED = mm.NOOP, mm.WRITTEN, mm.REFUSED
A = Atom

pytestmark = pytest.mark.gpu


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def tok(k: int) -> bytes:
    """A 20-byte token (the length unique/1 mints); k orders them."""
    return k.to_bytes(4, "big") + bytes(16)


def upd(var, cur, op):
    """update/4 on the device variable and, with the tokens it minted, on the model
    (tests/update4_model.py: update/3, then the bind's merge with cur)."""
    verd, res, _err, minted = var.update(tb(op))
    assert verd == OK, op
    want = um.update4("orset", op, cur, minted)
    assert (res == 0) == (want[0] == "ok"), op
    return want[1] if want[0] == "ok" else cur


def value_of(elems, seed, maxtok=5):
    """An OR-Set value over elems (ascending): 1..maxtok tokens per element, minted out of
    term order, about a third removed."""
    rng = random.Random(seed)
    out = []
    for i, e in enumerate(elems):
        nt = 1 + rng.randrange(maxtok)
        ks = rng.sample(range(8 * i, 8 * i + 8), nt)
        out.append((e, sorted((tok(k), rng.random() < 0.34) for k in ks)))
    return out


class Proc:
    """A device map and its model, stepped side by side."""

    def __init__(self, ctx, inv, fun, out=None):
        self.ctx, self.inv, self.fun = ctx, inv, fun
        self.lv = out if out is not None else ctx.list_var(inv)
        self.p = ctx.map(inv, self.lv)
        self.m = mm.MapModel(fun)
        self.out = []

    def check_out(self, where=None):
        verd, img = self.lv.read()
        assert verd == OK, where
        assert oetf.binary_to_term(img) == self.out, where
        assert img == tb(self.out), where
        assert self.lv.counts() == lm.counts(self.out), where

    def run(self, value, where=None):
        """One laspj_map_run against the model's."""
        st, pend, new = self.m.run(value, self.out)
        assert self.p.run() == (OK, st, pend), where
        self.out = new
        return st, pend

    def step(self, value, where=None):
        """NifMap.step against the model's: the status; out compared."""
        self.m.note_value(value)
        first = len(self.m.pending(value))
        if first:
            assert self.p.run() == (OK, NOOP, first), where
            verd, img, n = self.p.args()
            assert (verd, n) == (OK, first), where
            assert oetf.binary_to_term(img) == self.m.args(value), where
        want = self.m.step(value, self.out)
        assert want is not None, where
        st, _first, self.out = want
        assert self.p.step(self.fun) == (OK, st, 0), where
        self.check_out(where)
        return st

    def close(self):
        self.p.close()
        self.lv.close()


SIZES = [0, 1, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049]


def _held_and_extra(n):
    """n held elements (even integers) and odd ones between them that only a replica holds."""
    held = [2 * i for i in range(n)]
    extra = [2 * i + 1 for i in range(0, n + 3, 3)]
    return held, extra


@pytest.mark.parametrize("n", SIZES)
def test_sizes_at_the_kernels_edges(n):
    """Wave, block and 1024-position tile edges; the replica's elements make positions the
    producer skips; X + 10000 gives new ascending keys (the rank-indexed bind)."""
    ctx = _ctx()
    try:
        held, extra = _held_and_extra(n)
        inv = ctx.var("orset")
        rep = inv.replica()
        assert rep.write(tb(value_of(extra, 99, 2))) == OK
        value = value_of(held, n)
        if value:
            assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: x + 10000)
        st = p.step(value, n)
        assert st == (WRITTEN if n else NOOP)
        assert [k for k, _t in p.out] == [e + 10000 for e in held]
        assert p.run(value, n) == (NOOP, 0)
        if n:
            # one more token on the last element: no fun, one re-run, written
            value = upd(inv, value, (A("add"), held[-1]))
            assert p.run(value, n) == (WRITTEN, 0)
            p.check_out(n)
        p.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [1, 65, 1025])
def test_identity(n):
    """y == e: nothing is registered and the output equals in's value."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(n)), 7 + n)
        assert inv.write(tb(value)) == OK
        e0 = ctx.nif_stats()["dict_elements"]
        p = Proc(ctx, inv, lambda x: x)
        assert p.step(value, n) == WRITTEN
        assert p.out == value
        assert inv.read() == p.lv.read()
        assert ctx.nif_stats()["dict_elements"] == e0
        value = upd(inv, value, (A("add"), n - 1))
        assert p.run(value, n) == (WRITTEN, 0)
        p.check_out(n)
        assert p.out == value
        p.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [5, 65, 1025])
def test_non_injective(n):
    """X div 2: repeated keys, the tokens of two inputs in one rank row (at most 15 tokens
    under a key, its own included: verdict OK)."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(n)), 31 + n)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: x // 2)
        assert p.step(value, n) == WRITTEN
        assert [k for k, _t in p.out] == [e // 2 for e in range(n)]
        assert p.run(value, n) == (NOOP, 0)
        value = upd(inv, value, (A("add"), n - 1))
        value = upd(inv, value, (A("remove"), 0))
        st, new = lm.bind(p.out, p.m.acc(value))
        assert p.run(value, n) == (st, 0)
        p.check_out(n)
        p.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("n", [3, 65, 300])
def test_order_reversing(n):
    """-X: descending keys — the merge path, and not_asc at the next re-run."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(1, n + 1)), 5 + n, 3)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: -x)
        assert p.step(value, n) == WRITTEN
        assert [k for k, _t in p.out] == [-e for e in range(1, n + 1)]
        assert p.run(value, n) == (NOOP, 0)
        value = upd(inv, value, (A("add"), n // 2 + 1))
        st, pend = p.run(value, n)
        assert pend == 0 and st in (WRITTEN, REFUSED)           # (the model decided which)
        p.check_out(n)
        # a new element: the second bind of a longer descending list
        value = upd(inv, value, (A("add"), n + 1))
        p.step(value, n)
        p.close()
    finally:
        ctx.close()


def _mixed(x):
    kinds = (lambda v: A("k%d" % v), lambda v: (A("t"), v, b"x"), lambda v: b"bin%d" % v,
             lambda v: (v, (v + 1,)), lambda v: 2 ** 40 + v)
    return kinds[x % len(kinds)](x)


def test_mixed_term_kinds():
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(70)), 17, 3)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, _mixed)
        assert p.step(value) == WRITTEN
        assert [k for k, _t in p.out] == [_mixed(e) for e in range(70)]
        assert p.run(value) == (NOOP, 0)
        # inputs of mixed kinds too
        inv2 = ctx.var("orset")
        elems = sorted([3, -2, 2 ** 40, A("a"), A("zz"), b"", b"bin", (1, 2, 3), (A("k"), 1)],
                       key=lambda t: oetf.term_to_binary(t))
        value2 = []
        for e in elems:
            value2 = upd(inv2, value2, (A("add"), e))
        q = Proc(ctx, inv2, lambda x: (A("m"), x))
        assert q.step(value2) == WRITTEN
        assert len(q.out) == len(elems)
        p.close()
        q.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("fun,repeats", [(lambda x: x + 10000, False),
                                         (lambda x: x // 2 + 5000, True)], ids=["shift", "div2"])
def test_steady_steps(fun, repeats):
    """Three hundred random update/4 ops on in, each followed by step(fun) and replayed on
    the model with the device's minted tokens; several tokens per element exercise the
    popcount placement."""
    ctx = _ctx()
    try:
        rng = random.Random(4711)
        inv = ctx.var("orset")
        p = Proc(ctx, inv, fun)
        value = []
        known = list(range(12))
        seen = {NOOP: 0, WRITTEN: 0, REFUSED: 0}
        for step in range(300):
            r = rng.random()
            if r < 0.55 and value:
                op = (A("add"), rng.choice(value)[0])            # a known element
            elif r < 0.75:
                e = rng.randrange(400) if rng.random() < 0.5 else rng.choice(known)
                op = (A("add"), e)
            else:
                op = (A("remove"), rng.choice(value)[0] if value else 0)
            value = upd(inv, value, op)
            seen[p.step(value, step)] += 1
        # (the model decided every status; over repeated keys bind/3 refuses many merges —
        # orddict:merge as written does not inflate such lists — so div2 counts both)
        assert seen[WRITTEN] + (seen[REFUSED] if repeats else 0) >= 100, seen
        assert max(len(t) for _k, t in value) >= 4
        assert ctx.nif_stats()["fallbacks"] == 0
        p.close()
    finally:
        ctx.close()


def test_new_element_is_the_only_pending_one():
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(40)), 3)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: x + 10000)
        assert p.step(value) == WRITTEN
        value = upd(inv, value, (A("add"), 77))
        before = p.lv.read()
        assert p.p.run() == (OK, NOOP, 1)
        assert p.lv.read() == before
        verd, img, n = p.p.args()
        assert (verd, n) == (OK, 1) and oetf.binary_to_term(img) == [77]
        assert p.p.args() == (OK, img, 1)                        # nothing was registered
        assert p.p.results(tb([10077])) == OK
        p.m.note_value(value)
        assert p.m.evaluate(value)
        assert p.run(value) == (WRITTEN, 0)
        p.check_out()
        p.close()
    finally:
        ctx.close()


def test_token_the_map_registered_turns_up_in_the_input():
    """X div 2 puts 8's tokens under key 4, an input element too; the host does not pass such
    a slot on.  add_by_token then gives element 4 that very token: the device reports it
    unmapped, the host maps every token and the pass runs again inside the call."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(10)), 3, 2)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: x // 2)
        assert p.step(value) == WRITTEN
        t8 = value[8][1][0][0]
        value = upd(inv, value, (A("add_by_token"), t8, 4))
        assert t8 in [t for t, _f in dict(value)[4]]
        passes = ctx.nif_stats()["device_passes"]
        p.step(value)                                            # (the model's status)
        assert ctx.nif_stats()["device_passes"] >= passes + 2    # the pass, and again
        assert ctx.nif_stats()["fallbacks"] == 0
        # a second map from []: its output is AccValue itself, t8 under keys 4 (from 8) and 2 (from 4)
        q = Proc(ctx, inv, lambda x: x // 2)
        assert q.step(value) == WRITTEN
        assert sum(t == t8 for k, toks in q.out if k == 2 for t, _f in toks) == 1
        assert sum(t == t8 for k, toks in q.out if k == 4 for t, _f in toks) == 1
        q.close()
        value = upd(inv, value, (A("add"), 9))
        p.step(value)
        p.close()
    finally:
        ctx.close()


def test_peer_image_agrees_id_for_id():
    """The model's AccValue bound through laspj_lvar_etf_bind (the walker's ids), then the
    map's run over the same value: NOOP — and the other way round."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(130)), 23)
        assert inv.write(tb(value)) == OK
        fun = lambda x: x // 2 + 1000                            # noqa: E731
        acc = [(fun(k), t) for k, t in value]
        lv = ctx.list_var(inv)
        assert lv.bind(tb(acc)) == (OK, WRITTEN)
        p = Proc(ctx, inv, fun, out=lv)
        p.out = acc
        assert p.step(value) == NOOP
        p.p.close()
        # produced first, the peer's image after
        lv2 = ctx.list_var(inv)
        q = Proc(ctx, inv, fun, out=lv2)
        assert q.step(value) == WRITTEN
        assert lv2.bind(tb(acc)) == (OK, NOOP)
        assert lv2.read() == lv.read()
        q.close()
        lv.close()
    finally:
        ctx.close()


def test_cross_check_against_the_image_path():
    """The same value through laspj_var_etf_read + laspj_list_etf_args + laspj_list_etf_map +
    laspj_list_etf_bind gives the same image byte for byte (n = 257)."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(257)), 41)
        assert inv.write(tb(value)) == OK
        fun = lambda x: x + 10000                                # noqa: E731
        p = Proc(ctx, inv, fun)
        assert p.step(value) == WRITTEN
        verd, vimg = inv.read()
        assert verd == OK
        verd, aimg = ctx.list_etf("args", "orset", vimg)
        assert verd == OK
        res = tb([fun(a) for a in oetf.binary_to_term(aimg)])
        verd, acc = ctx.list_etf("map", "orset", vimg, res)
        assert verd == OK
        verd, st, img = ctx.list_etf_bind("orset", tb([]), acc)
        assert (verd, st) == (OK, WRITTEN)
        assert p.lv.read() == (OK, img)
        p.close()
    finally:
        ctx.close()


def _bystanders_still_answer(ctx, inv, value):
    """A filter and an update on the namespace after a refusal: both as the oracle says."""
    import filters_model as fm
    value = upd(inv, value, (A("add"), 1))
    out = inv.replica()
    f = ctx.filter(inv, out)
    m = fm.FilterModel("lasp_orset", lambda e: e % 2 == 0)
    st, _first, want = m.step(value, [])
    assert f.step(lambda e: e % 2 == 0) == (OK, st, 0)
    assert out.read() == (OK, tb(want))
    f.close()
    return value


def test_refusals():
    ctx = _ctx()
    try:
        # F(X) = float(X) over integer elements: `==`-equal terms under another image
        inv = ctx.var("orset")
        value = value_of(list(range(6)), 2)
        assert inv.write(tb(value)) == OK
        lv = ctx.list_var(inv)
        assert lv.bind(tb([(A("z"), [(tok(1), False)])])) == (OK, WRITTEN)
        before = lv.read()
        p = ctx.map(inv, lv)
        e0 = ctx.nif_stats()["dict_elements"]
        assert p.step(float) == (FALLBACK, NOOP, 6)
        assert ctx.nif_stats()["dict_elements"] == e0            # rolled back
        assert p.run() == (FALLBACK, NOOP, 0)
        assert p.args() == (FALLBACK, None, 0)
        assert lv.read() == before
        value = _bystanders_still_answer(ctx, inv, value)
        # another map of the namespace carries on
        q = Proc(ctx, inv, lambda x: x + 10000)
        assert q.step(value) == WRITTEN
        q.close()
        p.close()
        # seventy elements of one token each, F constant: 70 tokens under one key
        inv2 = ctx.var("orset")
        value2 = value_of(list(range(70)), 8, 1)
        assert inv2.write(tb(value2)) == OK
        lv2 = ctx.list_var(inv2)
        before = lv2.read()
        p2 = ctx.map(inv2, lv2)
        assert p2.step(lambda x: A("k")) == (FALLBACK, NOOP, 70)
        assert p2.run() == (FALLBACK, NOOP, 0)
        assert lv2.read() == before
        assert ctx.nif_stats()["namespaces_widened"] == 0
        _bystanders_still_answer(ctx, inv2, value2)
        m = mm.MapModel(lambda x: A("k"))
        assert m.step(value2, []) is None
        # a term kind the dictionary does not hold (an improper list, [1 | 2])
        inv3 = ctx.var("orset")
        assert inv3.write(tb(value[:3])) == OK
        lv3 = ctx.list_var(inv3)
        p3 = ctx.map(inv3, lv3)
        assert p3.run() == (OK, NOOP, 3)
        assert p3.args()[2] == 3
        assert p3.results(b"\x83l\x00\x00\x00\x03l\x00\x00\x00\x01a\x01a\x02a\x01a\x02j") == FALLBACK
        assert p3.run() == (FALLBACK, NOOP, 0)
    finally:
        ctx.close()


def test_lifecycle():
    from lasp_amd import _lib
    from lasp_amd._lib import LaspjError
    ctx = _ctx()
    try:
        fun = lambda x: x + 10000                                # noqa: E731
        inv = ctx.var("orset")
        value = value_of(list(range(20)), 13, 2)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, fun)
        assert p.step(value) == WRITTEN
        # two maps on one in
        q = Proc(ctx, inv, lambda x: x // 2)
        assert q.step(value) == WRITTEN
        # growth between runs: past the images' head-room
        value = upd(inv, value, (A("add_all"), list(range(100, 400))))
        assert p.step(value) == WRITTEN
        assert q.step(value) in (WRITTEN, REFUSED)               # (repeated keys: the model's)
        # results with no outstanding list, and with a wrong length
        with pytest.raises(LaspjError) as ei:
            p.p.results(tb([]))
        assert ei.value.status == _lib.E_INVAL
        value = upd(inv, value, (A("add_all"), [500, 501]))
        assert p.p.run() == (OK, NOOP, 2)
        assert p.p.args()[2] == 2
        with pytest.raises(LaspjError) as ei:
            p.p.results(tb([1, 2, 3]))
        assert ei.value.status == _lib.E_INVAL
        assert p.p.results(tb([10500, 10501])) == OK
        p.m.note_value(value)
        assert p.m.evaluate(value)
        assert p.run(value) == (WRITTEN, 0)
        p.check_out()
        # a dictionary reset: everything pending again, then the same value back
        assert p.p.run() == (OK, NOOP, 0)
        assert p.p.args()[2] == 0                                # an outstanding (empty) list
        before = p.lv.read()
        ctx.nif_reset()
        assert p.p.results(tb([])) == OK                         # the reset dropped the list
        assert p.p.run() == (OK, NOOP, len(value))
        assert p.lv.read() == before
        p.m.reset()
        assert p.step(value) in (NOOP, WRITTEN)
        assert p.lv.read() == before
        assert p.run(value) == (NOOP, 0)
        # a wide namespace gives FALLBACK
        before = p.lv.read()
        for _ in range(66):
            value = upd(inv, value, (A("add"), 7))
        assert ctx.nif_stats()["namespaces_widened"] >= 1
        assert p.p.run() == (FALLBACK, NOOP, 0)
        assert p.p.args() == (FALLBACK, None, 0)
        assert p.lv.read() == before
        # destroying in, out or the context kills the map
        inv2 = ctx.var("orset")
        assert inv2.write(tb(value_of([1, 2], 1))) == OK
        lv2, lv3 = ctx.list_var(inv2), ctx.list_var(inv2)
        a, b = ctx.map(inv2, lv2), ctx.map(inv2, lv3)
        assert a.step(fun)[:2] == (OK, WRITTEN)
        lv3.close()
        with pytest.raises(LaspjError) as ei:
            b.run()
        assert ei.value.status == _lib.E_INVAL
        b.close()
        assert a.run() == (OK, NOOP, 0)
        inv2.close()
        for call in (a.run, a.args, lambda: a.results(tb([]))):
            with pytest.raises(LaspjError) as ei:
                call()
            assert ei.value.status == _lib.E_INVAL
        a.close()
        # create's refusals
        g = ctx.var("gset")
        other = ctx.var("orset")
        lvo = ctx.list_var(other)
        for bad_in, bad_out, code in ((g, lvo, _lib.E_KIND), (inv, lvo, _lib.E_UNSUPPORTED)):
            with pytest.raises(LaspjError) as ei:
                ctx.map(bad_in, bad_out)
            assert ei.value.status == code
        c = ctx.map(other, lvo)
    finally:
        ctx.close()
    with pytest.raises(LaspjError):
        c.run()
    c.close()


def test_readd_by_a_removed_token_is_no_new_input():
    """update/4 is update/3 then the bind's merge (lasp_core.erl:283-312): an add_by_token by
    a token in holds removed, and a remove then an add_by_token of an element's only token
    in one call, leave in as it was — the re-run answers what the model answers, a no-op,
    and out reads as before."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = []
        for e in range(6):
            value = upd(inv, value, (A("add_by_token"), tok(e), e))
        value = upd(inv, value, (A("remove"), 3))
        p = Proc(ctx, inv, lambda x: x + 100)
        assert p.step(value) == WRITTEN
        before = p.lv.read()
        for op in ((A("add_by_token"), tok(3), 3),
                   (A("update"), [(A("remove"), 2), (A("add_by_token"), tok(2), 2)])):
            assert upd(inv, value, op) == value
            assert inv.read() == (OK, tb(value)), op
            assert p.run(value, op) == (NOOP, 0)
            p.check_out(op)
            assert p.lv.read() == before, op
        p.close()
    finally:
        ctx.close()
