"""Resident fold processes (include/laspj.h "resident fold processes"; lasp_amd/csrc/
laspj_lvars.hip k_lf_count / k_lf_write, laspj_nif_folds.hip) against tests/folds_model.py:
fold/6's body (lasp_core.erl:460-486) re-run from a resident OR-Set's cells and bound with
bind/3 (:291-312) into a list-valued variable.  Every case compares status, pending and
verdict, the decoded out.read() (list order, token order, flags), the image byte for byte and
laspj_lvar_counts with the model."""

import random

import pytest

import folds_model as fm
import lvars_model as lm
import update4_model as um
from oracle import etf as oetf
from oracle.terms import Atom

OK, FALLBACK = 0, 1
NOOP, WRITTEN, REFUSED = fm.NOOP, fm.WRITTEN, fm.REFUSED
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
    """A device fold and its model, stepped side by side."""

    def __init__(self, ctx, inv, fun, out=None):
        self.ctx, self.inv, self.fun = ctx, inv, fun
        self.lv = out if out is not None else ctx.list_var(inv)
        self.p = ctx.fold(inv, self.lv)
        self.m = fm.FoldModel(fun)
        self.out = []

    def check_out(self, where=None):
        verd, img = self.lv.read()
        assert verd == OK, where
        assert oetf.binary_to_term(img) == self.out, where
        assert img == tb(self.out), where
        assert self.lv.counts() == lm.counts(self.out), where

    def run(self, value, where=None):
        """One laspj_fold_run against the model's."""
        st, pend, new = self.m.run(value, self.out)
        assert self.p.run() == (OK, st, pend), where
        self.out = new
        return st, pend

    def step(self, value, where=None):
        """NifFold.step against the model's: the status; out compared."""
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


def _fan012(x):
    return [x + 10000, x + 20000][: x % 3]


@pytest.mark.parametrize("n", SIZES)
def test_position_edges(n):
    """Wave, block and 1024-position tile edges; the replica's odd elements make positions
    the producer skips; fan-out 0, 1 or 2 per element."""
    ctx = _ctx()
    try:
        held = [2 * i for i in range(n)]
        extra = [2 * i + 1 for i in range(0, n + 3, 3)]
        inv = ctx.var("orset")
        rep = inv.replica()
        assert rep.write(tb(value_of(extra, 99, 2))) == OK
        value = value_of(held, n)
        if value:
            assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, _fan012)
        st = p.step(value, n)
        assert st == (WRITTEN if n > 1 else NOOP)
        assert [k for k, _t in p.out] == [v for e in held for v in _fan012(e)]
        assert p.run(value, n) == (NOOP, 0)
        if n:
            # one more token on the last element: no fun, one re-run
            calls = len(p.m.calls)
            value = upd(inv, value, (A("add"), held[-1]))
            st, pend = p.run(value, n)
            assert (st, pend) == (WRITTEN if held[-1] % 3 else NOOP, 0)
            p.check_out(n)
            assert len(p.m.calls) == calls
        p.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("where", ["first", "middle", "last"])
@pytest.mark.parametrize("k", [63, 64, 65, 255, 256, 257, 1023, 1025, 2100])
def test_output_entry_edges(k, where):
    """Seventy elements, one of them (three tokens) with fan-out k, the others 0 or 1: the
    entry-parallel writer's strides and its search for an entry's position."""
    ctx = _ctx()
    try:
        wide = {"first": 0, "middle": 35, "last": 69}[where]
        inv = ctx.var("orset")
        value = value_of(list(range(70)), k, 2)
        value[wide] = (wide, [(tok(8 * wide + j), j == 1) for j in (0, 1, 5)])
        assert inv.write(tb(value)) == OK

        def fun(x):
            if x == wide:
                return [100000 + i for i in range(k)]
            return [x + 1000][: x % 2]

        p = Proc(ctx, inv, fun)
        assert p.step(value, (k, where)) == WRITTEN
        keys = [key for key, _t in p.out]
        assert len(keys) == k + sum(x % 2 for x in range(70) if x != wide)
        at = keys.index(100000)
        assert keys[at:at + k] == list(range(100000, 100000 + k))
        assert all(len(t) == 3 for _k, t in p.out[at:at + k])
        assert p.run(value) == (NOOP, 0)
        # a fourth token on the wide element: k tmap rows and one fmapped word change
        value = upd(inv, value, (A("add"), wide))
        passes = ctx.nif_stats()["device_passes"]
        assert p.run(value) == (WRITTEN, 0)
        assert ctx.nif_stats()["device_passes"] == passes + 1    # one device pass
        p.check_out((k, where))
        assert all(len(t) == 4 for _k, t in p.out[at:at + k])
        assert ctx.nif_stats()["fallbacks"] == 0
        p.close()
    finally:
        ctx.close()


def test_fan_out_zero_everywhere():
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(130)), 5)
        assert inv.write(tb(value)) == OK
        e0 = ctx.nif_stats()["dict_elements"]
        p = Proc(ctx, inv, lambda x: [])
        assert p.step(value) == NOOP
        assert p.out == [] and p.lv.read() == (OK, tb([]))
        assert ctx.nif_stats()["dict_elements"] == e0            # nothing registered
        value = upd(inv, value, (A("add"), 3))
        assert p.run(value) == (NOOP, 0)
        p.check_out()
        p.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("g,shared", [(lambda x: x + 10000, True), (lambda x: x, True),
                                      (lambda x: x // 2, False)],
                         ids=["shift", "identity", "div2"])
def test_fan_out_one_is_the_map(g, shared):
    """F(X) = [G(X)] gives byte for byte the image a NifMap with G gives over the same value,
    into a second list variable.  (X div 2: the map reads a variable of its own holding that
    value — of two processes over one variable whose outputs are inputs, each passes the
    tokens the other registered on)"""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        inv2 = inv if shared else ctx.var("orset")
        value = value_of(list(range(300)), 77)
        assert inv.write(tb(value)) == OK
        if not shared:
            assert inv2.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: [g(x)])
        assert p.step(value) == WRITTEN
        lv2 = ctx.list_var(inv2)
        m = ctx.map(inv2, lv2)
        assert m.step(g) == (OK, WRITTEN, 0)
        assert p.lv.read() == lv2.read()
        value = upd(inv, value, (A("add"), 299))
        value = upd(inv, value, (A("remove"), 0))
        if not shared:
            assert inv2.bind(tb(value)) == (OK, WRITTEN)
        st, _pend = p.run(value)
        assert m.run() == (OK, st, 0)
        p.check_out()
        assert p.lv.read() == lv2.read()
        m.close()
        lv2.close()
        p.close()
    finally:
        ctx.close()


def test_reference_known_answer():
    """riak_test/lasp_fold_test.erl:59-87 on the device."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = upd(inv, [], (A("add_all"), [1, 2, 3]))
        p = Proc(ctx, inv, lambda x: [x, x, x])
        assert p.step(value) == WRITTEN
        value = upd(inv, value, (A("add_all"), [4, 5, 6]))
        assert p.step(value) == WRITTEN
        verd, img = p.lv.value()
        assert verd == OK
        assert oetf.binary_to_term(img) == [x for x in range(1, 7) for _ in range(3)]
        verd, img = inv.value()
        assert verd == OK and oetf.binary_to_term(img) == [1, 2, 3, 4, 5, 6]
        p.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("fun", [lambda x: [x + 500] * 3, lambda x: [x // 2],
                                 lambda x: [x, x + 1]], ids=["vvv", "div2", "x_x1"])
@pytest.mark.parametrize("n", [5, 65, 1025])
def test_repeats(fun, n):
    """A V repeated inside one result, one V from two inputs, outputs that are inputs: the
    model decides WRITTEN or REFUSED; no FALLBACK."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(n)), 31 + n, 3)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, fun)
        assert p.step(value, n) == WRITTEN
        assert [k for k, _t in p.out] == [v for e in range(n) for v in fun(e)]
        p.run(value, n)
        p.check_out(n)
        value = upd(inv, value, (A("add"), n - 1))
        value = upd(inv, value, (A("remove"), 0))
        value = upd(inv, value, (A("add"), n // 2))
        p.run(value, n)
        p.check_out(n)
        value = upd(inv, value, (A("add"), n + 7))               # a new element
        p.step(value, n)
        assert ctx.nif_stats()["fallbacks"] == 0
        p.close()
    finally:
        ctx.close()


def _steady(x):
    return [x + 1000, x // 2 + 5000, x + 1000][: x % 4]


def test_steady_steps():
    """Three hundred random update/4 ops on in, each followed by step(fun) and replayed on
    the model with the device's minted tokens; fan-out 0 to 3, repeats at fan-out 3."""
    ctx = _ctx()
    try:
        rng = random.Random(4711)
        inv = ctx.var("orset")
        p = Proc(ctx, inv, _steady)
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
        # (the model decided every status; over repeated keys bind/3 refuses many merges)
        assert seen[WRITTEN] + seen[REFUSED] >= 100, seen
        assert max(len(t) for _k, t in value) >= 4
        assert ctx.nif_stats()["fallbacks"] == 0
        p.close()
    finally:
        ctx.close()


def test_token_the_fold_registered_turns_up_in_the_input():
    """[X div 2] puts 8's tokens under key 4, an input element too; the host does not pass
    such a slot on.  add_by_token then gives element 4 that very token: the device reports it
    unmapped, the host maps every token and the pass runs again inside the call."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(10)), 3, 2)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, lambda x: [x // 2])
        assert p.step(value) == WRITTEN
        t8 = value[8][1][0][0]
        value = upd(inv, value, (A("add_by_token"), t8, 4))
        assert t8 in [t for t, _f in dict(value)[4]]
        passes = ctx.nif_stats()["device_passes"]
        p.step(value)                                            # (the model's status)
        assert ctx.nif_stats()["device_passes"] >= passes + 2    # the pass, and again
        assert ctx.nif_stats()["fallbacks"] == 0
        # a second fold from []: its output is AccValue itself, t8 under keys 4 (from 8) and 2 (from 4)
        q = Proc(ctx, inv, lambda x: [x // 2])
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
    fold's run over the same value: NOOP — and the other way round."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(130)), 23)
        assert inv.write(tb(value)) == OK
        fun = lambda x: [x // 2 + 1000, x + 3000][: 1 + x % 2]   # noqa: E731
        acc = [(v, t) for k, t in value for v in fun(k)]
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
    """The same value through laspj_var_etf_read + laspj_list_etf_args + laspj_list_etf_fold +
    laspj_list_etf_bind gives the same image byte for byte (n = 257)."""
    ctx = _ctx()
    try:
        inv = ctx.var("orset")
        value = value_of(list(range(257)), 41)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, _fan012)
        assert p.step(value) == WRITTEN
        verd, vimg = inv.read()
        assert verd == OK
        verd, aimg = ctx.list_etf("args", "orset", vimg)
        assert verd == OK
        res = tb([_fan012(a) for a in oetf.binary_to_term(aimg)])
        verd, acc = ctx.list_etf("fold", "orset", vimg, res)
        assert verd == OK
        verd, st, img = ctx.list_etf_bind("orset", tb([]), acc)
        assert (verd, st) == (OK, WRITTEN)
        assert p.lv.read() == (OK, img)
        p.close()
    finally:
        ctx.close()


def _bystanders_still_answer(ctx, inv, value):
    """A filter, an update and another fold on the namespace after a refusal: all as the
    oracle says."""
    import filters_model as flm
    value = upd(inv, value, (A("add"), 1))
    out = inv.replica()
    f = ctx.filter(inv, out)
    m = flm.FilterModel("lasp_orset", lambda e: e % 2 == 0)
    st, _first, want = m.step(value, [])
    assert f.step(lambda e: e % 2 == 0) == (OK, st, 0)
    assert out.read() == (OK, tb(want))
    f.close()
    q = Proc(ctx, inv, lambda x: [x + 10000, x + 10000])
    assert q.step(value) == WRITTEN
    q.close()
    return value


# the results' image for three arguments: [[[1 | 2]], [], []] — a V that is an improper list
V_IMPROPER = (b"\x83l\x00\x00\x00\x03" + b"l\x00\x00\x00\x01" + b"l\x00\x00\x00\x01a\x01a\x02"
              + b"j" + b"j" + b"j" + b"j")
# [[1 | 2], [], []] — a result that is an improper list
R_IMPROPER = b"\x83l\x00\x00\x00\x03" + b"l\x00\x00\x00\x01a\x01a\x02" + b"j" + b"j" + b"j"


def test_refusals():
    from lasp_amd import _lib
    from lasp_amd._lib import LaspjError
    ctx = _ctx()
    try:
        # a float V over integer elements: `==`-equal terms under another image
        inv = ctx.var("orset")
        value = value_of(list(range(6)), 2)
        assert inv.write(tb(value)) == OK
        lv = ctx.list_var(inv)
        assert lv.bind(tb([(A("z"), [(tok(1), False)])])) == (OK, WRITTEN)
        before = lv.read()
        p = ctx.fold(inv, lv)
        e0 = ctx.nif_stats()["dict_elements"]
        assert p.step(lambda x: [x + 100, float(x)]) == (FALLBACK, NOOP, 6)
        assert ctx.nif_stats()["dict_elements"] == e0            # rolled back
        assert p.run() == (FALLBACK, NOOP, 0)
        assert p.args() == (FALLBACK, None, 0)
        assert lv.read() == before
        assert ctx.nif_stats()["namespaces_widened"] == 0
        value = _bystanders_still_answer(ctx, inv, value)
        p.close()
        m = fm.FoldModel(lambda x: [x + 100, float(x)])
        assert m.step(value, []) is None
        # seventy elements of one token each, all giving [k]: 70 tokens under one key
        inv2 = ctx.var("orset")
        value2 = value_of(list(range(70)), 8, 1)
        assert inv2.write(tb(value2)) == OK
        lv2 = ctx.list_var(inv2)
        before = lv2.read()
        p2 = ctx.fold(inv2, lv2)
        e0 = ctx.nif_stats()["dict_elements"]
        assert p2.step(lambda x: [A("k")]) == (FALLBACK, NOOP, 70)
        assert ctx.nif_stats()["dict_elements"] == e0
        assert p2.run() == (FALLBACK, NOOP, 0)
        assert lv2.read() == before
        assert ctx.nif_stats()["namespaces_widened"] == 0
        _bystanders_still_answer(ctx, inv2, value2)
        m = fm.FoldModel(lambda x: [A("k")])
        assert m.step(value2, []) is None
        # a V of a term kind the dictionary does not hold (an improper list, [1 | 2])
        inv3 = ctx.var("orset")
        value3 = value_of([1, 2, 3], 4)
        assert inv3.write(tb(value3)) == OK
        lv3 = ctx.list_var(inv3)
        before = lv3.read()
        p3 = ctx.fold(inv3, lv3)
        assert p3.run() == (OK, NOOP, 3)
        assert p3.args()[2] == 3
        e0 = ctx.nif_stats()["dict_elements"]
        # results that are no proper lists: LASPJ_E_INVAL, nothing recorded, the list stays
        for bad in (tb([5, [], []]), R_IMPROPER):
            with pytest.raises(LaspjError) as ei:
                p3.results(bad)
            assert ei.value.status == _lib.E_INVAL
            assert ctx.nif_stats()["dict_elements"] == e0
        assert p3.run() == (OK, NOOP, 3)
        assert p3.args()[2] == 3
        assert p3.results(V_IMPROPER) == FALLBACK
        assert ctx.nif_stats()["dict_elements"] == e0
        assert p3.run() == (FALLBACK, NOOP, 0)
        assert lv3.read() == before
        assert ctx.nif_stats()["namespaces_widened"] == 0
        _bystanders_still_answer(ctx, inv3, value3)
    finally:
        ctx.close()


def test_lifecycle():
    from lasp_amd import _lib
    from lasp_amd._lib import LaspjError
    ctx = _ctx()
    try:
        fun = lambda x: [x + 10000, x + 20000]                   # noqa: E731
        inv = ctx.var("orset")
        value = value_of(list(range(20)), 13, 2)
        assert inv.write(tb(value)) == OK
        p = Proc(ctx, inv, fun)
        assert p.step(value) == WRITTEN
        # two folds and a map on one in
        q = Proc(ctx, inv, lambda x: [x + 30000] * (x % 3))
        assert q.step(value) == WRITTEN
        lvm = ctx.list_var(inv)
        mp = ctx.map(inv, lvm)
        assert mp.step(lambda x: x + 40000) == (OK, WRITTEN, 0)
        # growth between runs: past the images' head-room
        value = upd(inv, value, (A("add_all"), list(range(100, 400))))
        assert p.step(value) == WRITTEN
        assert q.step(value) == WRITTEN
        assert mp.step(lambda x: x + 40000) == (OK, WRITTEN, 0)
        assert oetf.binary_to_term(lvm.read()[1]) == [(k + 40000, t) for k, t in value]
        # results with no outstanding list, and with a wrong length
        with pytest.raises(LaspjError) as ei:
            p.p.results(tb([]))
        assert ei.value.status == _lib.E_INVAL
        value = upd(inv, value, (A("add_all"), [500, 501]))
        assert p.p.run() == (OK, NOOP, 2)
        assert p.p.args()[2] == 2
        with pytest.raises(LaspjError) as ei:
            p.p.results(tb([[1], [2], [3]]))
        assert ei.value.status == _lib.E_INVAL
        assert p.p.results(tb([fun(500), fun(501)])) == OK
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
        # destroying in, out or the context kills the fold
        inv2 = ctx.var("orset")
        assert inv2.write(tb(value_of([1, 2], 1))) == OK
        lv2, lv3 = ctx.list_var(inv2), ctx.list_var(inv2)
        a, b = ctx.fold(inv2, lv2), ctx.fold(inv2, lv3)
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
                ctx.fold(bad_in, bad_out)
            assert ei.value.status == code
        c = ctx.fold(other, lvo)
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
        p = Proc(ctx, inv, lambda x: [x + 100, x + 200][: 1 + x % 2])
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
