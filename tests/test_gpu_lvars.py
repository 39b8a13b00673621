"""List-valued resident variables (include/laspj.h "list-valued resident variables";
lasp_amd/csrc/laspj_lvars.hip, laspj_nif_lvars.hip) against tests/lvars_model.py: intersection/7's
OR-Set branch (lasp_core.erl:559-568, 583) re-run from two resident variables' cells and
bound with bind/3 (:291-312) into a list held on the device, foreign binds, thresholds and
the variable's life with its namespace.  Statuses and read() images are compared with the
model after every step."""

import random

import pytest

import lvars_model as lm
import update4_model as um
from oracle import etf as oetf
from oracle import orset as oorset
from oracle.terms import Atom

OK, FALLBACK = 0, 1
NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
A = Atom
DESCENDING, REFUSED_VALUE, REFUSED_VALUE0 = lm.DESCENDING, lm.REFUSED_VALUE, lm.REFUSED_VALUE0

pytestmark = pytest.mark.gpu


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def upd(var, cur, op):
    """update/4 on the device variable and, with the tokens it minted, on the model
    (tests/update4_model.py: update/3, then the bind's merge with cur)."""
    verd, res, _err, minted = var.update(tb(op))
    assert verd == OK, op
    want = um.update4("orset", op, cur, minted)
    assert (res == 0) == (want[0] == "ok"), op
    return want[1] if want[0] == "ok" else cur


def tok(k: int) -> bytes:
    """A 20-byte token (the length unique/1 mints); k orders them."""
    return k.to_bytes(4, "big") + bytes(16)


def check(out, want, where=None):
    """read, value and counts of the device variable against the model's value."""
    assert out.read() == (OK, tb(want)), where
    assert out.value() == (OK, tb(lm.value(want))), where
    assert out.counts() == lm.counts(want), where


def rerun(out, l, r, lval, rval, cur, where=None):
    """One laspj_lvar_intersection against the model: its status, then the value."""
    st, new = lm.intersection(lval, rval, cur)
    assert out.intersection(l, r) == (OK, st), where
    assert out.read() == (OK, tb(new)), where
    return st, new


def test_random_dataflow_three_implementations():
    """60 random updates of l and r; after each the resident re-run, the model and the image
    path (laspj_list_etf_intersection + laspj_list_etf_bind on the images read back) agree."""
    ctx = _ctx()
    try:
        # ints, atoms, binaries and tuples that sort before, between and after one another
        pool = [0, 3, 7, 300, -2, A("a"), A("m"), A("zz"), b"", b"b", b"bin", (1, 2, 3),
                (A("k"), 1, b"x"), (0,), 2 ** 40, (A("p"), 5)]
        rng = random.Random(20261)
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        lval, rval, cur = [], [], []
        seen = {NOOP: 0, WRITTEN: 0, REFUSED: 0}
        for step in range(60):
            side = rng.random() < 0.5
            v, val = (l, lval) if side else (r, rval)
            kind = rng.random()
            e = pool[rng.randrange(len(pool))]
            if kind < 0.45:
                op = (A("add"), e)
            elif kind < 0.6:
                op = (A("remove"), e)
            elif kind < 0.8:
                op = (A("add_by_token"), bytes([rng.randrange(256) for _ in range(20)]), e)
            else:
                op = (A("add_all"), rng.sample(pool, 3))
            val = upd(v, val, op)
            if side:
                lval = val
            else:
                rval = val
            if step % 3 == 2:
                continue                                  # two updates between some re-runs
            before = out.read()[1]
            fresh = not cur
            st, cur = rerun(out, l, r, lval, rval, cur, step)
            seen[st] += 1
            check(out, cur, step)
            # the image path on the images read back
            (v1, limg), (v2, rimg) = l.read(), r.read()
            assert (v1, v2) == (OK, OK)
            va, acc = ctx.list_etf("intersection", "orset", limg, rimg)
            assert va == OK and acc == tb(lm.acc_value(lval, rval)), step
            vb, stb, img = ctx.list_etf_bind("orset", before, acc)
            assert (vb, stb) == (OK, st), step
            assert out.read()[1] == (img if stb == WRITTEN else before), step
            if step % 7 == 0 or fresh:
                # a re-run with nothing changed: the no-op of bind/3 when out is exactly
                # AccValue (always so right after the first write); a list merged as written
                # may differ from it, and the reference then writes again — the model decides
                st, cur = rerun(out, l, r, lval, rval, cur, step)
                seen[st] += 1
                assert st == NOOP or not fresh, step
        assert seen[WRITTEN] >= 1 and seen[NOOP] >= 1, seen
        assert len(cur) >= 4
    finally:
        ctx.close()


def _shape_values(n, rmode, ntok):
    """l over elements 0 .. n-1 with ntok tokens each (every 5th element tombstoned); r
    holding none / every other one / all of them with its own tokens (every 7th tombstoned)."""
    lval = [(e, [(tok(4 * e + k), e % 5 == 0) for k in range(ntok)]) for e in range(n)]
    held = {"none": [], "alternate": range(0, n, 2), "all": range(n)}[rmode]
    rval = [(e, [(tok(4 * e + 3 - k), e % 7 == 0) for k in range(ntok)][::-1]) for e in held]
    return lval, rval


def _fast_acc(lval, rval):
    """intersection/7's AccValue for orddicts of distinct keys (what the clause-by-clause
    model gives, tests/test_lvars_model.py, without its quadratic keyfind)."""
    rd = dict(rval)
    return [(k, toks + rd[k]) for k, toks in lval if k in rd]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049])
def test_producer_shape_edges(n):
    """Wave, block and 1024-position tile edges of the producer (and two tiles plus one
    position), r holding none / every other / every element, one and three tokens per element,
    tombstones on either side; the fused producer against the two-step composition."""
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        for rmode in ("none", "alternate", "all"):
            for ntok in (1, 3):
                where = (n, rmode, ntok)
                l = ctx.var("orset")
                r = l.replica()
                lval, rval = _shape_values(n, rmode, ntok)
                assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
                out, two = ctx.list_var(l), ctx.list_var(r)
                acc = _fast_acc(lval, rval)
                if n <= 65:
                    assert acc == lm.acc_value(lval, rval)
                want = WRITTEN if acc else NOOP
                assert out.intersection(l, r) == (OK, want), where
                assert out.read() == (OK, tb(acc)), where
                assert out.counts() == lm.counts(acc), where
                assert out.intersection(l, r) == (OK, NOOP), where
                # the composition (from_set, then intersection_set) gives the same items
                ctx.set_tuning(_lib.TUNE_LVAR_PRODUCER, 1)
                try:
                    assert two.intersection(l, r) == (OK, want), where
                finally:
                    ctx.set_tuning(_lib.TUNE_LVAR_PRODUCER, 0)
                assert two.read() == out.read(), where
                # one more token on the last element of both: the rank-indexed re-bind
                lval = upd(l, lval, (A("add"), n - 1))
                if rmode == "all" or (rmode == "alternate" and (n - 1) % 2 == 0):
                    acc2 = _fast_acc(lval, rval)
                    merged = oorset.merge(acc, acc2)
                    assert out.intersection(l, r) == (OK, WRITTEN), where
                    assert out.read() == (OK, tb(merged)), where
                    assert out.value() == (OK, tb(lm.value(merged))), where
                else:
                    assert out.intersection(l, r) == (OK, NOOP), where
                for v in (out, two, l, r):
                    v.close()
    finally:
        ctx.close()


def test_long_token_runs():
    """One element whose 64 token slots are split 40 / 24 between l and r (a 64-token run),
    then one where both hold all 64 (128 tokens: longer than a wave), flags mixed."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        toks = [tok(1000 - 7 * k) for k in range(64)]       # minted out of term order
        lt = sorted(toks[:40])
        rt = sorted(toks[40:])
        lval = [(5, [(t, i % 3 == 0) for i, t in enumerate(lt)]), (9, [(tok(1), False)])]
        rval = [(5, [(t, i % 2 == 0) for i, t in enumerate(rt)])]
        assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN and lm.counts(cur) == (1, 64)
        check(out, cur)
        # both hold all 64 tokens of another element
        allt = sorted(tok(5000 + 13 * ((k * 37) % 64)) for k in range(64))
        lval = lval + [(A("x"), [(t, False) for t in allt])]
        rval = rval + [(A("x"), [(t, i % 4 == 0) for i, t in enumerate(allt)])]
        assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
        st, cur = rerun(out, l, r, lval, rval, cur)
        assert st == WRITTEN and lm.counts(cur) == (2, 64 + 128)
        check(out, cur)
        assert rerun(out, l, r, lval, rval, cur)[0] == NOOP
    finally:
        ctx.close()


def test_l_with_shorter_cells_than_the_namespace():
    """l's cells were sized before r's elements joined the namespace: they are empty beyond."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        lval = [(e, [(tok(e), False)]) for e in range(40)]
        assert l.write(tb(lval)) == OK
        rval = [(e, [(tok(10000 + e), e % 2 == 0)]) for e in range(20, 700)]
        assert r.write(tb(rval)) == OK                    # the namespace grows past l's cells
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN and [k for k, _ in cur] == list(range(20, 40))
        check(out, cur)
        # and the other way round
        out2 = ctx.list_var(r)
        st, cur2 = rerun(out2, r, l, rval, lval, [])
        assert st == WRITTEN and lm.counts(cur2) == (20, 40)
    finally:
        ctx.close()


def _bound(ctx, images):
    """A fresh list variable with the images bound one after another beside the model."""
    peer = ctx.var("orset")
    out = ctx.list_var(peer)
    cur = []
    for v in images:
        st, cur = lm.bind(cur, v)
        assert out.bind(tb(v)) == (OK, st), v
        check(out, cur, v)
    return peer, out, cur


def test_foreign_binds():
    """Images with ascending keys, descending keys, a repeated key and a repeated token;
    statuses 0 / 1 / 2 against the model, the CPU test's literals among them."""
    ctx = _ctx()
    try:
        asc = [(1, [(b"a", False)]), (2, [(b"b", True), (b"c", False)]), (A("k"), [(b"a", False)])]
        rep_key = [(4, [(b"x", False)]), (2, [(b"y", False)]), (4, [(b"z", True)])]
        rep_tok = [(6, [(b"q", False), (b"q", True), (b"p", False)])]
        for images in ([asc, asc], [DESCENDING, DESCENDING, asc], [rep_key, asc, rep_key],
                       [rep_tok, rep_tok, asc], [asc, rep_key, rep_tok, DESCENDING],
                       [[], asc, []]):
            _peer, out, cur = _bound(ctx, images)
            assert out.resident
        # the refused bind: nothing is written
        _peer, out, cur = _bound(ctx, [REFUSED_VALUE0])
        assert lm.bind(cur, REFUSED_VALUE)[0] == REFUSED
        before = out.read()
        assert out.bind(tb(REFUSED_VALUE)) == (OK, REFUSED)
        assert out.read() == before == (OK, tb(REFUSED_VALUE0))
        check(out, REFUSED_VALUE0)
    finally:
        ctx.close()


def test_rerun_after_a_descending_bind():
    """After a foreign state with descending keys the next re-run leaves the rank-indexed
    path (the list merge as written) and still equals the model."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        lval = rval = []
        for e in (3, 7, A("z"), 11):
            lval = upd(l, lval, (A("add"), e))
            rval = upd(r, rval, (A("add"), e))
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN
        st, cur = lm.bind(cur, DESCENDING)
        assert out.bind(tb(DESCENDING)) == (OK, st)
        check(out, cur)
        for k in range(3):
            lval = upd(l, lval, (A("add"), (3, 7, 12)[k]))
            rval = upd(r, rval, (A("add"), 12))
            st, cur = rerun(out, l, r, lval, rval, cur, k)
            check(out, cur, k)
    finally:
        ctx.close()


def test_thresholds_and_writes():
    ctx = _ctx()
    try:
        peer = ctx.var("orset")
        out = ctx.list_var(peer)
        canon = [(1, [(b"a", False)]), (2, [(b"b", True), (b"c", False)])]
        for val in (canon, DESCENDING):
            assert out.write(tb(val)) == OK
            check(out, val)
            cases = [[], val, val[:1], val[1:], [(val[1][0], val[1][1][:1])],
                     [(99, [(b"a", False)])],                       # a key the value lacks
                     [(val[0][0], [(b"nope", False)])],             # a token it lacks
                     val + [(100, [(b"n", False)])]]
            for t in cases:
                for strict in (False, True):
                    want = lm.threshold(val, t, strict)
                    assert out.threshold(tb(t), strict) == (OK, want), (val, t, strict)
            check(out, val)                                         # thresholds change nothing
        # a write replaces the value; then binds go on from it
        assert out.write(tb([])) == OK
        check(out, [])
        assert out.bind(tb(canon)) == (OK, WRITTEN)
        check(out, canon)
    finally:
        ctx.close()


def test_lifecycle_growth_reset_widening():
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        lval = upd(l, [], (A("add_all"), list(range(30))))
        rval = upd(r, [], (A("add_all"), list(range(10, 40))))
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN and lm.counts(cur) == (20, 40)
        # a never-seen element (the images are rebuilt: the tables are derived again)
        for e in (A("new"), 1000):
            lval = upd(l, lval, (A("add"), e))
            assert rerun(out, l, r, lval, rval, cur)[0] == NOOP
            rval = upd(r, rval, (A("add"), e))
            st, cur = rerun(out, l, r, lval, rval, cur)
            assert st == WRITTEN
        # growth past the images' headroom
        rval = upd(r, rval, (A("add_all"), list(range(2000, 2400))))
        lval = upd(l, lval, (A("add"), 2399))
        st, cur = rerun(out, l, r, lval, rval, cur)
        assert st == WRITTEN and cur[-2][0] == 2399
        check(out, cur)
        # a dictionary reset: the list is written out, read is unchanged, the next re-run
        # walks it back in over the fresh dictionary
        before = out.read()
        s0 = ctx.nif_stats()
        ctx.nif_reset()
        assert not out.resident
        assert out.read() == before == (OK, tb(cur))
        lval = upd(l, lval, (A("add"), 15))
        st, cur = rerun(out, l, r, lval, rval, cur)
        assert st == WRITTEN and out.resident
        s1 = ctx.nif_stats()
        assert s1["vars_spilled"] > s0["vars_spilled"] and s1["vars_hydrated"] > s0["vars_hydrated"]
        check(out, cur)
        # (NOOP or WRITTEN again by where the minted token sorts: the model decides)
        st, cur = rerun(out, l, r, lval, rval, cur)
        check(out, cur)
        # an element of l pushed past 64 tokens: the namespace goes wide, the list is held
        # on the host and the re-run answers FALLBACK with the value unchanged
        before = out.read()
        for _ in range(66):
            lval = upd(l, lval, (A("add"), 7))
        assert ctx.nif_stats()["namespaces_widened"] >= 1
        assert out.intersection(l, r) == (FALLBACK, NOOP)
        assert out.read() == before and not out.resident
        assert out.bind(tb(DESCENDING)) == (FALLBACK, NOOP)
        assert out.value() == (FALLBACK, None)
        assert out.threshold(tb([])) == (FALLBACK, None)
        assert out.read() == before
    finally:
        ctx.close()


def test_peer_or_context_gone_first():
    from lasp_amd import _lib
    ctx = _ctx()
    try:
        peer = ctx.var("orset")
        out = ctx.list_var(peer)
        peer.close()                                      # the namespace is shared-owned
        assert out.bind(tb(DESCENDING)) == (OK, WRITTEN)
        check(out, DESCENDING)
        out.close()
        l = ctx.var("orset")
        out = ctx.list_var(l)
        assert out.bind(tb(DESCENDING)) == (OK, WRITTEN)
        g = ctx.var("gset")
        with pytest.raises(_lib.LaspjError) as ex:
            ctx.list_var(g)
        assert ex.value.status == _lib.E_KIND
    finally:
        ctx.close()
    # the context went first: every call answers E_INVAL, destroy still frees
    for call in (out.read, out.value, out.counts, lambda: out.bind(tb([])),
                 lambda: out.write(tb([])), lambda: out.threshold(tb([])),
                 lambda: out.intersection(l, l), lambda: out.resident):
        with pytest.raises(_lib.LaspjError) as ex:
            call()
        assert ex.value.status == _lib.E_INVAL
    out.close()
    l.close()


def test_every_fallback_cause_leaves_out_unchanged():
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        lval = upd(l, [], (A("add_all"), [1, 2, 3]))
        rval = upd(r, [], (A("add_all"), [2, 3, 4]))
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN
        before = out.read()
        f0 = ctx.nif_stats()["fallbacks"]
        # variables of another namespace, of another kind
        other = ctx.var("orset")
        upd(other, [], (A("add_all"), [2, 3]))
        g = ctx.var("gset")
        for a, b in ((other, r), (l, other), (g, r), (l, g)):
            assert out.intersection(a, b) == (FALLBACK, NOOP)
            assert out.read() == before
        # an input held on the host (`==`-equal keys under two images)
        held = l.replica()
        assert held.write(tb([(1, [(b"t", False)]), (1.0, [(b"t", False)])])) == FALLBACK
        assert not held.resident
        assert out.intersection(held, r) == (FALLBACK, NOOP)
        assert out.intersection(l, held) == (FALLBACK, NOOP)
        assert out.read() == before
        # images the walk refuses
        for bad in (tb([1, 2, 3]), tb([(1, [b"t"])]), tb([(1, [(b"t", 3)])]), tb(A("x")),
                    tb([(1, [(bytes([k]), False) for k in range(65)])])):
            assert out.bind(bad) == (FALLBACK, NOOP)
            assert out.threshold(bad) == (FALLBACK, None)
            assert out.read() == before
        assert out.resident
        check(out, cur)
        # out held on the host by a write the walk refused
        bad = tb([1, 2, 3])
        assert out.write(bad) == FALLBACK
        assert not out.resident and out.read() == (OK, bad)
        assert out.intersection(l, r) == (FALLBACK, NOOP)
        assert out.bind(tb(DESCENDING)) == (FALLBACK, NOOP)
        assert out.read() == (OK, bad)
        assert ctx.nif_stats()["fallbacks"] >= f0 + 15
        # until the next write
        assert out.write(tb(cur)) == OK and out.resident
        assert rerun(out, l, r, lval, rval, cur)[0] == NOOP
    finally:
        ctx.close()


def test_readd_by_a_removed_token_is_no_new_input():
    """update/4 is update/3 then the bind's merge (lasp_core.erl:283-312): an add_by_token by
    a token in holds removed, and a remove then an add_by_token of an element's only token
    in one call, leave l as it was — the re-run answers what the model answers, a no-op,
    and out reads as before."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.list_var(l)
        lval, rval = [], []
        for e in range(6):
            lval = upd(l, lval, (A("add_by_token"), tok(e), e))
        for e in range(2, 8):
            rval = upd(r, rval, (A("add_by_token"), tok(100 + e), e))
        lval = upd(l, lval, (A("remove"), 3))
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN and [k for k, _t in cur] == [2, 3, 4, 5]
        before = out.read()
        for op in ((A("add_by_token"), tok(3), 3),
                   (A("update"), [(A("remove"), 4), (A("add_by_token"), tok(4), 4)])):
            assert upd(l, lval, op) == lval
            assert l.read() == (OK, tb(lval)), op
            assert rerun(out, l, r, lval, rval, cur, op) == (NOOP, cur)
            check(out, cur, op)
            assert out.read() == before, op
    finally:
        ctx.close()
