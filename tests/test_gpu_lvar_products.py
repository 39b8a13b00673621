"""Pair-keyed list variables and the resident product/7 (include/laspj.h "pair-keyed list
variables", laspj_lvar_product; lasp_amd/csrc/laspj_lvars.hip k_lp_*, laspj_nif_lvars.hip,
laspj_host.cpp list_walk_pairs) against tests/lvar_products_model.py: product/7's OR-Set branch
(lasp_core.erl:499-533, lasp_lattice.erl:303-308) re-run from two resident variables' cells
and bound with bind/3 (:291-312) into a list of {{X, Y}, [{[Tx, Ty], Bool}]} held on the
device, and the rest of the variable's life through the pair walk."""

import random

import pytest

import lvar_products_model as pm
import lvar_reads_model as lrm
import lvar_waiters_model as lwm
import lvars_model as lm
import update4_model as um
from oracle import etf as oetf
from oracle.terms import Atom

OK, FALLBACK = 0, 1
NOOP, WRITTEN, REFUSED = pm.NOOP, pm.WRITTEN, pm.REFUSED
A = Atom

pytestmark = pytest.mark.gpu


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def upd(var, cur, op):
    """update/4 on the device variable and, with the tokens it minted, on the model."""
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
    assert out.value() == (OK, tb(pm.value(want))), where
    assert out.counts() == pm.counts(want), where


def rerun(out, l, r, lval, rval, cur, where=None):
    """One laspj_lvar_product against the model: its status, then the value."""
    st, new = pm.product(lval, rval, cur)
    assert out.product(l, r) == (OK, st), where
    assert out.read() == (OK, tb(new)), where
    return st, new


# ---- 1. three implementations -----------------------------------------------------------

def test_random_dataflow_three_implementations():
    """48 random updates of l and r; after each re-run the resident product, the model and the
    image path (laspj_list_etf_product + laspj_list_etf_bind on the images read back) agree."""
    ctx = _ctx()
    try:
        # ints, atoms, binaries and tuples that sort before, between and after one another
        pool = [0, 7, 300, -2, A("a"), A("zz"), b"", b"bin", (1, 2, 3), (A("k"), 1, b"x")]
        rng = random.Random(20267)
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.pair_list_var(l)
        lval, rval, cur = [], [], []
        seen = {NOOP: 0, WRITTEN: 0, REFUSED: 0}
        for step in range(48):
            side = rng.random() < 0.5
            v, val = (l, lval) if side else (r, rval)
            kind = rng.random()
            e = pool[rng.randrange(len(pool))]
            if kind < 0.55:
                op = (A("add"), e)
            elif kind < 0.75:
                op = (A("remove"), e)
            else:
                op = (A("add_by_token"), bytes([rng.randrange(256) for _ in range(20)]), e)
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
            va, acc = ctx.list_etf("product", "orset", limg, rimg)
            assert va == OK and acc == tb(pm.acc_value(lval, rval)), step
            vb, stb, img = ctx.list_etf_bind("orset", before, acc)
            assert (vb, stb) == (OK, st), step
            assert out.read()[1] == (img if stb == WRITTEN else before), step
            if step % 7 == 0 or (fresh and cur):
                # a re-run with nothing changed: bind/3's no-op when out is exactly AccValue
                # (always so right after the first write); the model decides otherwise
                st, cur = rerun(out, l, r, lval, rval, cur, step)
                seen[st] += 1
                assert st == NOOP or not fresh, step
        assert seen[WRITTEN] >= 1 and seen[NOOP] >= 1, seen
        assert len(cur) >= 4
    finally:
        ctx.close()


# ---- 2. producer edges ------------------------------------------------------------------

def _side(elems, ntok, every, mirror):
    """elements `elems` with ntok tokens each in term order, tombstones on every `every`-th."""
    out = []
    for i, e in enumerate(elems):
        ks = [4 * e + 3 - k for k in range(ntok)][::-1] if mirror else [4 * e + k for k in range(ntok)]
        out.append((e, [(tok(k), i % every == 0) for k in ks]))
    return out


def _spread(n, N, back):
    """n distinct elements of range(N), evenly spaced (from the far end: back)."""
    es = sorted({(i * N) // n for i in range(n)})
    assert len(es) == n
    return sorted(N - 1 - e for e in es) if back else es


SHAPES = [(1, 1), (1, 65), (65, 1), (63, 64), (64, 64), (3, 257), (257, 3), (2, 1025), (1025, 2),
          (33, 33)]


@pytest.mark.parametrize("nl,nr", SHAPES, ids=[f"{a}x{b}" for a, b in SHAPES])
def test_producer_shape_edges(nl, nr):
    """Wave, block and tile edges of the side pass and the write pass: the namespace holds
    elements neither side holds and elements only one side holds (so the compaction matters
    and the positions cross a 1024-position tile while the held counts stay small), tombstones
    on every 5th element of l and every 7th of r, one token each and 3 x 2 tokens."""
    ctx = _ctx()
    try:
        N = 3 * max(nl, nr, 400)
        for a, b in ((1, 1), (3, 2)):
            where = (nl, nr, a, b)
            l = ctx.var("orset")
            r = l.replica()
            pad = l.replica()
            assert pad.write(tb([(e, [(tok(4 * e), False)]) for e in range(N)])) == OK
            lval = _side(_spread(nl, N, False), a, 5, False)
            rval = _side(_spread(nr, N, True), b, 7, True)
            assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
            out = ctx.pair_list_var(l)
            acc = pm.closed_form(lval, rval)
            if nl * nr <= 130:
                assert acc == pm.acc_value(lval, rval)
            assert out.product(l, r) == (OK, WRITTEN), where
            assert out.read() == (OK, tb(acc)), where
            assert out.counts() == (nl * nr, nl * a * nr * b), where
            assert out.product(l, r) == (OK, NOOP), where
            for v in (out, l, r, pad):
                v.close()
    finally:
        ctx.close()


@pytest.mark.parametrize("n,a", [(1, 1), (33, 2), (65, 3)])
def test_producer_same_handle(n, a):
    """l == r: the square of one variable."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        lval = _side(_spread(n, 1500, False), a, 5, False)
        pad = l.replica()
        assert pad.write(tb([(e, [(tok(4 * e), False)]) for e in range(1500)])) == OK
        assert l.write(tb(lval)) == OK
        out = ctx.pair_list_var(l)
        acc = pm.closed_form(lval, lval)
        if n * n <= 130:
            assert acc == pm.acc_value(lval, lval)
        assert out.product(l, l) == (OK, WRITTEN)
        assert out.read() == (OK, tb(acc))
        assert out.product(l, l) == (OK, NOOP)
    finally:
        ctx.close()


# ---- 3. empty sides ---------------------------------------------------------------------

@pytest.mark.parametrize("which", ["l", "r", "both"])
def test_empty_sides(which):
    """AccValue = [] when a side is empty; bind/3 decides, into an empty and a non-empty out."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        full = [(1, [(tok(1), False)]), (A("b"), [(tok(2), True), (tok(3), False)])]
        assert l.write(tb(full)) == OK and r.write(tb(full)) == OK      # the terms registered
        out0, out1 = ctx.pair_list_var(l), ctx.pair_list_var(l)
        assert out1.product(l, r) == (OK, WRITTEN)
        cur1 = pm.acc_value(full, full)
        lval = [] if which in ("l", "both") else full
        rval = [] if which in ("r", "both") else full
        assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
        assert pm.acc_value(lval, rval) == []
        cur0 = []
        for out, cur in ((out0, cur0), (out1, cur1)):
            st, new = rerun(out, l, r, lval, rval, cur, which)
            assert new == cur
            check(out, new, which)
        # and in a namespace that never saw a term
        e = ctx.var("orset")
        oute = ctx.pair_list_var(e)
        assert oute.product(e, e) == (OK, NOOP) and oute.read() == (OK, tb([]))
    finally:
        ctx.close()


# ---- 4. the rest of the variable's life on pairs -----------------------------------------

def _pair_value():
    l = [(1, [(tok(1), False), (tok(2), False)]), (5, [(tok(3), True)])]
    r = [(A("y"), [(tok(4), False)]), ((0,), [(tok(5), False), (tok(6), True)])]
    return l, r, pm.acc_value(l, r)


def test_foreign_bind_and_write():
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        out = ctx.pair_list_var(l)
        _l, _r, acc = _pair_value()
        cur = []
        for val in (acc[:2], acc[:2], acc, [((9, 9), [([1, 2], False), ([tok(1), 3], True)])]):
            st, cur = pm.bind(cur, val)
            assert out.bind(tb(val)) == (OK, st), val
            check(out, cur)
        assert cur != acc
        # the refused KAT: value0 written, then the bind that must not be written
        assert out.write(tb(pm.REFUSED_VALUE0)) == OK
        check(out, pm.REFUSED_VALUE0)
        assert pm.bind(pm.REFUSED_VALUE0, pm.REFUSED_VALUE)[0] == REFUSED
        assert out.bind(tb(pm.REFUSED_VALUE)) == (OK, REFUSED)
        check(out, pm.REFUSED_VALUE0)
        assert out.write(tb([])) == OK
        check(out, [])
    finally:
        ctx.close()


def test_thresholds():
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        out = ctx.pair_list_var(l)
        _l, _r, acc = _pair_value()
        assert out.write(tb(acc)) == OK
        k0, t0 = acc[0]
        flipped = [(k0, [(t0[0][0], not t0[0][1])] + t0[1:])] + acc[1:]
        forms = {
            "a subset of entries": acc[1:3],
            "a token the value lacks": [(k0, t0 + [([tok(77), tok(4)], False)])],
            "a tombstone flip": flipped,
            "equal": acc,
        }
        for name, th in forms.items():
            for strict in (False, True):
                want = pm.threshold(acc, th, strict)
                assert out.threshold(tb(th), strict) == (OK, want), (name, strict)
        assert pm.threshold(acc, forms["equal"], False) and not pm.threshold(acc, forms["equal"], True)
        assert not pm.threshold(acc, forms["a token the value lacks"], False)
    finally:
        ctx.close()


def test_wait_then_product_recheck():
    """Waiters registered on the product's output fire as the model's reply_to_all fires them,
    in its order, inside the re-run's own call."""
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.pair_list_var(l)
        lval = upd(l, [], (A("add"), 1))
        rval = upd(r, [], (A("add"), A("y")))
        m = lwm.ListReplyModel()
        st, m.value = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN
        # what the value will be after 5 joins l, after 7 joins l, and something never met
        l5 = um.update4("orset", (A("add_by_token"), tok(50), 5), lval, [])[1]
        next5 = pm.acc_value(l5, rval)
        never = [((A("no"), A("y")), [([tok(1), tok(2)], False)])]
        waits = [(next5, False, 11), (m.value, True, 12), (never, False, 13), (next5[:1], True, 14),
                 (m.value, False, 15)]
        for th, strict, wid in waits:
            want = m.wait(th, strict, wid)
            assert out.wait(tb(th), strict, wid) == (OK, want), wid
        assert [w[0] for w in out.waiters()] == [w[0] for w in m.waiting]
        # nothing changed: NOOP, nobody fires
        assert out.product_recheck(l, r) == (OK, NOOP, [], len(m.waiting))
        verd, res, _e, minted = l.update(tb((A("add_by_token"), tok(50), 5)))
        assert (verd, res) == (OK, 0)
        lval = um.update4("orset", (A("add_by_token"), tok(50), 5), lval, minted)[1]
        assert lval == l5
        st, new = pm.product(lval, rval, m.value)
        assert st == WRITTEN
        m.value = new
        fired, _flags = m.write()
        assert fired and m.waiting
        assert out.product_recheck(l, r) == (OK, WRITTEN, fired, len(m.waiting))
        assert out.waiters() == m.listing()
        check(out, new)
    finally:
        ctx.close()


def test_wait_needed_read_and_read_any_across_modes():
    """wait_needed, read and read_any over one pair-keyed and one plain variable of one
    namespace: each variable's threshold is walked in that variable's mode."""
    from lasp_amd import engine
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        pairs, plain = ctx.pair_list_var(l), ctx.list_var(l)
        lval, rval, acc = _pair_value()
        assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
        mp, ml = lrm.ListDv(), lrm.ListDv()
        assert pairs.product(l, r) == (OK, WRITTEN)
        mp.wrote(acc)
        iv = lm.acc_value(lval, lval)
        assert plain.intersection(l, l) == (OK, WRITTEN)
        ml.wrote(iv)
        more_p = acc + [((7, 7), [([tok(8), tok(9)], False)])]
        more_l = iv + [(7, [(tok(8), False)])]
        # lazy threads: unmet thresholds are kept, met ones answer at once
        for d, m, th, wid in ((pairs, mp, more_p, 21), (pairs, mp, acc[:1], 22),
                              (plain, ml, more_l, 23), (plain, ml, iv[:1], 24)):
            want = m.wait_needed(th, False, wid)
            assert d.wait_needed(tb(th), False, wid) is want, wid
        assert pairs.lazy() == mp.lazy_listing() and plain.lazy() == ml.lazy_listing()
        # read/6 on the pair-keyed one: met, and one that blocks and fires the lazy thread
        for th, strict, rid in ((acc[:2], False, 31), (more_p, False, 32)):
            want = mp.read(th, strict, rid)
            assert pairs.read(tb(th), strict, rid) == want, rid
        assert pairs.lazy() == mp.lazy_listing() and pairs.waiters() == mp.listing()
        # read_any over both modes: unmet on the pair-keyed one first, met on the plain one
        reads = [(mp, never_p(), False), (ml, iv[:1], False)]
        want = lrm.read_any(reads, 41)
        got = engine.list_read_any([(pairs, tb(never_p()), False), (plain, tb(iv[:1]), False)], 41)
        assert got == want and want[0] == 1
        # and none met: both block
        reads = [(ml, more_l, False), (mp, never_p(), True)]
        want = lrm.read_any(reads, 42)
        got = engine.list_read_any([(plain, tb(more_l), False), (pairs, tb(never_p()), True)], 42)
        assert got == want and want[0] == -1
        assert pairs.waiters() == mp.listing() and plain.waiters() == ml.listing()
        assert pairs.lazy() == mp.lazy_listing() and plain.lazy() == ml.lazy_listing()
        # a pair image as the plain variable's threshold is walked in plain mode: {9, 9} is
        # one key there and [T, T] one token (the plain walk takes any terms)
        th = [((9, 9), [([tok(1), tok(2)], False)])]
        assert plain.threshold(tb(th), False) == (OK, lm.threshold(iv, th, False))
    finally:
        ctx.close()


def never_p():
    return [((A("no"), A("no")), [([tok(90), tok(91)], False)])]


# ---- 5. refusals --------------------------------------------------------------------------

REFUSED_IMAGES = {
    "a key that is no tuple": [(1, [([tok(1), tok(2)], False)])],
    "a 3-tuple key": [((1, 2, 3), [([tok(1), tok(2)], False)])],
    "a token that is a binary": [((1, 2), [(tok(1), False)])],
    "a 3-element token list": [((1, 2), [([tok(1), tok(2), tok(3)], False)])],
}


def _improper() -> bytes:
    """[{{1, 2}, [{[T1, T2], false}]} | 0]"""
    entry = tb(((1, 2), [([tok(1), tok(2)], False)]))[1:]
    return b"\x83\x6c\x00\x00\x00\x01" + entry + tb(0)[1:]


def test_pair_walk_refusals():
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        out = ctx.pair_list_var(l)
        _l, _r, acc = _pair_value()
        assert out.write(tb(acc)) == OK
        before = out.read()
        images = {k: tb(v) for k, v in REFUSED_IMAGES.items()}
        images["an improper list"] = _improper()
        for name, img in images.items():
            s0 = ctx.nif_stats()
            assert out.bind(img) == (FALLBACK, NOOP), name
            assert out.threshold(img, False) == (FALLBACK, None), name
            assert out.wait(img, False, 5) == (FALLBACK, None), name
            assert out.wait_needed(img, False, 6) is None, name
            s1 = ctx.nif_stats()
            assert s1["registrations"] == s0["registrations"], name
            assert s1["dict_elements"] == s0["dict_elements"], name
            assert s1["fallbacks"] == s0["fallbacks"] + 4, name
            assert out.read() == before and out.waiters() == [] and out.lazy() == [], name
        # a refused write is held: read answers it byte for byte, the other calls FALLBACK
        for name, img in images.items():
            held = ctx.pair_list_var(l)
            assert held.write(img) == FALLBACK, name
            assert held.read() == (OK, img) and not held.resident, name
            assert held.bind(tb(acc)) == (FALLBACK, NOOP), name
            assert held.write(tb(acc)) == OK and held.read() == before, name
            held.close()
    finally:
        ctx.close()


def test_cross_mode_and_namespace_refusals():
    from lasp_amd import _lib
    from lasp_amd._lib import LaspjError
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        lval, rval, acc = _pair_value()
        assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
        pairs, plain = ctx.pair_list_var(l), ctx.list_var(l)
        assert pairs.product(l, r) == (OK, WRITTEN)
        # product into a plain list variable, intersection into a pair-keyed one
        assert plain.product(l, r) == (FALLBACK, NOOP) and plain.read() == (OK, tb([]))
        assert plain.product_recheck(l, r) == (FALLBACK, NOOP, [], 0)
        assert pairs.intersection(l, r) == (FALLBACK, NOOP)
        assert pairs.intersection_recheck(l, r) == (FALLBACK, NOOP, [], 0)
        check(pairs, acc)
        # l from another namespace
        other = ctx.var("orset")
        assert other.write(tb(lval)) == OK
        assert pairs.product(other, r) == (FALLBACK, NOOP)
        assert pairs.product(l, other) == (FALLBACK, NOOP)
        # a G-Set is no input of this body
        g = ctx.var("gset")
        assert pairs.product(g, r) == (FALLBACK, NOOP)
        check(pairs, acc)
        # map/6 and fold/6 do not write pairs
        for make in (ctx.map, ctx.fold):
            with pytest.raises(LaspjError) as ei:
                make(l, pairs)
            assert ei.value.status == _lib.E_KIND
        # a wide namespace: the list is held on the host, the re-run answers FALLBACK
        before = pairs.read()
        for _ in range(66):
            lval = upd(l, lval, (A("add"), 1))
        assert ctx.nif_stats()["namespaces_widened"] >= 1
        assert pairs.product(l, r) == (FALLBACK, NOOP)
        assert pairs.read() == before and not pairs.resident
    finally:
        ctx.close()


# ---- 6. reset -----------------------------------------------------------------------------

def test_reset_between_reruns():
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        out = ctx.pair_list_var(l)
        lval, rval, _acc = _pair_value()
        assert l.write(tb(lval)) == OK and r.write(tb(rval)) == OK
        st, cur = rerun(out, l, r, lval, rval, [])
        assert st == WRITTEN
        th = cur + [((A("w"), A("y")), [([tok(60), tok(4)], False)])]
        assert out.wait(tb(th), False, 3) == (OK, False)
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
        # the waiter's threshold comes back through the pair walk too
        assert out.recheck() == (OK, [], 1)
        st, cur = rerun(out, l, r, lval, rval, cur)
        check(out, cur)
    finally:
        ctx.close()


# ---- 7. range -----------------------------------------------------------------------------

def test_product_past_the_list_counts_is_refused_on_the_host():
    """65,536 one-token elements on each side: 2^32 entries.  LASPJ_E_RANGE from the host's
    check of the four totals, before anything of that size is allocated; out is unchanged."""
    from lasp_amd import _lib
    from lasp_amd._lib import LaspjError
    ctx = _ctx()
    try:
        l = ctx.var("orset")
        r = l.replica()
        img = tb([(e, [(tok(e), False)]) for e in range(65536)])
        assert l.write(img) == OK and r.write(img) == OK
        out = ctx.pair_list_var(l)
        keep = [((1, 2), [([tok(1), tok(2)], False)])]
        assert out.write(tb(keep)) == OK
        with pytest.raises(LaspjError) as ei:
            out.product(l, r)
        assert ei.value.status == _lib.E_RANGE
        assert out.read() == (OK, tb(keep)) and out.resident
        assert out.counts() == (1, 1)
    finally:
        ctx.close()
