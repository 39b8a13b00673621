"""tests/lvar_products_model.py pinned on literals (no GPU): product/7's OR-Set branch
(lasp_core.erl:499-533, lasp_lattice.erl:303-308) and bind/3 (:291-312) of its output into a
pair-keyed list value."""

import random

import lvar_products_model as pm
import update4_model as um
from oracle import etf as oetf
from oracle.terms import Atom

A = Atom
NOOP, WRITTEN, REFUSED = pm.NOOP, pm.WRITTEN, pm.REFUSED


def test_key_order_is_x_major():
    l = [(1, [(b"a", False)]), (2, [(b"b", False)])]
    r = [(7, [(b"p", False)]), (8, [(b"q", False)]), (9, [(b"s", False)])]
    acc = pm.acc_value(l, r)
    assert [k for k, _t in acc] == [(1, 7), (1, 8), (1, 9), (2, 7), (2, 8), (2, 9)]
    assert sorted(k for k, _t in acc) == [k for k, _t in acc]


def test_both_token_runs_are_reversed():
    """3 tokens x 2 tokens: token u * 2 + v is [Cx[2 - u], Cy[1 - v]] — a u/v swap or one run
    left forward gives another list."""
    l = [(1, [(b"a", False), (b"b", False), (b"c", False)])]
    r = [(2, [(b"x", False), (b"y", False)])]
    assert pm.acc_value(l, r) == [((1, 2), [([b"c", b"y"], False), ([b"c", b"x"], False),
                                            ([b"b", b"y"], False), ([b"b", b"x"], False),
                                            ([b"a", b"y"], False), ([b"a", b"x"], False)])]
    assert pm.closed_form(l, r) == pm.acc_value(l, r)


def test_flags_are_ored():
    l = [(1, [(b"a", True), (b"b", False)])]
    r = [(2, [(b"x", False), (b"y", True)])]
    assert pm.acc_value(l, r) == [((1, 2), [([b"b", b"y"], True), ([b"b", b"x"], False),
                                            ([b"a", b"y"], True), ([b"a", b"x"], True)])]


def test_empty_sides_give_the_empty_list():
    v = [(1, [(b"a", False)])]
    assert pm.acc_value([], v) == [] and pm.acc_value(v, []) == [] and pm.acc_value([], []) == []
    assert pm.product([], v, []) == (NOOP, [])
    cur = pm.acc_value(v, v)
    # bind/3 of [] into a non-empty value: not `=:=`, the merge is the value, which inflates
    # itself — WRITTEN with the value as it was
    assert pm.product([], v, cur) == (WRITTEN, cur)
    assert pm.product(v, [], cur) == (WRITTEN, cur)


def test_rerun_after_the_first_write_is_a_noop():
    l = [(1, [(b"a", False)]), (3, [(b"b", True), (b"c", False)])]
    r = [(A("k"), [(b"x", False)])]
    st, out = pm.product(l, r, [])
    assert st == WRITTEN and out == pm.acc_value(l, r)
    assert pm.product(l, r, out) == (NOOP, out)


def test_pair_keyed_refused_bind():
    assert pm.bind(pm.REFUSED_VALUE0, pm.REFUSED_VALUE) == (REFUSED, pm.REFUSED_VALUE0)


def test_a_token_of_two_small_integers_is_string_ext():
    img = oetf.term_to_binary([1, 2])
    assert img == bytes([131, 107, 0, 2, 1, 2])
    # and inside a value: {{X, Y}, [{[1, 2], false}]}
    img = oetf.term_to_binary([((5, 6), [([1, 2], False)])])
    assert bytes([107, 0, 2, 1, 2]) in img
    assert oetf.binary_to_term(img) == [((5, 6), [([1, 2], False)])]


def test_closed_form_is_the_model_on_random_orddicts():
    rng = random.Random(7)
    for _ in range(40):
        def side():
            ks = sorted(rng.sample(range(30), rng.randrange(0, 5)))
            return [(k, [(bytes([65 + t]), rng.random() < 0.3)
                         for t in sorted(rng.sample(range(20), rng.randrange(1, 4)))]) for k in ks]
        l, r = side(), side()
        assert pm.closed_form(l, r) == pm.acc_value(l, r)


def test_random_dataflow_stays_bounded():
    """60 updates over a 12-term pool: statuses WRITTEN and NOOP, never REFUSED."""
    pool = [0, 3, 7, 300, -2, A("a"), A("m"), b"", b"b", (1, 2, 3), (0,), 2 ** 40]
    rng = random.Random(11)
    lval, rval, cur = [], [], []
    seen = {NOOP: 0, WRITTEN: 0, REFUSED: 0}
    k = 0
    for step in range(60):
        side = rng.random() < 0.5
        val = lval if side else rval
        e = pool[rng.randrange(len(pool))]
        kind = rng.random()
        if kind < 0.6:
            k += 1
            op, minted = (A("add"), e), [k.to_bytes(4, "big") + bytes(16)]
        else:
            op, minted = (A("remove"), e), []
        res = um.update4("orset", op, val, minted)
        if res[0] == "ok":
            if side:
                lval = res[1]
            else:
                rval = res[1]
        st, cur = pm.product(lval, rval, cur)
        seen[st] += 1
        if step % 5 == 0:
            st, cur = pm.product(lval, rval, cur)
            seen[st] += 1
    assert seen[WRITTEN] >= 1 and seen[NOOP] >= 1 and seen[REFUSED] == 0, seen
    assert len(cur) <= 144 and pm.counts(cur)[1] <= 5000
