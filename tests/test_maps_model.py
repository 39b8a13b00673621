"""The map-process model (tests/maps_model.py) pinned on literals against the oracle's map/6
body (lasp_core.erl:641-667) and bind/3 (:291-312).  No GPU."""

import lvars_model as lm
import maps_model as mm
from oracle import core as ocore
from oracle.terms import Atom

A = Atom
NOOP, WRITTEN, REFUSED = mm.NOOP, mm.WRITTEN, mm.REFUSED


def t(k: int) -> bytes:
    return k.to_bytes(4, "big") + bytes(16)


VALUE = [(1, [(t(1), False)]), (2, [(t(2), True), (t(3), False)]), (5, [(t(4), False)])]


def test_injective_monotone_gives_an_orddict():
    m = mm.MapModel(lambda x: x + 100)
    assert m.run(VALUE, []) == (NOOP, 3, [])                 # nothing evaluated: untouched
    assert m.args(VALUE) == [1, 2, 5]
    st, first, out = m.step(VALUE, [])
    assert (st, first) == (WRITTEN, 3)
    assert out == [(101, [(t(1), False)]), (102, [(t(2), True), (t(3), False)]),
                   (105, [(t(4), False)])]
    assert out == ocore.map_body("lasp_orset", lambda x: x + 100, VALUE)
    assert m.calls == [1, 2, 5]
    assert m.step(VALUE, out) == (NOOP, 0, out)              # F is not asked again
    assert m.calls == [1, 2, 5]


def test_non_injective_keeps_each_inputs_tokens():
    value = [(4, [(t(9), False)]), (5, [(t(2), True)]), (6, [(t(5), False)])]
    m = mm.MapModel(lambda x: x // 2)
    st, _first, out = m.step(value, [])
    assert st == WRITTEN
    # repeated keys, each with its own X's tokens — no orddict
    assert out == [(2, [(t(9), False)]), (2, [(t(2), True)]), (3, [(t(5), False)])]


def test_order_reversing_bound_twice_interleaves():
    """-X gives descending keys; a second bind of a longer AccValue goes through
    orddict:merge as written over lists that are no orddicts."""
    m = mm.MapModel(lambda x: -x)
    v1 = [(1, [(t(1), False)]), (2, [(t(2), False)])]
    st, _f, out = m.step(v1, [])
    assert (st, out) == (WRITTEN, [(-1, [(t(1), False)]), (-2, [(t(2), False)])])
    v2 = v1 + [(3, [(t(3), False)])]
    acc = ocore.map_body("lasp_orset", lambda x: -x, v2)
    assert acc == [(-1, [(t(1), False)]), (-2, [(t(2), False)]), (-3, [(t(3), False)])]
    st, new = lm.bind(out, acc)
    got = m.step(v2, out)
    assert got == (st, 1, new)
    # the reference's interleaving: equal heads pair up, then the rest of the longer list
    assert st == WRITTEN
    assert new == [(-1, [(t(1), False)]), (-2, [(t(2), False)]), (-3, [(t(3), False)])]


def test_refused_literal():
    """lvars_model's REFUSED pair reached through a map: out holds descending keys, F sends
    the one input to key 1 with another token."""
    m = mm.MapModel(lambda x: 1)
    value = [(7, lm.REFUSED_VALUE[0][1])]
    st, first, out = m.step(value, lm.REFUSED_VALUE0)
    assert (st, first, out) == (REFUSED, 1, lm.REFUSED_VALUE0)


def test_refusal_rules():
    # `==`-equal to a registered term under another image
    m = mm.MapModel(float)
    assert m.step([(1, [(t(1), False)])], []) is None and m.refused
    assert m.results == {}
    # 70 one-token elements onto one key
    m = mm.MapModel(lambda x: A("k"))
    value = [(e, [(t(e), False)]) for e in range(70)]
    assert m.step(value, []) is None and m.refused
    # 64 fit
    m = mm.MapModel(lambda x: A("k"))
    assert m.step(value[:64], [])[0] == WRITTEN
    # a term kind the dictionary does not hold
    m = mm.MapModel(lambda x: {"a": x})
    assert m.step(value[:1], []) is None
    # a reset forgets the refusal
    m.reset()
    assert not m.refused and m.pending(value[:2]) == [0, 1]
