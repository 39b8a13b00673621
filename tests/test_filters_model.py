"""The filter-process model against the oracle's filter/6 body, and the new entry points'
null-handle answers (no GPU)."""

import ctypes
import random

import pytest

import filters_model as fm
from oracle import core as ocore
from oracle import gset as ogset
from oracle import orset as oorset
from oracle.terms import Atom, exact_eq

A = Atom


def _tokens():
    k = [0]

    def mint(_actor):
        k[0] += 1
        return k[0].to_bytes(20, "big")
    return mint


@pytest.mark.parametrize("type_", ["lasp_orset", "lasp_gset"])
def test_lazy_filter_equals_the_body(type_):
    """Over random op sequences the model's lazily evaluated filter — Function called only
    on elements it has not seen — gives filter_body's AccValue with Function applied
    directly, binds as bind/3 does, and never calls Function twice for an element."""
    rng = random.Random(7)
    mint = _tokens()
    elems = list(range(24)) + [A("a"), A("b"), b"bin", (A("a"), 1), (A("a"), 2), (3, 4)]
    fun = lambda v: (v % 3 == 0) if isinstance(v, int) else v == A("a")  # noqa: E731
    m = fm.FilterModel(type_, fun)
    value, out, seen = [], [], []
    merge = oorset.merge if type_ == "lasp_orset" else ogset.merge
    for step in range(120):
        e = rng.choice(elems)
        if type_ == "lasp_orset":
            op = (A("add"), e) if rng.random() < 0.7 else (A("remove"), e)
            res = oorset.update(op, A("x"), value, tokens=mint)
            if res[0] == "ok":
                value = res[1]
        else:
            value = ogset.update((A("add"), e), A("x"), value)[1]
        want_pending = [x for x in m.elements(value)
                        if not any(exact_eq(x, y) for y in seen)]
        assert len(m.pending(value)) == len(want_pending)
        if m.pending(value):
            st, pend, new = m.run(value, out)
            assert (st, new) == (fm.NOOP, out) and pend == len(want_pending)
        st, _first, out2 = m.step(value, out)
        acc = ocore.filter_body(type_, fun, value)
        assert exact_eq(m.acc(value), acc), step
        assert st == (fm.NOOP if exact_eq(out, acc) else fm.WRITTEN)
        assert exact_eq(out2, merge(out, acc) if st else out)
        out = out2
        seen += want_pending
    assert len(seen) == len(m.calls)
    assert len(m.results) == len(m.calls)            # one call per element, ever
    assert len(m.calls) >= 10


def test_gset_pair_elements_share_an_argument():
    m = fm.FilterModel("lasp_gset", lambda v: v == A("a"))
    value = [(A("a"), 1), (A("a"), 2), (A("b"), 1)]
    assert m.args(value) == [A("a"), A("a"), A("b")]
    st, first, out = m.step(value, [])
    assert (st, first) == (fm.WRITTEN, 3) and out == [(A("a"), 1), (A("a"), 2)]


def test_intersection_model():
    assert fm.intersection([1, 2, 3], [2, 3, 4], []) == (fm.WRITTEN, [2, 3])
    assert fm.intersection([1, 2, 3], [2, 3, 4], [2, 3]) == (fm.NOOP, [2, 3])
    assert fm.intersection([1, 2, 3], [2, 3, 4], [2, 3, 9]) == (fm.WRITTEN, [2, 3, 9])


def test_null_handles_answer_inval():
    """laspj_filter_* and laspj_var_intersection on null handles: LASPJ_E_INVAL, no crash,
    no GPU."""
    from lasp_amd import _lib, build
    build.build()
    lib = _lib.load()
    st, verd, pend = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_uint32()
    h = ctypes.c_void_p()
    assert lib.laspj_filter_run(None, ctypes.byref(st), ctypes.byref(pend),
                                ctypes.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_filter_create(None, None, ctypes.byref(h)) == _lib.E_INVAL
    assert lib.laspj_var_intersection(None, None, None, ctypes.byref(st),
                                      ctypes.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_filter_destroy(None) == _lib.E_INVAL
    assert lib.laspj_filter_results(None, None, 0) == _lib.E_INVAL
    assert lib.laspj_filter_run_many(None, 0, None, None, None, None) == _lib.E_INVAL
