"""tests/folds_model.py against the oracle's own fold/6 body and bind/3 (no GPU): the model
the device tests compare with computes what lasp_core.erl:460-486 plus :291-312 compute, and
gives the reference's own known answer (riak_test/lasp_fold_test.erl:59-87).  Also the C
boundary without a device: the five entry points are exported with the signatures _lib
declares, reject null handles, and the engine wraps them."""

import ctypes as C
import random

import pytest

import folds_model as fm
import lvars_model as lm
from oracle import core as ocore
from oracle import etf as oetf
from oracle import orset as oorset
from oracle.terms import Atom

A = Atom
NOOP, WRITTEN, REFUSED = fm.NOOP, fm.WRITTEN, fm.REFUSED


def tok(k: int) -> bytes:
    return k.to_bytes(4, "big") + bytes(16)


def _minter():
    n = [0]

    def mint(_actor):
        n[0] += 1
        return tok(n[0])
    return mint


def _update(value, op, mint):
    st, new = oorset.update(op, A("a"), value, tokens=mint)
    return new if st == "ok" else value


def _fun(x):
    return [x + 1000, x // 2 + 5000, x + 1000][: x % 4]


@pytest.mark.parametrize("seed", range(6))
def test_model_is_fold_body_then_bind(seed):
    rng = random.Random(seed)
    mint = _minter()
    m = fm.FoldModel(_fun)
    value, out, want = [], [], []
    statuses = set()
    for _ in range(120):
        r = rng.random()
        if r < 0.5 and value:
            op = (A("add"), rng.choice(value)[0])
        elif r < 0.8:
            op = (A("add"), rng.randrange(60))
        else:
            op = (A("remove"), rng.choice(value)[0] if value else 0)
        value = _update(value, op, mint)
        got = m.step(value, out)
        assert got is not None
        st, _first, out = got
        # the oracle, with no memory of earlier results
        acc = ocore.fold_body(lm.TYPE, _fun, value)
        assert m.acc(value) == acc
        wst, want = lm.bind(want, acc)
        assert (st, out) == (wst, want)
        statuses.add(st)
    assert WRITTEN in statuses
    assert len(m.calls) == len(set(m.calls))                 # F asked once per element


def test_pending_leaves_out_alone():
    mint = _minter()
    m = fm.FoldModel(lambda x: [x, x])
    value = _update([], (A("add_all"), [1, 2]), mint)
    out = [(9, [(tok(99), False)])]
    assert m.run(value, out) == (NOOP, 2, out)
    assert m.args(value) == [1, 2]


def test_refusals():
    mint = _minter()
    value = _update([], (A("add_all"), list(range(70))), mint)
    for fun in (lambda x: [float(x)], lambda x: [A("k")], lambda x: [x + 100, {1: 2}]):
        m = fm.FoldModel(fun)
        assert m.step(value, []) is None
        assert m.refused and not m.results
    m = fm.FoldModel(lambda x: x)
    m.note_value(value)
    with pytest.raises(TypeError):
        m.evaluate(value)                                    # bad_generator
    # 64 tokens under one key still fit
    m = fm.FoldModel(lambda x: [A("k"), A("k")])
    assert m.step(value[:64], []) is not None


def test_reference_known_answer():
    """riak_test/lasp_fold_test.erl:59-87."""
    mint = _minter()
    m = fm.FoldModel(lambda x: [x, x, x])
    value = _update([], (A("add_all"), [1, 2, 3]), mint)
    st, first, out = m.step(value, [])
    assert (st, first) == (WRITTEN, 3)
    assert lm.value(out) == [1, 1, 1, 2, 2, 2, 3, 3, 3]
    value = _update(value, (A("add_all"), [4, 5, 6]), mint)
    st, first, out = m.step(value, out)
    assert (st, first) == (WRITTEN, 3)
    assert lm.value(out) == [x for x in range(1, 7) for _ in range(3)]
    assert oorset.value(value) == [1, 2, 3, 4, 5, 6]
    assert oetf.binary_to_term(oetf.term_to_binary(out)) == out


# ---- the C boundary, without a device ----------------------------------------------------

NAMES = ("laspj_fold_create", "laspj_fold_destroy", "laspj_fold_run", "laspj_fold_args",
         "laspj_fold_results")


@pytest.fixture(scope="module")
def lib():
    from lasp_amd import _lib, build
    build.build()
    return _lib.load()


def test_entry_points_are_exported_and_reject_null_handles(lib):
    from lasp_amd import _lib
    for name in NAMES:
        assert name in _lib.SIGNATURES, name
        assert getattr(lib, name) is not None, name
    st, verd, pend, cnt = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
    out, olen = C.c_void_p(), C.c_uint64()
    h = C.c_void_p()
    assert lib.laspj_fold_create(None, None, C.byref(h)) == _lib.E_INVAL and not h
    assert lib.laspj_fold_destroy(None) == _lib.E_INVAL
    assert lib.laspj_fold_run(None, C.byref(st), C.byref(pend), C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_fold_args(None, C.byref(out), C.byref(olen), C.byref(cnt),
                               C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_fold_results(None, b"\x83j", 2, C.byref(verd)) == _lib.E_INVAL
    assert lib.laspj_abi_version() == 2           # additive: the version stands


def test_engine_wraps_the_process():
    from lasp_amd import engine
    for name in ("run", "args", "results", "step", "close"):
        assert callable(getattr(engine.NifFold, name)), name
    assert callable(engine.Context.fold)
