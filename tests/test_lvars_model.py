"""The list-valued variable's model (tests/lvars_model.py) against the oracle's own clauses:
its properties, and the two literals the GPU tests bind — a value bind/3 refuses (found by
the search below, kept as a literal) and a written value whose keys descend."""

import itertools
import random

import lvars_model as lm
from oracle import lattice as olattice
from oracle import orset as oorset
from oracle.terms import Atom, exact_eq

A = Atom

REFUSED_VALUE0, REFUSED_VALUE, DESCENDING = lm.REFUSED_VALUE0, lm.REFUSED_VALUE, lm.DESCENDING


def _orset(rng, elems, p_rm=0.3):
    v = []
    for e in elems:
        if rng.random() < 0.6:
            toks = sorted({bytes([rng.randrange(97, 103)]) for _ in range(rng.randrange(1, 4))})
            v.append((e, [(t, rng.random() < p_rm) for t in toks]))
    return v


def test_rerun_with_unchanged_inputs_is_noop():
    rng = random.Random(5)
    for _ in range(50):
        l, r = _orset(rng, range(8)), _orset(rng, range(8))
        st, out = lm.intersection(l, r, [])
        assert st in (lm.NOOP, lm.WRITTEN)
        assert lm.intersection(l, r, out) == (lm.NOOP, out)


def test_entry_tokens_are_cx_then_cy():
    rng = random.Random(6)
    for _ in range(50):
        l, r = _orset(rng, range(8)), _orset(rng, range(8))
        acc = lm.acc_value(l, r)
        rd, ld = dict(r), dict(l)
        assert [k for k, _ in acc] == [k for k, _ in l if k in rd]
        for k, toks in acc:
            assert exact_eq(toks, ld[k] + rd[k])
        # tombstoned entries of either side are entries all the same
        assert all(k in ld and k in rd for k, _ in acc)


def test_refused_literal():
    merged = oorset.merge(REFUSED_VALUE0, REFUSED_VALUE)
    assert merged == [(1, [(b"c", False)]), (2, [(b"a", False)]), (1, [(b"b", False)])]
    assert not olattice.is_inflation("lasp_orset", REFUSED_VALUE0, merged)
    assert lm.bind(REFUSED_VALUE0, REFUSED_VALUE) == (lm.REFUSED, REFUSED_VALUE0)


def test_search_finds_a_refused_bind():
    """The search that found the literal: two-entry values over keys {1, 2} in any order
    against one-entry values; some pair must be refused, and the literal is among them."""
    toks = [b"a", b"b", b"c"]
    found = []
    for k0, k1 in itertools.permutations((1, 2)):
        v0 = [(k0, [(toks[0], False)]), (k1, [(toks[1], False)])]
        for k in (1, 2):
            v = [(k, [(toks[2], False)])]
            if lm.bind(v0, v)[0] == lm.REFUSED:
                found.append((v0, v))
    assert (REFUSED_VALUE0, REFUSED_VALUE) in found
    # an orddict is never refused
    assert all(v0[0][0] > v0[1][0] for v0, _v in found)


def test_descending_literal_is_written():
    st, out = lm.bind([], DESCENDING)
    assert (st, out) == (lm.WRITTEN, DESCENDING)
    assert [k for k, _ in out] != sorted(k for k, _ in out if isinstance(k, int))
    assert lm.bind(out, DESCENDING) == (lm.NOOP, out)
    assert lm.value(out) == [A("z"), 3]
    assert lm.counts(out) == (3, 4)


def test_thresholds_on_lists():
    v = DESCENDING
    assert lm.threshold(v, []) and lm.threshold(v, [], strict=True)
    assert lm.threshold(v, v) and not lm.threshold(v, v, strict=True)
    assert lm.threshold(v, [(3, [(b"t0", False)])], strict=True)
    assert not lm.threshold(v, [(4, [(b"t0", False)])])
    assert not lm.threshold(v, [(3, [(b"zz", False)])])
