"""tests/list_bodies_model.py against the oracle (oracle/core.py bodies, oracle/lattice.py
predicates, oracle/orset.py value) — CPU only.

Lists are raw items over the hand-made dictionary of the model module (slot 2v = int v,
slot 2v + 1 = float v, equal rank; token 64 e + k = tok_term(k)): the oracle runs on the
terms the items stand for, the model on the items, and the model's output must stand for
the oracle's term exactly (exact_eq: 1 and 1.0 differ, so the key an operation keeps is
pinned).  Shapes: hypothesis lists as tests/test_gpu_lists.py draws them, and seeded lists
of 300 and 1100 entries (600 for the inflation pair, whose oracle is the slowest) with
unsorted and repeated keys, unsorted and repeated tokens and empty token runs.

`equal` and the inflation pair use one slot per rank (int slots): include/laspj.h states
that equal rank is the same term there, and =:= / sets:is_subset would tell 1 from 1.0.
"""

import os

import numpy as np
import pytest
from hypothesis import HealthCheck, given, settings, strategies as st

import list_bodies_model as m
from oracle import core as ocore, lattice as olat, orset as oorset
from oracle.terms import exact_eq

V = 400                                   # key values of the seeded lists
HV = 13                                   # ... of the hypothesis lists (-3..9 there)
SETTINGS = settings(max_examples=60 * int(os.environ.get("LASPJ_SOAK", "1")), deadline=None,
                    suppress_health_check=[HealthCheck.too_slow, HealthCheck.data_too_large])

SLOT = st.integers(min_value=0, max_value=2 * HV - 1)
TOKS = st.lists(st.tuples(st.integers(0, 6), st.booleans()), max_size=5)
OLIST = st.lists(st.tuples(SLOT, TOKS), max_size=10)
GLIST = st.lists(SLOT, max_size=12)


def olist(spec):
    return m.pack([(s, [(64 * s + k) | (m.REMOVED if f else 0) for k, f in ts])
                   for s, ts in spec], False)


def glist(spec):
    return m.pack(list(spec), True)


def ints_only(lst):
    """The same list over int slots only (one slot per rank)."""
    keys, toff, toks = lst
    keys = keys & ~np.uint64(1)
    if toks is not None:
        toks = toks & ~np.uint64(64)
    return keys, toff, toks


# ------------------------------------------------------------------- funs and their tables

def funs(nv):
    def mapf(x):
        return float((int(x) * 7 + 3) % nv) if isinstance(x, int) else int(x) // 2

    def keepf(x):
        return int(x) % 3 == 0 or isinstance(x, float)

    def foldf(x):
        return [[], [x], [x, float(int(x)), (int(x) + 1) % nv]][int(x) % 3]
    return mapf, keepf, foldf


def per_key_tables(nv):
    mapf, keepf, foldf = funs(nv)
    terms = [m.slot_term(s) for s in range(2 * nv)]
    mt = np.asarray([m.key_item(mapf(t)) for t in terms], dtype=np.uint64)
    kt = np.asarray([1 if keepf(t) is True else 0 for t in terms], dtype=np.uint8)
    rows = [[m.key_item(y) for y in foldf(t)] for t in terms]
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    fk = np.asarray([k for r in rows for k in r], dtype=np.uint64)
    return mt, kt, off, fk


def pair_tables(lst, gset, nv):
    """Per-entry tables over a product output: F sees the pair (OR-Set), or — the bodies
    match {X, Causality} before X (lasp_core.erl:467-474) — the first component of a G-Set's
    2-tuple element, whose second one is re-attached."""
    swap = lambda k: (k[1], k[0])                                  # noqa: E731
    same = lambda k: k[0] == k[1]                                  # noqa: E731
    both = lambda k: [k[0], k[1], k[0]]                            # noqa: E731
    terms = [m.key_term(k) for k in np.asarray(lst[0]).tolist()]
    if gset:
        mapf, keepf, foldf = funs(nv)
        mt = [m.key_item((mapf(t[0]), t[1])) for t in terms]
        kt = [1 if keepf(t[0]) is True else 0 for t in terms]
        rows = [[m.key_item((y, t[1])) for y in foldf(t[0])] for t in terms]
        fs = (mapf, keepf, foldf)
    else:
        mt = [m.key_item(swap(t)) for t in terms]
        kt = [1 if same(t) is True else 0 for t in terms]
        rows = [[m.key_item(y) for y in both(t)] for t in terms]
        fs = (swap, same, both)
    off = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint32)
    return fs, (np.asarray(mt, dtype=np.uint64), np.asarray(kt, dtype=np.uint8), off,
                np.asarray([k for r in rows for k in r], dtype=np.uint64))


# ------------------------------------------------------------------- the comparisons

def same(got, want):
    assert exact_eq(m.to_terms(got), want)


def check_unary(kind, lst, fs, tabs, per_entry):
    mapf, keepf, foldf = fs
    mt, kt, off, fk = tabs
    t = m.to_terms(lst)
    same(m.map(lst, mt, per_entry), ocore.map_body(kind, mapf, t))
    same(m.filter(lst, kt, per_entry), ocore.filter_body(kind, keepf, t))
    same(m.fold(lst, off, fk, per_entry), ocore.fold_body(kind, foldf, t))


def check_bodies(a, b, nv, pa=None, pb=None):
    """Every body of one kind on (a, b); the product on (pa, pb) when given (its output is
    |pa| x |pb| entries)."""
    gs = m.is_gset(a)
    kind = "lasp_gset" if gs else "lasp_orset"
    krank, _grank = m.rank_tables(nv)
    ta, tb = m.to_terms(a), m.to_terms(b)
    if gs:
        same(m.concat(a, b), ocore.union_body(kind, ta, tb))
    else:
        same(m.value(a), oorset.value(ta))
    # lists:member is =:= where lists:keyfind is ==: G-Set lists over one slot per rank
    ia, ib = (ints_only(a), ints_only(b)) if gs else (a, b)
    same(m.intersection(ia, ib, krank),
         ocore.intersection_body(kind, m.to_terms(ia), m.to_terms(ib)))
    same(m.intersection(ib, ia, krank),
         ocore.intersection_body(kind, m.to_terms(ib), m.to_terms(ia)))
    if not gs:
        check_unary(kind, a, funs(nv), per_key_tables(nv), False)
    pa, pb = (a, b) if pa is None else (pa, pb)
    p = m.product(pa, pb)
    same(p, ocore.product_body(kind, m.to_terms(pa), m.to_terms(pb)))
    fs, tabs = pair_tables(p, gs, nv)
    check_unary(kind, p, fs, tabs, True)


def canonical(rng, nv, gset):
    """A canonical value over int slots: cells (present, removed), the element order, the
    token-order rows, and the value as a term (an orddict / ordset)."""
    E = 2 * nv
    present = np.zeros(E, dtype=np.uint64)
    removed = np.zeros(E, dtype=np.uint64)
    for v in rng.choice(nv, nv // 2, replace=False).tolist():
        bits = 1 if gset else int(rng.integers(1, 64))            # token slots 0..5
        present[2 * v] = bits
        removed[2 * v] = 0 if gset else bits & int(rng.integers(0, 64))
    order = np.arange(0, E, 2, dtype=np.uint32)
    tord = np.full((E, 64), 0xFF, dtype=np.uint8)
    tord[:, :6] = np.arange(6, dtype=np.uint8)
    term = []
    for v in range(nv):
        p, r = int(present[2 * v]), int(removed[2 * v])
        if p and gset:
            term.append(v)
        elif p:
            term.append((v, [(m.tok_term(k), bool((r >> k) & 1)) for k in range(6)
                             if (p >> k) & 1]))
    return present, removed, order, tord, term


def check_sets(a, nv, seed):
    """from_set and intersection_set: the right side a canonical value."""
    gs = m.is_gset(a)
    kind = "lasp_gset" if gs else "lasp_orset"
    present, removed, order, tord, term = canonical(np.random.default_rng(seed), nv, gs)
    same(m.from_set(present, removed, order, tord, gs), term)
    a = ints_only(a)
    same(m.intersection_set(a, present, removed, tord, gs),
         ocore.intersection_body(kind, m.to_terms(a), term))


def check_predicates(pairs, nv):
    krank, grank = m.rank_tables(nv)
    for p, c in pairs:
        gs = m.is_gset(p)
        kind = "lasp_gset" if gs else "lasp_orset"
        tp, tc = m.to_terms(p), m.to_terms(c)
        assert m.equal(p, c, krank, grank) == exact_eq(tp, tc)
        assert m.is_inflation(p, c, krank, grank) == olat.is_inflation(kind, tp, tc)
        assert m.is_strict_inflation(p, c, krank, grank) == \
            olat.is_strict_inflation(kind, tp, tc)


def inflated(rng, p, nv):
    """A list that inflates p: p's entries in another order, a token appended to some runs,
    new entries in between (keys may repeat p's: keyfind then meets the first)."""
    if m.is_gset(p):
        extra = m.gen(rng, 5, nv, gset=True, ints=True)[0]
        return rng.permutation(np.concatenate([p[0], extra])), None, None
    ents = m.entries(p)
    ents = [(k, ts + ([64 * k + 5] if rng.integers(0, 4) == 0 else [])) for k, ts in ents]
    ents += m.entries(m.gen(rng, 5, nv, ints=True))
    return m.pack([ents[i] for i in rng.permutation(len(ents)).tolist()], False)


def predicate_pairs(rng, a, b, nv):
    """(prev, cur) pairs that answer both ways: unrelated lists, a list and itself, an
    inflation and its reverse, one flag flipped, one token order swapped, an empty side."""
    gs = m.is_gset(a)
    a, b = ints_only(a), ints_only(b)
    up = inflated(rng, a, nv)
    empty = m.pack([], gs)
    pairs = [(a, b), (a, a), (a, up), (up, a), (empty, a), (a, empty), (empty, empty)]
    if not gs and len(a[2]):
        flip = (a[0], a[1], a[2].copy())
        flip[2][-1] ^= np.uint64(m.REMOVED)
        pairs.append((a, flip))
        ents = m.entries(a)
        i = max(range(len(ents)), key=lambda j: len(set(ents[j][1])))
        ents[i] = (ents[i][0], ents[i][1][::-1])
        pairs.append((a, m.pack(ents, False)))
    return pairs


# ------------------------------------------------------------------- hypothesis shapes

@SETTINGS
@given(OLIST, OLIST)
def test_orset_bodies_small(a, b):
    check_bodies(olist(a), olist(b), HV)
    check_sets(olist(a), HV, len(a))


@SETTINGS
@given(GLIST, GLIST)
def test_gset_bodies_small(a, b):
    check_bodies(glist(a), glist(b), HV)
    check_sets(glist(a), HV, len(a))


@SETTINGS
@given(OLIST, OLIST, st.integers(0, 1000))
def test_orset_predicates_small(a, b, seed):
    rng = np.random.default_rng(seed)
    check_predicates(predicate_pairs(rng, olist(a), olist(b), HV), HV)


@SETTINGS
@given(GLIST, GLIST, st.integers(0, 1000))
def test_gset_predicates_small(a, b, seed):
    rng = np.random.default_rng(seed)
    check_predicates(predicate_pairs(rng, glist(a), glist(b), HV), HV)


# ------------------------------------------------------------------- seeded shapes

@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
@pytest.mark.parametrize("n", [300, 1100])
def test_bodies_seeded(n, gs):
    """The product's output is |l| x |r| entries and the oracle appends each of l's rows to
    a growing list, so its right side is short: 300 x 40 and 1100 x 12."""
    rng = np.random.default_rng(n + gs)
    a, b = m.gen(rng, n, V, gset=gs), m.gen(rng, n - 37, V, gset=gs)
    check_bodies(a, b, V, pa=a, pb=m.gen(rng, 40 if n == 300 else 12, V, gset=gs))
    check_sets(a, V, n)


@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
@pytest.mark.parametrize("n", [300, 600])
def test_predicates_seeded(n, gs):
    rng = np.random.default_rng(7 * n + gs)
    a, b = m.gen(rng, n, V, gset=gs, ints=True), m.gen(rng, n, V, gset=gs, ints=True)
    check_predicates(predicate_pairs(rng, a, b, V), V)


def test_fun_table_errors():
    """A failed row, a missing row and nested pairs raise only when the list reaches them."""
    a = olist([(4, [(1, False)]), (6, [])])
    mt = np.arange(8, dtype=np.uint64)
    mt[5] = m.FAILED
    same(m.map(a, mt, False), [(2, [(m.tok_term(1), False)]), (3, [])])
    mt[6] = m.FAILED
    with pytest.raises(m.FunFailed):
        m.map(a, mt, False)
    with pytest.raises(m.TableRange):
        m.map(a, mt[:6], False)
    with pytest.raises(m.FunFailed):
        m.filter(a, [0, 0, 0, 0, 1, 0, 2], False)
    with pytest.raises(m.FunFailed):
        m.fold(a, [0, 0, 0, 0, 0, 1, 1, 2], [3, m.FAILED], False)
    with pytest.raises(m.TableRange):
        m.fold(a, [0, 0, 0, 0, 0, 1], [3], False)
    p = m.product(a, a)
    with pytest.raises(m.Nested):
        m.product(p, a)
    with pytest.raises(m.TableRange):
        m.map(p, np.arange(1 << 10, dtype=np.uint64), False)       # pair keys: per entry only
