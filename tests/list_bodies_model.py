"""A raw-item reference of the list combinator bodies and predicates (TEST INFRASTRUCTURE).

The CPU oracle (oracle/core.py, oracle/lattice.py) is the authority for what
laspj_list_* computes, but `Acc ++ Values` and lists:keyfind make it quadratic: past
about 1100 entries it is too slow for a test.  This module restates the same reference
bodies item by item over the device's own representation, in one pass each, so the GPU
tests can compare shapes of a quarter of a million items; tests/test_list_bodies_model.py
compares it with the oracle at the sizes the oracle can do.

A list value is (keys u64[n], toff u32[n+1], toks u64[nt]) as laspj_list_upload takes it
(include/laspj.h "list values"); a G-Set list is (keys, None, None).  Key items are
element slots, or LIST_PAIR | x << 31 | y; token items are 64 e + k, or LIST_COMPOUND |
gx << 31 | gy, with LIST_REMOVED as the flag.  Term order and `==` come from the rank
tables krank (per element slot) and grank (per token id): equal rank = `==`.

Nothing here is borrowed from the kernels: no tiles, no hashing of ranks into tables of a
chosen size — keyfind is a Python dict from rank to first index.
"""

import numpy as np

from lasp_amd import _lib

PAIR = _lib.LIST_PAIR
COMPOUND = _lib.LIST_COMPOUND
REMOVED = _lib.LIST_REMOVED
ID = (1 << 31) - 1
FAILED = (1 << 64) - 1           # a fun table's entry for a key on which the fun raised


class FunFailed(Exception):
    """The fun raised on a key of the list: the reference body crashes (E_FUN)."""


class TableRange(Exception):
    """A key of the list has no row in the fun table (E_RANGE)."""


class Nested(Exception):
    """product/7 over product outputs: nested pairs are not representable (E_UNSUPPORTED)."""


# ------------------------------------------------------------------- items <-> entries

def entries(lst):
    """[(key, [token, ...])] (OR-Set) or [key] (G-Set), Python ints, in list order."""
    keys, toff, toks = lst
    ks = np.asarray(keys, dtype=np.uint64).tolist()
    if toff is None:
        return ks
    o = np.asarray(toff).tolist()
    t = np.asarray(toks, dtype=np.uint64).tolist() if toks is not None else []
    return [(k, t[o[i]:o[i + 1]]) for i, k in enumerate(ks)]


def pack(ents, gset):
    """entries -> (keys, toff, toks) arrays ((keys, None, None) for a G-Set list)."""
    if gset:
        return np.asarray(ents, dtype=np.uint64).reshape(-1), None, None
    keys = np.asarray([k for k, _ in ents], dtype=np.uint64).reshape(-1)
    toff = np.zeros(len(ents) + 1, dtype=np.uint32)
    if ents:
        toff[1:] = np.cumsum([len(ts) for _, ts in ents])
    toks = np.asarray([t for _, ts in ents for t in ts], dtype=np.uint64).reshape(-1)
    return keys, toff, toks


def is_gset(lst):
    return lst[1] is None


def key_ord(item, krank):
    """Term order of a key item: a slot by krank; {X, Y} element-wise, after every slot."""
    if item & PAIR:
        return (1, int(krank[(item >> 31) & ID]), int(krank[item & ID]))
    return (0, int(krank[item & ID]))


def tok_ord(item, grank):
    """Term order of a token item, flag ignored: [Tx, Ty] (a list) below binaries."""
    if item & COMPOUND:
        return (0, int(grank[(item >> 31) & ID]), int(grank[item & ID]))
    return (1, int(grank[item & ID]))


def _first_index(keys, krank):
    """lists:keyfind / lists:member over `keys`: rank -> index of the first match."""
    first = {}
    for j, k in enumerate(keys):
        first.setdefault(key_ord(k, krank), j)
    return first


# ------------------------------------------------------------------- bodies

def from_set(present, removed, order, tord, gset):
    """A canonical value's list form (lasp_orset.erl / lasp_gset.erl values are orddicts /
    ordsets): one entry per present element slot, slots in term order (`order`), and per
    entry its present token slots in term order (`tord[e]`, 0xFF-terminated), flag from
    the removed mask.  present / removed: per element slot, 64-bit masks (G-Set: 0 / 1)."""
    out = []
    for e in np.asarray(order).tolist():
        p = int(present[e])
        if not p:
            continue
        if gset:
            out.append(e)
            continue
        rm = int(removed[e])
        ts = []
        for k in np.asarray(tord[e]).tolist():
            if k >= 64:
                break
            if (p >> k) & 1:
                ts.append((64 * e + k) | (REMOVED if (rm >> k) & 1 else 0))
        out.append((e, ts))
    return pack(out, gset)


def value(lst):
    """lasp_orset:value/1 (lasp_orset.erl:67-73): the keys of entries holding at least one
    {_, false} token, in list order, repeats kept."""
    return pack([k for k, ts in entries(lst) if any(not t & REMOVED for t in ts)], True)


def concat(l, r):
    """union/7 body, G-Set branch: LValue ++ RValue (lasp_core.erl:602-627)."""
    return pack(entries(l) + entries(r), True)


def intersection(l, r, krank):
    """intersection/7 body (lasp_core.erl:546-589): per element of L in list order,
    lists:keyfind(X, 1, R) -> {X, Cx ++ Cy} (orset_causal_union, lasp_lattice.erl:311-312);
    G-Set: the elements of L that are lists:member of R (=:=, which is equal rank where
    every rank has one slot, include/laspj.h).  L's key is kept."""
    gs = is_gset(l)
    le, re_ = entries(l), entries(r)
    first = _first_index(re_ if gs else [k for k, _ in re_], krank)
    out = []
    for el in le:
        j = first.get(key_ord(el if gs else el[0], krank))
        if j is None:
            continue
        out.append(el if gs else (el[0], el[1] + re_[j][1]))
    return pack(out, gs)


def intersection_set(l, present, removed, tord, gset):
    """The same body with a canonical right side: keyfind / member of X in R's list form is
    R's cell of X's own slot (distinct slots are distinct terms in a Store's dictionary);
    Cy = the cell's tokens in term order.  A pair key is no element of a set."""
    E = len(present)
    out = []
    for el in entries(l):
        k = el if gset else el[0]
        e = k & ID
        if (k & PAIR) or e >= E or not int(present[e]):
            continue
        if gset:
            out.append(el)
            continue
        p, rm = int(present[e]), int(removed[e])
        cy = []
        for s in np.asarray(tord[e]).tolist():
            if s >= 64:
                break
            if (p >> s) & 1:
                cy.append((64 * e + s) | (REMOVED if (rm >> s) & 1 else 0))
        out.append((k, el[1] + cy))
    return pack(out, gset)


def product(l, r):
    """product/7 body (lasp_core.erl:499-533): l-major {X, Y}; tokens
    orset_causal_product(Cx, Cy) (lasp_lattice.erl:303-308): a foldl that prepends, so both
    runs come out reversed, flag XDeleted orelse YDeleted."""
    gs = is_gset(l)
    out, re_ = [], entries(r)
    for a in entries(l):
        kx = a if gs else a[0]
        for b in re_:
            ky = b if gs else b[0]
            if (kx & PAIR) or (ky & PAIR):
                raise Nested
            key = PAIR | ((kx & ID) << 31) | (ky & ID)
            if gs:
                out.append(key)
                continue
            ts = []
            for x in reversed(a[1]):
                for y in reversed(b[1]):
                    if (x & COMPOUND) or (y & COMPOUND):
                        raise Nested
                    ts.append(COMPOUND | ((x & ID) << 31) | (y & ID) | ((x | y) & REMOVED))
            out.append((key, ts))
    return pack(out, gs)


def _row(key, i, per_entry, ntab):
    """The fun table's row of entry i: its position (per_entry), else its element slot."""
    if not per_entry and key & PAIR:
        raise TableRange
    idx = i if per_entry else key & ID
    if idx >= ntab:
        raise TableRange
    return idx


def map(lst, tab, per_entry):                                    # noqa: A001
    """map/6 body (lasp_core.erl:641-667): {F(X), C} / F(X) in list order."""
    gs = is_gset(lst)
    tab = np.asarray(tab, dtype=np.uint64).tolist()
    out = []
    for i, el in enumerate(entries(lst)):
        v = tab[_row(el if gs else el[0], i, per_entry, len(tab))]
        if v == FAILED:
            raise FunFailed
        out.append(v if gs else (v, el[1]))
    return pack(out, gs)


def filter(lst, keep, per_entry):                                # noqa: A001
    """filter/6 body (lasp_core.erl:681-712): the elements with F(V) =:= true, tombstoned
    ones included; keep: 1 = true, 0 = anything else, 2 = F raised."""
    gs = is_gset(lst)
    keep = np.asarray(keep, dtype=np.uint8).tolist()
    out = []
    for i, el in enumerate(entries(lst)):
        v = keep[_row(el if gs else el[0], i, per_entry, len(keep))]
        if v == 2:
            raise FunFailed
        if v == 1:
            out.append(el)
    return pack(out, gs)


def fold(lst, off, keys, per_entry):
    """fold/6 body (lasp_core.erl:460-486): Acc ++ [{V, C} || V <- F(X)] / Acc ++ F(X);
    F's result of row i is keys[off[i]:off[i + 1]]."""
    gs = is_gset(lst)
    off = np.asarray(off).tolist()
    keys = np.asarray(keys, dtype=np.uint64).tolist()
    out = []
    for i, el in enumerate(entries(lst)):
        row = _row(el if gs else el[0], i, per_entry, len(off) - 1)
        vs = keys[off[row]:off[row + 1]]
        if FAILED in vs:
            raise FunFailed
        out.extend(vs if gs else [(v, el[1]) for v in vs])
    return pack(out, gs)


# ------------------------------------------------------------------- predicates

def equal(a, b, krank, grank):
    """`case Value0 of Value` (lasp_core.erl:292-296): =:= of the two lists — the same
    entries in the same order, each the same key, token run and flags (equal rank is the
    same term in a Store's dictionary, include/laspj.h)."""
    gs = is_gset(a)
    ea, eb = entries(a), entries(b)
    if len(ea) != len(eb):
        return False
    for x, y in zip(ea, eb):
        if gs:
            if key_ord(x, krank) != key_ord(y, krank):
                return False
            continue
        if key_ord(x[0], krank) != key_ord(y[0], krank) or len(x[1]) != len(y[1]):
            return False
        for s, t in zip(x[1], y[1]):
            if tok_ord(s, grank) != tok_ord(t, grank) or (s ^ t) & REMOVED:
                return False
    return True


def is_inflation(prev, cur, krank, grank):
    """is_lattice_inflation (lasp_lattice.erl:137-140 G-Set: sets:is_subset of the two
    from_lists; :153-161 OR-Set: every Prev entry keyfinds — first match — in Cur, and
    ids_inflated :277-285: each of its tokens keyfinds among that entry's, flags ignored)."""
    if is_gset(prev):
        have = {key_ord(k, krank) for k in entries(cur)}
        return all(key_ord(k, krank) in have for k in entries(prev))
    ce = entries(cur)
    first = _first_index([k for k, _ in ce], krank)
    for k, ts in entries(prev):
        j = first.get(key_ord(k, krank))
        if j is None:
            return False
        have = {tok_ord(t, grank) for t in ce[j][1]}
        if any(tok_ord(t, grank) not in have for t in ts):
            return False
    return True


def is_strict_inflation(prev, cur, krank, grank):
    """is_lattice_strict_inflation (lasp_lattice.erl:212-215 G-Set: an inflation whose
    usorts differ; :235-253 OR-Set: ([], Cur) when Cur =/= []; else an inflation with
    DeletedElements — some Prev entry whose Ids =/= the Ids1 of its first match, order and
    flags included — or NewElements, length(Prev) < length(Cur))."""
    if is_gset(prev):
        p = {key_ord(k, krank) for k in entries(prev)}
        c = {key_ord(k, krank) for k in entries(cur)}
        return p <= c and p != c
    pe, ce = entries(prev), entries(cur)
    if not pe and ce:
        return True
    if not is_inflation(prev, cur, krank, grank):
        return False
    first = _first_index([k for k, _ in ce], krank)
    deleted = False
    for k, ts in pe:
        j = first.get(key_ord(k, krank))
        if j is None:
            continue
        us = ce[j][1]
        if len(ts) != len(us) or any(tok_ord(s, grank) != tok_ord(t, grank) or (s ^ t) & REMOVED
                                     for s, t in zip(ts, us)):
            deleted = True
            break
    return deleted or len(pe) < len(ce)


# ------------------------------------------------------------------- the tests' dictionary
# The hand-made dictionary of tests/test_gpu_lists_sorted.py: element slot 2v is the int v
# and slot 2v + 1 the float v, both of rank v (1 == 1.0), so which of two `==` keys an
# operation keeps is visible; token id 64 e + k is the term tok_term(k) whatever e, of
# rank k.  No term dictionary is built: the rank tables are two aranges.

def rank_tables(V):
    """(krank u32[2V], grank u32[64 * 2V]) of V key values."""
    K = 2 * V
    return (np.arange(K, dtype=np.uint32) // 2), np.tile(np.arange(64, dtype=np.uint32), K)


def tok_term(k):
    return b"t%02d" % k + b"\x00" * 17


def slot_term(slot):
    v = slot // 2
    return float(v) if slot & 1 else v


def term_slot(t):
    return 2 * int(t) + (1 if isinstance(t, float) else 0)


def key_term(item):
    if item & PAIR:
        return (slot_term((item >> 31) & ID), slot_term(item & ID))
    return slot_term(item & ID)


def key_item(t):
    if isinstance(t, tuple):
        return PAIR | (term_slot(t[0]) << 31) | term_slot(t[1])
    return term_slot(t)


def token_term(item):
    flag = bool(item & REMOVED)
    if item & COMPOUND:
        return ([tok_term((item >> 31) & 63), tok_term(item & 63)], flag)
    return (tok_term(item & 63), flag)


def to_terms(lst):
    """The Lasp value a list of items stands for under the dictionary above."""
    if is_gset(lst):
        return [key_term(k) for k in entries(lst)]
    return [(key_term(k), [token_term(t) for t in ts]) for k, ts in entries(lst)]


def gen(rng, n, V, gset=False, ints=False, max_tokens=3, ntok=6):
    """A seeded list of n entries: keys unsorted and repeated (drawn from V values, both
    twins unless `ints`), token runs of 0..max_tokens tokens, unsorted and repeated (drawn
    from ntok token terms), any flags."""
    vals = rng.integers(0, V, n)
    keys = (2 * vals + (0 if ints else rng.integers(0, 2, n))).astype(np.uint64)
    if gset:
        return keys, None, None
    cnt = rng.integers(0, max_tokens + 1, n)
    toff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    nt = int(toff[-1])
    toks = (64 * np.repeat(keys, cnt) + rng.integers(0, ntok, nt).astype(np.uint64)) | \
        (rng.integers(0, 2, nt).astype(np.uint64) << np.uint64(63))
    return keys, toff, toks.astype(np.uint64)
