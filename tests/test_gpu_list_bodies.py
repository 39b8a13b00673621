"""The list combinator bodies (the tiled producer k_tp_count / k_tp_scan / k_tp_write and its
nine functors), laspj_list_equal and laspj_list_inflation past one 1024-item tile, one
replica, one gridDim.y and one 64-slot hash table — against tests/list_bodies_model.py
everywhere and against the oracle (oracle/core.py, oracle/lattice.py) where a list has at
most 1100 entries (600 for the inflation pair); tests/test_list_bodies_model.py ties the
model to the oracle.  Every comparison is exact.

Lists are raw items over the model module's hand-made dictionary (slot 2v = int v, slot
2v + 1 = float v, equal rank; token 64 e + k = tok_term(k)), so no term dictionary is built
for the large shapes.  laspj_list_from_set has no oracle body (a canonical value's list
form is the value itself): it is compared with the model, whose output the CPU test
compares with the value as a term.
"""

import numpy as np
import pytest

import list_bodies_model as m
from oracle import core as ocore, lattice as olat, orset as oorset
from oracle.terms import exact_eq

pytestmark = pytest.mark.gpu

V = 3000                       # key values: slots 0 .. 2V - 1
K = 2 * V
DROP = 200                     # slots below this: filter drops them (whole tiles of them)
EDGES = [0, 1, 1023, 1024, 1025, 2048, 2049, 3000]          # around the 1024-item tile
ORACLE_MAX, ORACLE_MAX_INFLATION = 1100, 600


class Env:
    pass


def make_env(krank=None):
    from lasp_amd import _lib, engine
    from lasp_amd.orset import context
    e = Env()
    e.ctx, e.lib, e.engine = context(), _lib, engine
    e.krank, e.grank = m.rank_tables(V)
    if krank is not None:
        e.krank = krank
    kr, gr = e.ctx.buffer(4 * K), e.ctx.buffer(4 * 64 * K)
    kr.upload(e.krank)
    gr.upload(e.grank)
    e.order = _lib.ListOrder()
    e.order.krank, e.order.nkeys, e.order.grank, e.order.ntokens = kr.h.value, K, gr.h.value, 64 * K
    e.keep = (kr, gr)
    return e


@pytest.fixture(scope="module")
def env():
    return make_env()


@pytest.fixture(scope="module")
def spread_env():
    """The same dictionary with sparse order labels for ranks (the kernels only compare
    ranks): V ascending labels below 2^31, the first one 0, twins equal.  Dense small ranks
    hardly ever share a keyfind slot; these do, as a dictionary of many terms would."""
    rng = np.random.default_rng(31)
    labels = np.sort(rng.choice((1 << 31) - 1, V, replace=False)).astype(np.uint32)
    labels[0] = 0
    return make_env(np.repeat(labels, 2))


# ------------------------------------------------------------------- host <-> device

def kind_of(env, gs):
    return env.lib.KIND_GSET_LIST if gs else env.lib.KIND_ORSET_LIST


def counts_of(lst):
    return len(lst[0]), (0 if lst[2] is None else len(lst[2]))


def upload(env, lists, gs, cap_e=None, cap_t=None):
    """One batch holding `lists`, a replica each; capacities exactly the longest list's
    unless given (the keyfind tables are sized from them)."""
    ce = max([1] + [counts_of(x)[0] for x in lists]) if cap_e is None else cap_e
    ct = max([1] + [counts_of(x)[1] for x in lists]) if cap_t is None else cap_t
    lb = env.engine.ListBatch(env.ctx, kind_of(env, gs), len(lists), ce, ct)
    for r, x in enumerate(lists):
        lb.upload(*x, replica=r)
    return lb


def fetch(lb, r, cnt):
    """One replica through laspj_list_download, its sizes from an earlier counts() call."""
    from lasp_amd._lib import check
    n, nt = int(cnt[r][0]), int(cnt[r][1])
    keys = np.zeros(max(n, 1), dtype=np.uint64)
    toff = np.zeros(n + 1, dtype=np.uint32)
    toks = np.zeros(max(nt, 1), dtype=np.uint64)
    check(lb.ctx.L.laspj_list_download(lb.ctx.h, lb.h, r, keys.ctypes.data, toff.ctypes.data,
                                       toks.ctypes.data), lb.ctx.h)
    return (keys[:n], None, None) if lb.gset else (keys[:n], toff, toks[:nt])


def assert_same(got, want, what=""):
    assert len(got[0]) == len(want[0]), (what, len(got[0]), len(want[0]))
    assert np.array_equal(got[0], want[0]), (what, "keys")
    if want[1] is not None:
        assert np.array_equal(got[1], want[1]), (what, "toff")
        assert np.array_equal(got[2], want[2]), (what, "tokens")


def assert_batch(lb, wants, what="", replicas=None):
    """counts() of every replica, contents of `replicas` (default: all) against the model."""
    cnt = lb.counts()
    want_cnt = np.asarray([counts_of(w) for w in wants], dtype=np.uint32).reshape(-1, 2)
    assert np.array_equal(cnt, want_cnt), (what, np.flatnonzero((cnt != want_cnt).any(axis=1))[:8])
    for r in range(len(wants)) if replicas is None else replicas:
        assert_same(fetch(lb, r, cnt), wants[r], (what, r))


# ------------------------------------------------------------------- inputs

def tables(rng):
    """Per-key fun tables over the K slots: map's F(X) slot, filter's keep byte (0 below
    DROP), fold's result rows of length 0, 1 and 3."""
    mt = rng.integers(0, K, K).astype(np.uint64)
    kt = rng.integers(0, 2, K).astype(np.uint8)
    kt[:DROP] = 0
    flen = rng.choice([0, 1, 3], K)
    off = np.concatenate([[0], np.cumsum(flen)]).astype(np.uint32)
    fk = rng.integers(0, K, int(off[-1])).astype(np.uint64)
    return mt, kt, off, fk


def table_funs(tabs):
    """The funs the tables tabulate, over terms, for the oracle."""
    mt, kt, off, fk = tabs
    mapf = lambda x: m.slot_term(int(mt[m.term_slot(x)]))                      # noqa: E731
    keepf = lambda x: bool(kt[m.term_slot(x)] == 1)                            # noqa: E731
    foldf = lambda x: [m.slot_term(int(k)) for k in                            # noqa: E731
                       fk[off[m.term_slot(x)]:off[m.term_slot(x) + 1]]]
    return mapf, keepf, foldf


def drop_tiles(lst):
    """The list with every key of tile 0 and of tile 2 (items 0..1023, 2048..3071) moved
    below DROP: filter drops those tiles whole."""
    keys = lst[0].copy()
    for a in (0, 2048):
        keys[a:a + 1024] %= np.uint64(DROP)
    return keys, lst[1], lst[2]


def cells(rng, E, gs, ints=False):
    """A canonical value's cells over E element slots: (present, removed) masks per slot
    (token slots 0..5), about half the slots present."""
    on = rng.integers(0, 2, E).astype(np.uint64)
    if ints:
        on[1::2] = 0
    if gs:
        return on, np.zeros(E, dtype=np.uint64)
    present = on * rng.integers(1, 64, E).astype(np.uint64)
    return present, present & rng.integers(0, 64, E).astype(np.uint64)


def token_orders(rng, E, permuted):
    tord = np.full((E, 64), 0xFF, dtype=np.uint8)
    tord[:, :6] = np.arange(6, dtype=np.uint8)
    if permuted:
        tord[:, :6] = rng.permuted(tord[:, :6], axis=1)
    return tord


def set_batch(env, cs, gs):
    """The device OR-Set / G-Set batch of per-replica cells [(present, removed)]."""
    E = len(cs[0][0])
    b = env.ctx.gset_batch(len(cs), E) if gs else env.ctx.orset_batch(len(cs), E)
    host = np.zeros((len(cs), b.words_per_replica), dtype=np.uint64)
    for r, (p, rm) in enumerate(cs):
        if gs:
            e = np.flatnonzero(p)
            np.bitwise_or.at(host[r], e >> 6, np.uint64(1) << (e & 63).astype(np.uint64))
        else:
            host[r, 0:2 * E:2] = p
            host[r, 1:2 * E:2] = rm
    b.upload(host)
    return b


def device_buffer(env, arr):
    buf = env.ctx.buffer(max(8, arr.nbytes))
    if arr.nbytes:
        buf.upload(arr)
    return buf


# ------------------------------------------------------------------- one op, many replicas

OPS = [("value", False), ("union", True), ("intersection", False), ("intersection", True),
       ("intersection_set", False), ("intersection_set", True), ("map", False), ("map", True),
       ("filter", False), ("filter", True), ("fold", False), ("fold", True),
       ("from_set", False), ("from_set", True)]
OP_IDS = ["%s-%s" % (op, "gset" if gs else "orset") for op, gs in OPS]


def run_op(env, op, gs, lens, seed, permuted=False):
    """`op` over one batch with a replica per item count in `lens`; every replica against
    the model, and against the oracle where its lists are short enough."""
    rng = np.random.default_rng(seed)
    kind = "lasp_gset" if gs else "lasp_orset"
    R = len(lens)
    tabs = tables(rng)
    fs = table_funs(tabs)
    unary = op in ("map", "filter", "fold")
    twins = op not in ("intersection_set",) and not (gs and op == "intersection")
    ls, rs = [], []
    for n in lens:
        nl = n // 3 if op == "union" else n
        x = m.gen(rng, nl, V, gset=gs, ints=not twins)
        ls.append(drop_tiles(x) if unary else x)
        rs.append(m.gen(rng, n - nl if op == "union" else max(0, n // 2 + 3), V, gset=gs,
                        ints=not twins))
    if op in ("from_set", "intersection_set"):
        E = max(lens) + 5 if op == "from_set" else 4000
        cs = [cells(rng, E, gs, ints=op == "intersection_set") for _ in lens]
        tord = token_orders(rng, E, permuted)
        tb = None if gs else device_buffer(env, tord.reshape(-1))
    if op == "from_set":
        # every replica converts the first max(lens) slots of one element order; replica r
        # has cells in its first lens[r] slots only
        n = max(lens)
        order = rng.permutation(E)[:n].astype(np.uint32)
        for r, (p, rm) in enumerate(cs):
            gone = np.ones(E, dtype=bool)
            gone[order[:lens[r]]] = False
            p[gone] = 0
            rm[gone] = 0
        S = set_batch(env, cs, gs)
        got = env.engine.ListBatch.from_set(S, device_buffer(env, order), n, tb)
        want = [m.from_set(p, rm, order, tord, gs) for p, rm in cs]
        assert_batch(got, want, op)
        return
    L = upload(env, ls, gs)
    if op == "value":
        got, want = L.value(), [m.value(x) for x in ls]
        ora = lambda r: oorset.value(m.to_terms(ls[r]))                        # noqa: E731
    elif op == "union":
        got = L.union(upload(env, rs, gs), env.order)
        want = [m.concat(x, y) for x, y in zip(ls, rs)]
        ora = lambda r: ocore.union_body(kind, m.to_terms(ls[r]), m.to_terms(rs[r]))   # noqa: E731
    elif op == "intersection":
        got = L.intersection(upload(env, rs, gs), env.order)
        want = [m.intersection(x, y, env.krank) for x, y in zip(ls, rs)]
        ora = lambda r: ocore.intersection_body(kind, m.to_terms(ls[r]), m.to_terms(rs[r]))  # noqa: E731
    elif op == "intersection_set":
        got = L.intersection_set(set_batch(env, cs, gs), tb)
        want = [m.intersection_set(x, p, rm, tord, gs) for x, (p, rm) in zip(ls, cs)]
        elems = np.arange(E, dtype=np.uint32)
        ora = None if permuted else lambda r: ocore.intersection_body(         # noqa: E731
            kind, m.to_terms(ls[r]), m.to_terms(m.from_set(*cs[r], elems, tord, gs)))
    elif op == "map":
        got, want = L.map(tabs[0], False), [m.map(x, tabs[0], False) for x in ls]
        ora = lambda r: ocore.map_body(kind, fs[0], m.to_terms(ls[r]))         # noqa: E731
    elif op == "filter":
        got, want = L.filter(tabs[1], False), [m.filter(x, tabs[1], False) for x in ls]
        ora = lambda r: ocore.filter_body(kind, fs[1], m.to_terms(ls[r]))      # noqa: E731
    elif op == "fold":
        got = L.fold(tabs[2], tabs[3], False)
        want = [m.fold(x, tabs[2], tabs[3], False) for x in ls]
        ora = lambda r: ocore.fold_body(kind, fs[2], m.to_terms(ls[r]))        # noqa: E731
    if gs or op == "value":
        want = [(w[0], None, None) for w in want]
    assert got.replicas == R
    assert_batch(got, want, op)
    cnt = got.counts()
    for r, n in enumerate(lens):
        if ora is not None and n <= ORACLE_MAX:
            assert exact_eq(m.to_terms(fetch(got, r, cnt)), ora(r)), (op, r)


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("op,gs", OPS, ids=OP_IDS)
def test_tile_edges(env, op, gs, n):
    """One replica whose item count sits on, before and after the tile boundaries (union:
    both sides together, split 1 : 2)."""
    run_op(env, op, gs, [n], 100 + n)


@pytest.mark.parametrize("lens", [(0, 1, 1024, 1025, 2500), (2500, 1025, 0, 1024, 1)],
                         ids=["ascending", "permuted"])
@pytest.mark.parametrize("op,gs", OPS, ids=OP_IDS)
def test_replicas_of_unequal_length(env, op, gs, lens):
    """Five replicas in one batch, from empty to 2500 items (three tiles): a replica's tile
    prefixes, keyfind table and output block are its own."""
    run_op(env, op, gs, list(lens), 7 + lens[0], permuted=True)


PRODUCTS = [(32, 32), (33, 32), (1, 1025), (1025, 1), (0, 5), (5, 0)]


@pytest.mark.parametrize("nl,nr", PRODUCTS)
@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
def test_product_tile_edges(env, gs, nl, nr):
    """product/7 around one tile of output items (32 x 32 = 1024), 0-2 tokens per entry."""
    rng = np.random.default_rng(nl * 31 + nr)
    kind = "lasp_gset" if gs else "lasp_orset"
    a, b = (m.gen(rng, n, V, gset=gs, max_tokens=2) for n in (nl, nr))
    got = upload(env, [a], gs).product(upload(env, [b], gs))
    assert_batch(got, [m.product(a, b)], "product")
    assert exact_eq(m.to_terms(fetch(got, 0, got.counts())),
                    ocore.product_body(kind, m.to_terms(a), m.to_terms(b)))


def test_product_replicas_of_unequal_length(env):
    """Five replicas whose products span 0 to 2550 output items, both kinds."""
    for gs in (False, True):
        rng = np.random.default_rng(55 + gs)
        shapes = [(0, 4), (1, 1), (32, 32), (41, 25), (50, 51)]
        ls = [m.gen(rng, a, V, gset=gs, max_tokens=2) for a, _ in shapes]
        rs = [m.gen(rng, b, V, gset=gs, max_tokens=2) for _, b in shapes]
        for perm in ([0, 1, 2, 3, 4], [4, 3, 0, 2, 1]):
            xs, ys = [ls[i] for i in perm], [rs[i] for i in perm]
            got = upload(env, xs, gs).product(upload(env, ys, gs))
            assert_batch(got, [m.product(x, y) for x, y in zip(xs, ys)], ("product", gs, perm))


@pytest.mark.parametrize("op", ["map", "filter", "product"])
def test_more_than_256_tiles(env, op):
    """k_tp_scan's carry over more than kPT = 256 tiles of one replica: 262 145 items
    (257 tiles), and a 513 x 512 G-Set product (262 656 items)."""
    rng = np.random.default_rng(262145)
    if op == "product":
        a, b = m.gen(rng, 513, V, gset=True), m.gen(rng, 512, V, gset=True)
        got = upload(env, [a], True).product(upload(env, [b], True))
        assert_batch(got, [m.product(a, b)], op)
        return
    tabs = tables(rng)
    x = drop_tiles(m.gen(rng, 262145, V, max_tokens=2))
    L = upload(env, [x], False)
    if op == "map":
        assert_batch(L.map(tabs[0], False), [m.map(x, tabs[0], False)], op)
    else:
        assert_batch(L.filter(tabs[1], False), [m.filter(x, tabs[1], False)], op)


# ------------------------------------------------------------------- more replicas than gridDim.y

BIG_R = 65539                                  # the grids cap y at 65535 and loop
BIG_E = 8


def big_sample():
    s = set(range(64)) | set(range(65500, 65601)) | set(range(BIG_R - 64, BIG_R)) | \
        set(range(0, BIG_R, 97))
    return sorted(r for r in s if r < BIG_R)


def big_lists(env, gs):
    """Two batches of BIG_R lists of 0-3 entries, built by one cell-batch upload and
    laspj_list_from_set each (itself compared here), and the lists as the model has them."""
    rng = np.random.default_rng(65539 + gs)
    b = Env()
    b.gs = gs
    order = np.asarray([1, 0, 2, 3, 5, 4, 6, 7], dtype=np.uint32)      # a term order (twins tie)
    tord = token_orders(rng, BIG_E, True)
    tb = None if gs else device_buffer(env, tord.reshape(-1))
    ob = device_buffer(env, order)
    b.lists, b.batches = [], []
    for _side in range(2):
        nent = rng.integers(0, 4, BIG_R)
        on = (np.argsort(rng.random((BIG_R, BIG_E)), axis=1) < nent[:, None])
        bits = rng.integers(1, 8, (BIG_R, BIG_E)).astype(np.uint64)
        present = on.astype(np.uint64) * (np.uint64(1) if gs else bits)
        removed = np.zeros_like(present) if gs else present & rng.integers(0, 8, present.shape).astype(np.uint64)
        S = set_batch(env, list(zip(present, removed)), gs)
        lb = env.engine.ListBatch.from_set(S, ob, BIG_E, tb)
        lists = [m.from_set(p, rm, order, tord, gs) for p, rm in zip(present, removed)]
        assert_batch(lb, lists, "from_set", big_sample())
        b.lists.append(lists)
        b.batches.append(lb)
        if not _side:
            b.cells, b.set, b.tord, b.tb = list(zip(present, removed)), S, tord, tb
    # per-key tables of BIG_E rows (a row per slot in use)
    flen = np.asarray([0, 1, 3, 1, 0, 3, 1, 3])
    b.tabs = (rng.integers(0, K, BIG_E).astype(np.uint64),
              np.asarray([1, 0, 1, 1, 0, 1, 0, 1], dtype=np.uint8),
              np.concatenate([[0], np.cumsum(flen)]).astype(np.uint32),
              rng.integers(0, K, int(flen.sum())).astype(np.uint64))
    return b


BIG_OPS = ["intersection", "intersection_set", "map", "filter", "fold", "product", "equal",
           "is_inflation", "is_strict_inflation"]


@pytest.fixture(scope="module")
def big_orset(env):
    return big_lists(env, False)


@pytest.fixture(scope="module")
def big_gset(env):
    return big_lists(env, True)


@pytest.mark.parametrize("op", ["value"] + BIG_OPS)
def test_more_replicas_than_grid_y_orset(env, big_orset, op):
    more_replicas_than_grid_y(env, big_orset, op)


@pytest.mark.parametrize("op", ["union"] + BIG_OPS)
def test_more_replicas_than_grid_y_gset(env, big_gset, op):
    more_replicas_than_grid_y(env, big_gset, op)


def more_replicas_than_grid_y(env, big, op):
    """65 539 replicas: blockIdx.y wraps (r += gridDim.y) in the count, write, keyfind-table
    and probe kernels.  counts() and the predicates for every replica, contents for the
    first and last 64, 65 500-65 600 (around the wrap) and every 97th."""
    gs = big.gs
    A, B = big.batches
    la, lb_ = big.lists
    mt, kt, off, fk = big.tabs
    if op == "equal":
        got = A.equal(B, env.order)
        want = [m.equal(x, y, env.krank, env.grank) for x, y in zip(la, lb_)]
        assert np.array_equal(got, np.asarray(want))
        assert 0 < sum(want) < BIG_R
        assert A.equal(A, env.order).all()
        return
    if op in ("is_inflation", "is_strict_inflation"):
        # B against A for every replica (both answers occur), and merge(A, B) against A
        # for the sampled ones
        M = A.merge(B, env.order)
        cnt = M.counts()
        lm = {r: fetch(M, r, cnt) for r in big_sample()}
        f = m.is_inflation if op == "is_inflation" else m.is_strict_inflation
        got = B.is_inflation_of(A, env.order, strict=op != "is_inflation")
        want = [f(x, y, env.krank, env.grank) for x, y in zip(la, lb_)]
        assert np.array_equal(got, np.asarray(want))
        assert 0 < sum(want) < BIG_R
        got = M.is_inflation_of(A, env.order, strict=op != "is_inflation")
        for r, y in lm.items():
            assert bool(got[r]) == f(la[r], y, env.krank, env.grank), r
        return
    if op == "value":
        got, want = A.value(), [m.value(x) for x in la]
    elif op == "union":
        got, want = A.union(B, env.order), [m.concat(x, y) for x, y in zip(la, lb_)]
    elif op == "intersection":
        got = A.intersection(B, env.order)
        want = [m.intersection(x, y, env.krank) for x, y in zip(la, lb_)]
    elif op == "intersection_set":
        got = B.intersection_set(big.set, big.tb)
        want = [m.intersection_set(x, p, rm, big.tord, gs) for x, (p, rm) in zip(lb_, big.cells)]
    elif op == "map":
        got, want = A.map(mt, False), [m.map(x, mt, False) for x in la]
    elif op == "filter":
        got, want = A.filter(kt, False), [m.filter(x, kt, False) for x in la]
    elif op == "fold":
        got, want = A.fold(off, fk, False), [m.fold(x, off, fk, False) for x in la]
    elif op == "product":
        got, want = A.product(B), [m.product(x, y) for x, y in zip(la, lb_)]
    assert_batch(got, want, op, big_sample())


# ------------------------------------------------------------------- keyfind tables under load

def loaded(rng, n, gs):
    """n entries over 200 ranks that occur 5 times or more each (rank 0 among them), in
    both twins, and single ranks for the rest, shuffled: the first match in list order is
    at no particular slot or tile."""
    ranks = np.concatenate([np.repeat(np.arange(200), 5), 200 + np.arange(n - 1000)])
    ranks = rng.permutation(ranks)
    keys = (2 * ranks + (0 if gs else rng.integers(0, 2, n))).astype(np.uint64)
    if gs:
        return keys, None, None
    cnt = rng.integers(0, 4, n)
    toff = np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)
    toks = (64 * np.repeat(keys, cnt) + rng.integers(0, 6, int(toff[-1])).astype(np.uint64)) | \
        (rng.integers(0, 2, int(toff[-1])).astype(np.uint64) << np.uint64(63))
    return keys, toff, toks.astype(np.uint64)


@pytest.mark.parametrize("n", [1024, 2048])
@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
def test_keyfind_first_match_among_repeats(env, gs, n):
    """r (intersection) / cur (inflation) of exactly n = cap_e entries, 200 of whose ranks
    occur five times: keyfind's first match is the table's smallest index of a rank."""
    rng = np.random.default_rng(n + gs)
    kind = "lasp_gset" if gs else "lasp_orset"
    r = loaded(rng, n, gs)
    l = m.gen(rng, 1500, n - 600, gset=gs, ints=gs)          # ranks in and out of r
    Rb = upload(env, [r], gs)
    got = upload(env, [l], gs).intersection(Rb, env.order)
    assert_batch(got, [m.intersection(l, r, env.krank)], "intersection")
    if n <= ORACLE_MAX:
        assert exact_eq(m.to_terms(fetch(got, 0, got.counts())),
                        ocore.intersection_body(kind, m.to_terms(l), m.to_terms(r)))
    # prev: entries of cur at their first occurrence (an inflation), then one entry taken
    # from a later occurrence, with a token its first occurrence lacks
    ce = m.entries(r)
    first = {}
    for j, e in enumerate(ce):
        first.setdefault(m.key_ord(e if gs else e[0], env.krank), j)
    firsts = sorted(first.values())
    pick = [ce[j] for j in rng.permutation(firsts)[:150].tolist()]
    good = m.pack(pick, gs)
    if gs:
        bad = m.pack(pick + [2 * (n + 7)], True)
    else:
        j = next(j for j, e in enumerate(ce) if first[m.key_ord(e[0], env.krank)] != j)
        bad = m.pack(pick + [(ce[j][0], [64 * ce[j][0] + 9])], False)
    for prev in (good, bad):
        P = upload(env, [prev], gs)
        for strict in (False, True):
            f = m.is_strict_inflation if strict else m.is_inflation
            want = f(prev, r, env.krank, env.grank)
            assert bool(Rb.is_inflation_of(P, env.order, strict=strict)[0]) == want
            assert want == (prev is good)


def distinct(rng, n, gs):
    """n entries of n different ranks (rank 0 among them), either twin, 0-3 tokens each."""
    ranks = rng.permutation(V)[:n]
    if 0 not in ranks:
        ranks[int(rng.integers(0, n))] = 0
    lst = m.gen(rng, n, V, gset=gs, ints=gs)
    keys = (2 * ranks + (lst[0] & np.uint64(1)).astype(np.int64)).astype(np.uint64)
    return keys, lst[1], lst[2]


@pytest.mark.parametrize("n", [1024, 2048])
@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
def test_keyfind_tables_at_load_one_half(spread_env, gs, n):
    """Twenty-four replicas whose r / cur hold exactly n = cap_e entries of n different
    ranks each: every table has 2 n slots at load 0.5, so some probe chain runs into the
    table's last slot and goes on at slot 0 (about one table in five has one, whatever the
    hash).  l / prev ask for every rank of r / cur and for ranks it lacks."""
    env = spread_env
    rng = np.random.default_rng(5 * n + gs)
    R = 24
    rs = [distinct(rng, n, gs) for _ in range(R)]
    ls, prevs = [], []
    for r in rs:
        other = m.gen(rng, 300, V, gset=gs, ints=gs)
        ents = m.entries(r) + m.entries(other)
        ls.append(m.pack([ents[i] for i in rng.permutation(len(ents)).tolist()], gs))
        # prev: cur's entries in another order, each with a prefix of its tokens; odd
        # replicas also ask for a rank cur lacks
        ents = [e if gs else (e[0], e[1][:int(rng.integers(0, 4))]) for e in m.entries(r)]
        ents = [ents[i] for i in rng.permutation(n).tolist()][:n - 1]
        if len(prevs) % 2:
            lack = 2 * int(np.setdiff1d(np.arange(V), r[0].astype(np.int64) // 2)[0])
            ents.append(lack if gs else (lack, []))
        prevs.append(m.pack(ents, gs))
    Rb = upload(env, rs, gs)
    assert_batch(upload(env, ls, gs).intersection(Rb, env.order),
                 [m.intersection(l, r, env.krank) for l, r in zip(ls, rs)], "intersection")
    P = upload(env, prevs, gs)
    for strict in (False, True):
        f = m.is_strict_inflation if strict else m.is_inflation
        want = [f(p, c, env.krank, env.grank) for p, c in zip(prevs, rs)]
        assert want == [r % 2 == 0 for r in range(R)]
        assert list(Rb.is_inflation_of(P, env.order, strict=strict)) == want


# ------------------------------------------------------------------- the bound that did not hold

def past_the_bound(rng, n=2500):
    """l repeats, from item 1100 on, a key whose entry of r holds 7 tokens: the output's
    tokens outgrow known_t(l) + known_t(r)."""
    l = m.entries(m.gen(rng, n, V, max_tokens=1))
    hot = 2 * 77
    l = [(hot + int(i % 2), ts) if i >= 1100 and i % 3 else (k, ts) for i, (k, ts) in enumerate(l)]
    r = [(hot, [(64 * hot + k) | (m.REMOVED if k % 2 else 0) for k in range(7)])] + \
        m.entries(m.gen(rng, 40, V, max_tokens=2))
    return m.pack(l, False), m.pack(r, False)


def test_intersection_retry_past_the_host_bound(env):
    """The 2500-entry form of test_orset_list_intersection_past_the_host_bound: the write
    pass finds dst short, dst is re-sized from the counts and the write pass runs again —
    alone, as replica 3 of 5 whose other replicas fit, and once more on the same context."""
    rng = np.random.default_rng(2500)
    l, r = past_the_bound(rng)
    want = m.intersection(l, r, env.krank)
    assert counts_of(want)[1] > counts_of(l)[1] + counts_of(r)[1]
    for _again in range(2):
        got = upload(env, [l], False).intersection(upload(env, [r], False), env.order)
        assert_batch(got, [want], "alone")
    small = [(m.gen(rng, n, V, max_tokens=1), m.gen(rng, 30, V, max_tokens=1))
             for n in (5, 1025, 0, 300)]
    ls = [x for x, _ in small[:3]] + [l] + [small[3][0]]
    rs = [y for _, y in small[:3]] + [r] + [small[3][1]]
    wants = [m.intersection(x, y, env.krank) for x, y in zip(ls, rs)]
    bound = max(counts_of(x)[1] for x in ls) + max(counts_of(y)[1] for y in rs)
    assert all(counts_of(w)[1] <= bound for i, w in enumerate(wants) if i != 3)
    for _again in range(2):
        got = upload(env, ls, False).intersection(upload(env, rs, False), env.order)
        assert_batch(got, wants, "replica 3 of 5")


# ------------------------------------------------------------------- errors outside tile 0

def test_errors_outside_tile_0_then_a_clean_call(env):
    """A fun failure, a short table and nested pairs that only a block past the first sees
    are reported; the same call with good inputs on the same context then answers."""
    E_FUN, E_RANGE, E_UNSUPPORTED = env.lib.E_FUN, env.lib.E_RANGE, env.lib.E_UNSUPPORTED
    rng = np.random.default_rng(1500)
    mt, kt, off, fk = tables(rng)
    lone = K - 1                                       # the last slot, at item 1500 only
    ents = m.entries(m.gen(rng, 2500, V - 1))
    ents[1500] = (lone, [64 * lone + 1])
    x = m.pack(ents, False)
    L = upload(env, [x], False)

    def raises(status, call):
        with pytest.raises(env.lib.LaspjError) as ei:
            call()
        assert ei.value.status == status

    bad = mt.copy()
    bad[lone] = m.FAILED
    raises(E_FUN, lambda: L.map(bad, False))
    assert_batch(L.map(mt, False), [m.map(x, mt, False)], "map")
    bad = kt.copy()
    bad[lone] = 2
    raises(E_FUN, lambda: L.filter(bad, False))
    assert_batch(L.filter(kt, False), [m.filter(x, kt, False)], "filter")
    bad = fk.copy()
    grown = off.copy()
    if off[lone + 1] == off[lone]:                     # give the lone key a row to fail in
        grown[lone + 1:] += 1
        bad = np.insert(fk, int(off[lone]), 0)
    bad[int(grown[lone])] = m.FAILED
    raises(E_FUN, lambda: L.fold(grown, bad, False))
    assert_batch(L.fold(off, fk, False), [m.fold(x, off, fk, False)], "fold")
    # tables one row short of the lone key
    raises(E_RANGE, lambda: L.map(mt[:lone], False))
    raises(E_RANGE, lambda: L.filter(kt[:lone], False))
    raises(E_RANGE, lambda: L.fold(off[:lone + 1], fk, False))
    assert_batch(L.map(mt, False), [m.map(x, mt, False)], "map after E_RANGE")
    # product: the only pair key / compound token lies past the first 1024 output items
    for gs in (False, True):
        a, b = m.gen(rng, 1100, V, gset=gs, max_tokens=1), m.gen(rng, 2, V, gset=gs, max_tokens=1)
        Bb = upload(env, [b], gs)
        nested = a[0].copy()
        nested[600] = m.PAIR | (3 << 31) | 4
        raises(E_UNSUPPORTED, lambda: upload(env, [(nested, a[1], a[2])], gs).product(Bb))
        assert_batch(upload(env, [a], gs).product(Bb), [m.product(a, b)], "product")
    a = m.entries(m.gen(rng, 1100, V, max_tokens=1))
    a[600] = (a[600][0], [m.COMPOUND | (5 << 31) | 6])
    b = m.pack([(8, [64 * 8 + 1]), (10, [64 * 10])], False)
    Bb = upload(env, [b], False)
    raises(E_UNSUPPORTED, lambda: upload(env, [m.pack(a, False)], False).product(Bb))
    a[600] = (a[600][0], [64 * a[600][0] + 2])
    assert_batch(upload(env, [m.pack(a, False)], False).product(Bb),
                 [m.product(m.pack(a, False), b)], "product after a compound token")


# ------------------------------------------------------------------- equal, inflation at 2500

def distinct_runs(rng, n):
    """n entries, 1-3 distinct tokens each, unsorted keys with repeats, int slots."""
    ents = []
    for k in (2 * rng.integers(0, V, n)).tolist():
        ks = rng.permutation(6)[:int(rng.integers(1, 4))].tolist()
        ents.append((k, [(64 * k + t) | (m.REMOVED if rng.integers(0, 2) else 0) for t in ks]))
    return ents


@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
def test_equal_at_2500(env, gs):
    rng = np.random.default_rng(25 + gs)
    ents = distinct_runs(rng, 2500)
    if gs:
        ents = [k for k, _ in ents]
    variants = {"same": list(ents)}
    last = list(ents)
    last[-1] = ents[-1] ^ 2 if gs else (ents[-1][0] ^ 2, ents[-1][1])
    variants["last key"] = last
    variants["one shorter"] = ents[:-1]
    if not gs:
        k, ts = ents[-1]
        variants["last token"] = ents[:-1] + [(k, ts[:-1] + [(ts[-1] & m.REMOVED) | (64 * k + 7)])]
        k, ts = ents[1700]
        variants["one flag"] = ents[:1700] + [(k, [ts[0] ^ m.REMOVED] + ts[1:])] + ents[1701:]
        (k0, t0), (k1, t1) = ents[1301], ents[1302]
        variants["split"] = ents[:1301] + [(k0, t0 + t1[:1]), (k1, t1[1:])] + ents[1303:]
    a = m.pack(ents, gs)
    A = upload(env, [a], gs)
    for name, v in variants.items():
        b = m.pack(v, gs)
        want = m.equal(a, b, env.krank, env.grank)
        assert want == (name == "same"), name
        assert bool(A.equal(upload(env, [b], gs), env.order)[0]) == want, name
        assert bool(upload(env, [b], gs).equal(A, env.order)[0]) == want, name


def both_predicates(env, P, C, prev, cur, what, want=None, want_strict=None):
    for strict, w in ((False, want), (True, want_strict)):
        f = m.is_strict_inflation if strict else m.is_inflation
        model = f(prev, cur, env.krank, env.grank)
        if w is not None:
            assert model == w, (what, strict)
        assert bool(C.is_inflation_of(P, env.order, strict=strict)[0]) == model, (what, strict)


def test_orset_inflation_at_2500(env):
    """is_inflation / is_strict_inflation with a violation or a change that only a late
    block sees (lasp_lattice.erl:153-161, 235-253, 277-285)."""
    rng = np.random.default_rng(2501)
    # distinct ascending keys: one entry's change is the only change, and a merge emits
    # every entry of prev before any other entry of its key, so merge(prev, x) inflates it
    keys = sorted((2 * rng.permutation(V)[:2500]).tolist())
    pe = [(k, ts) for k, (_k, ts) in zip(keys, distinct_runs(rng, 2500))]
    pe = [(k, [(64 * k + (t & 63)) | (t & m.REMOVED) for t in ts]) for k, ts in pe]
    pe[2499] = (pe[2499][0], [64 * pe[2499][0] + 1, 64 * pe[2499][0] + 4])
    prev = m.pack(pe, False)
    P = upload(env, [prev], False)
    new = 2 * int(np.setdiff1d(np.arange(V), np.asarray(keys) // 2)[0])
    x = m.pack(m.entries(m.gen(rng, 900, V, ints=True)) + [(new, [64 * new + 3])], False)
    M = P.merge(upload(env, [x], False), env.order)
    merged = fetch(M, 0, M.counts())
    both_predicates(env, P, M, prev, merged, "merge", True, True)

    def against(ce, what, want, want_strict):
        cur = m.pack(ce, False)
        both_predicates(env, P, upload(env, [cur], False), prev, cur, what, want, want_strict)

    k, ts = pe[2499]
    against(pe[:2499] + [(k, ts[:1])], "a token missing at entry 2499", False, False)
    against(pe[:1300] + pe[1301:], "a key missing at entry 1300", False, False)
    against(pe[:2499] + [(k, [ts[0] ^ m.REMOVED, ts[1]])], "a flag flipped at 2499", True, True)
    against(pe[:2499] + [(k, ts[::-1])], "token order swapped at 2499", True, True)
    against(list(pe), "equal lists", True, False)
    against(pe + [pe[5]], "only np < nc", True, True)
    empty = m.pack([], False)
    Eb = upload(env, [empty], False)
    both_predicates(env, Eb, Eb, empty, empty, "[] -> []", True, False)
    both_predicates(env, Eb, P, empty, prev, "[] -> cur", True, True)
    both_predicates(env, P, Eb, prev, empty, "prev -> []", False, False)
    # cur's capacity below prev's: prev repeats cur's 300 entries
    ce = pe[:300]
    long_prev = m.pack([ce[i] for i in rng.integers(0, 300, 2500).tolist()] + ce, False)
    cur = m.pack(ce, False)
    both_predicates(env, upload(env, [long_prev], False), upload(env, [cur], False), long_prev,
                    cur, "cap_e(cur) < cap_e(prev)", True, False)
    # broadcast: one prev against four curs
    curs = [prev, m.pack(pe[:1300] + pe[1301:], False), merged, m.pack(pe + [pe[5]], False)]
    C = upload(env, curs, False)
    for strict, want in ((False, [True, False, True, True]), (True, [False, False, True, True])):
        f = m.is_strict_inflation if strict else m.is_inflation
        assert [f(prev, c, env.krank, env.grank) for c in curs] == want
        assert list(C.is_inflation_of(P, env.order, strict=strict)) == want


def test_gset_inflation_at_2500(env):
    """sets:is_subset and the usort comparison (lasp_lattice.erl:137-140, 212-215)."""
    rng = np.random.default_rng(2502)
    pk = (2 * rng.permutation(V)[:2400]).tolist()
    pk = pk + pk[:100]                                   # 2500 entries, 100 repeats
    prev = m.pack(pk, True)
    P = upload(env, [prev], True)
    new = 2 * int(np.setdiff1d(np.arange(V), np.asarray(pk) // 2)[0])
    x = m.pack(m.entries(m.gen(rng, 900, V, gset=True, ints=True)) + [new], True)
    M = P.merge(upload(env, [x], True), env.order)
    merged = fetch(M, 0, M.counts())
    both_predicates(env, P, M, prev, merged, "merge", True, True)

    def against(ck, what, want, want_strict):
        cur = m.pack(ck, True)
        both_predicates(env, P, upload(env, [cur], True), prev, cur, what, want, want_strict)

    against([k for k in pk if k != pk[1300]], "a key missing", False, False)
    against(pk[::-1], "the same set, reversed", True, False)
    against(pk[:2400], "the same set, shorter (cap_e below prev's)", True, False)
    against(pk + [pk[7]], "only a repeat more", True, False)
    against(pk + [new], "one new key at the end", True, True)
    empty = m.pack([], True)
    Eb = upload(env, [empty], True)
    both_predicates(env, Eb, Eb, empty, empty, "[] -> []", True, False)
    both_predicates(env, Eb, P, empty, prev, "[] -> cur", True, True)
    both_predicates(env, P, Eb, prev, empty, "prev -> []", False, False)
    curs = [prev, m.pack(pk[1:1300] + pk[1301:], True), merged, m.pack(pk + [new], True)]
    C = upload(env, curs, True)
    for strict in (False, True):
        f = m.is_strict_inflation if strict else m.is_inflation
        want = [f(prev, c, env.krank, env.grank) for c in curs]
        assert want == ([True, False, True, True] if not strict else [False, False, True, True])
        assert list(C.is_inflation_of(P, env.order, strict=strict)) == want


@pytest.mark.parametrize("gs", [False, True], ids=["orset", "gset"])
def test_predicates_against_the_oracle_at_600(env, gs):
    """equal and the inflation pair on unsorted 600-entry lists, three replicas in one batch,
    against oracle/lattice.py directly."""
    rng = np.random.default_rng(600 + gs)
    kind = "lasp_gset" if gs else "lasp_orset"
    a = m.gen(rng, ORACLE_MAX_INFLATION, 250, gset=gs, ints=True)
    b = m.gen(rng, ORACLE_MAX_INFLATION, 250, gset=gs, ints=True)
    A1, B1 = upload(env, [a], gs), upload(env, [b], gs)
    M = A1.merge(B1, env.order)
    mg = fetch(M, 0, M.counts())
    pairs = [(a, b), (a, mg), (mg, a)]
    P = upload(env, [p for p, _ in pairs], gs)
    C = upload(env, [c for _, c in pairs], gs)
    eq = P.equal(C, env.order)
    inf = C.is_inflation_of(P, env.order)
    sinf = C.is_inflation_of(P, env.order, strict=True)
    for r, (p, c) in enumerate(pairs):
        tp, tc = m.to_terms(p), m.to_terms(c)
        assert bool(eq[r]) == exact_eq(tp, tc), r
        assert bool(inf[r]) == olat.is_inflation(kind, tp, tc), r
        assert bool(sinf[r]) == olat.is_strict_inflation(kind, tp, tc), r


# ------------------------------------------------------------------- bind at R = 6

def test_bind_six_replicas_mixed_statuses(env):
    """laspj_list_bind over six replicas (past the R <= 4 fused scan) of unsorted lists of
    up to 600 entries whose statuses come out 0, 1 and 2: the oracle's bind/3
    (lasp_core.erl:291-312)."""
    rng = np.random.default_rng(6)
    pairs = []
    for r in range(6):
        a = m.gen(rng, int(rng.integers(300, 601)), 150, ints=True)
        b = m.gen(rng, int(rng.integers(300, 601)), 150, ints=True)
        if r % 3 == 0:
            b = a                                            # Value0 =:= Value
        elif r % 3 == 1:
            # Value0 with ascending distinct keys: the merge emits all of it
            ents = dict((k, ts) for k, ts in m.entries(a))
            a = m.pack(sorted(ents.items()), False)
        pairs.append((a, b))
    want = []
    for a, b in pairs:
        ta, tb = m.to_terms(a), m.to_terms(b)
        if exact_eq(ta, tb):
            want.append((0, None))
            continue
        mg = oorset.merge(ta, tb)
        want.append((1 if olat.is_inflation("lasp_orset", ta, mg) else 2, mg))
    assert sorted(set(w for w, _ in want)) == [0, 1, 2], [w for w, _ in want]
    P, Vb = upload(env, [a for a, _ in pairs], False), upload(env, [b for _, b in pairs], False)
    merged, status = P.bind(Vb, env.order)
    assert list(status) == [w for w, _ in want]
    cnt = merged.counts()
    for r, (w, mg) in enumerate(want):
        if w:
            assert exact_eq(m.to_terms(fetch(merged, r, cnt)), mg), r
