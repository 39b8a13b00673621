"""The chunked list walk (k_merge_spec, laspj_lists.hip) where it does what it exists
for: wrong entry guesses corrected chunk by chunk over several rounds, walks from different
columns meeting, the barrier over many workgroups, more than 64 chunks, 2..4 replicas per
launch, every way of falling back to the one-wave walk, and the device words it must leave
zero.  LASPJ_TUNE_LIST_CHUNK 64 / 100 / 256 puts lists of 0.6k-5.2k rows at 3..82 chunks in
1..21 workgroups (100 is no multiple of the wave: chunk starts fall inside a 256-rank
window).

Every case is compared with the oracle's clauses (oracle/otp.py through oracle/orset.py,
oracle/gset.py, oracle/core.py) in both argument orders and in the kernel's three modes,
with the step walk (LASPJ_TUNE_LIST_WALK 1), and — so that a fall-back cannot stand in for
the chunked plan writer, nor the reverse — with the path tests/spec_walk_model.py says the
launch takes (Context.last_list_walk: 1 settled, 2 fell back, 0 not launched).  The
model's verdicts stand beside the cases as literals; tests/test_spec_walk_model.py (CPU)
recomputes them and proves the table reaches every branch named there.  Keys use the
1 == 1.0 dictionary of test_gpu_lists_sorted.py, so the side ordsets:union's argument
switch carries across chunks is visible in a G-Set merge as int vs float."""

import numpy as np
import pytest

from oracle import core as ocore, gset as ogset, orset as oorset
from oracle.terms import exact_eq

from test_gpu_lists_sorted import V, decode, env, key_term, tok_term  # noqa: F401
from test_gpu_lists_walk import _list

pytestmark = pytest.mark.gpu

SEED = 36
CHUNKS = (64, 100, 256)


# ------------------------------------------------------------------ the case table
def _saw(rng, n, blocks, lo=0, hi=V):
    """n rows in `blocks` ascending blocks."""
    cuts = np.linspace(0, n, blocks + 1).astype(int)
    out = []
    for a, b in zip(cuts, cuts[1:]):
        out += sorted(int(x) for x in rng.integers(lo, hi, b - a))
    return out


def _edit(rng, vals, n_ins, n_del, lo, hi):
    """vals with n_del rows dropped and n_ins random rows inserted, at places in [lo, hi)."""
    v = list(vals)
    for _ in range(n_del):
        v.pop(int(rng.integers(lo, min(hi, len(v)))))
    for _ in range(n_ins):
        v.insert(int(rng.integers(lo, min(hi, len(v)) + 1)), int(rng.integers(0, V)))
    return v


def _paired(n, k, p, q):
    """Two descending n-row lists with a paired edit: k extra rows (the key before them
    again) in A at p, in B at q."""
    a = list(range(V - 1, V - 1 - n, -1))
    b = list(a)
    for _ in range(k):
        a.insert(p, V - 1 - p)
    for _ in range(k):
        b.insert(q, V - 1 - q)
    return a, b


def _cases():
    rng = np.random.default_rng(SEED)
    out = []
    s7 = _saw(rng, 5194, 7)
    out.append(("sawtooth 5194/7, edited copy", s7, _edit(rng, s7, 6, 4, 0, len(s7)), CHUNKS))
    out.append(("sawtooth 5194/7, itself", s7, list(s7), (64,)))
    s3 = _saw(rng, 1300, 3)
    out.append(("sawtooth 1300/3, rows inserted", s3, _edit(rng, s3, 6, 0, 0, len(s3)), CHUNKS))
    for k, p, q in ((1, 100, 900), (3, 200, 500), (1, 640, 900), (5, 100, 1100), (2, 1000, 1200),
                    (8, 64, 640), (20, 500, 1000), (40, 10, 1270), (64, 300, 600), (2, 630, 650)):
        a, b = _paired(1280, k, p, q)
        out.append((f"descending 1280, paired edit k={k} {p}->{q}", a, b, (64,)))
    perm = [int(x) for x in rng.permutation(V)[:2000]]
    out.append(("permutation, itself", perm, list(perm), (100,)))
    out.append(("permutation, edited at the start", perm, _edit(rng, perm, 3, 3, 0, 60), CHUNKS))
    out.append(("permutation, edited in the middle", perm, _edit(rng, perm, 4, 4, 900, 1000),
                CHUNKS))
    out.append(("permutation, edited at the end", perm, _edit(rng, perm, 3, 3, 1900, 2000), CHUNKS))
    asc = sorted(int(x) for x in rng.integers(0, V, 2500))
    a1 = list(asc)
    a1[700], a1[701] = min(V - 1, a1[701] + 5), a1[700]
    out.append(("ascending, one descent, edited copy", a1, _edit(rng, asc, 10, 10, 0, 2500),
                CHUNKS))
    # long ascending blocks of small keys in B (1400, 300 and 40 rows): B runs longer than
    # the plan writer's 32, the walk's 256-rank window and its 1024-rank stream step
    big = sorted(int(x) for x in rng.integers(V // 2, V, 1500))
    big[700], big[701] = min(V - 1, big[701] + 7), big[700]
    small = sorted(int(x) for x in rng.integers(0, V // 2, 1740))
    out.append(("long blocks of small keys in B", big,
                small[340:] + big[:400] + small[40:340] + big[400:900] + small[:40] + big[905:],
                CHUNKS))
    # one B row goes first, then every row pairs: chunks with no single step, so the side
    # a later pair takes is carried over them
    p3 = _saw(rng, 640, 3)
    out.append(("whole chunks only pair", p3, p3[:5] + [max(0, p3[5] - 1)] + p3[5:], CHUNKS))
    out.append(("B empty", [int(x) for x in rng.permutation(V)[:333]], [], CHUNKS))
    out.append(("one row each", [5], [5], (64,)))
    return out


CASES = _cases()

# tests/spec_walk_model.py's verdict per case and chunk knob, (A, B) then (B, A): (what
# Context.last_list_walk answers, rounds).  (1, 0): the keys ascend — launched, and the
# kernel skips the replica; (0, 0): A is empty, nothing is launched.  (2, 16): fell at the
# round cap; (2, fewer): by the majority rule.
# test_spec_walk_model.py::test_case_table_matches_model recomputes them.
EXPECT = {
    "sawtooth 5194/7, edited copy": {
        64: ((1, 13), (1, 13)),
        100: ((1, 5), (1, 4)),
        256: ((1, 3), (1, 2)),
    },
    "sawtooth 5194/7, itself": {
        64: ((1, 2), (1, 2)),
    },
    "sawtooth 1300/3, rows inserted": {
        64: ((1, 6), (1, 6)),
        100: ((1, 5), (1, 4)),
        256: ((1, 2), (1, 2)),
    },
    "descending 1280, paired edit k=1 100->900": {
        64: ((1, 7), (2, 2)),
    },
    "descending 1280, paired edit k=3 200->500": {
        64: ((1, 14), (2, 16)),
    },
    "descending 1280, paired edit k=1 640->900": {
        64: ((1, 7), (1, 12)),
    },
    "descending 1280, paired edit k=5 100->1100": {
        64: ((1, 4), (2, 2)),
    },
    "descending 1280, paired edit k=2 1000->1200": {
        64: ((1, 3), (1, 7)),
    },
    "descending 1280, paired edit k=8 64->640": {
        64: ((1, 11), (2, 3)),
    },
    "descending 1280, paired edit k=20 500->1000": {
        64: ((1, 6), (1, 15)),
    },
    "descending 1280, paired edit k=40 10->1270": {
        64: ((1, 2), (2, 2)),
    },
    "descending 1280, paired edit k=64 300->600": {
        64: ((1, 11), (2, 16)),
    },
    "descending 1280, paired edit k=2 630->650": {
        64: ((1, 11), (1, 13)),
    },
    "permutation, itself": {
        100: ((1, 2), (1, 2)),
    },
    "permutation, edited at the start": {
        64: ((1, 2), (1, 2)),
        100: ((1, 2), (1, 2)),
        256: ((1, 2), (1, 2)),
    },
    "permutation, edited in the middle": {
        64: ((1, 2), (1, 2)),
        100: ((1, 2), (1, 2)),
        256: ((1, 2), (1, 2)),
    },
    "permutation, edited at the end": {
        64: ((1, 2), (1, 2)),
        100: ((1, 2), (1, 2)),
        256: ((1, 2), (1, 2)),
    },
    "ascending, one descent, edited copy": {
        64: ((2, 16), (2, 16)),
        100: ((2, 2), (2, 2)),
        256: ((2, 2), (2, 2)),
    },
    "long blocks of small keys in B": {
        64: ((1, 2), (2, 2)),
        100: ((1, 2), (2, 2)),
        256: ((1, 2), (2, 2)),
    },
    "whole chunks only pair": {
        64: ((1, 2), (1, 2)),
        100: ((1, 2), (1, 2)),
        256: ((1, 2), (1, 2)),
    },
    "B empty": {
        64: ((1, 2), (0, 0)),
        100: ((1, 2), (0, 0)),
        256: ((1, 2), (0, 0)),
    },
    "one row each": {
        64: ((1, 0), (1, 0)),
    },
}


def _replica_batches():
    """2, 3 and 4 replicas per launch (chunk 64; L and the grid come from the longest A):
    name -> [(A, B) per replica]."""
    rng = np.random.default_rng(SEED + 1)
    long_pair = _paired(1280, 1, 640, 900)                  # 21 chunks in 6 workgroups
    short_pair = _paired(200, 1, 50, 120)                   # 4 chunks: 5 workgroups idle
    up = (sorted(int(x) for x in rng.integers(0, V, 900)),
          sorted(int(x) for x in rng.integers(0, V, 800)))   # both ascend: the kernel skips it
    s2 = _saw(rng, 1000, 4)
    mid_pair = (s2, _edit(rng, s2, 3, 3, 0, len(s2)))
    a_empty = ([], [int(x) for x in rng.permutation(V)[:300]])
    fa, fb = _paired(1280, 5, 100, 1100)
    settles = _paired(1280, 2, 1000, 1200)
    return {"2 replicas, 21 and 4 chunks": [long_pair, short_pair],
            "3 replicas: ascending, sawtooth, A empty": [up, mid_pair, a_empty],
            "4 replicas: one falls, one settles, ascending, A empty": [(fb, fa), settles, up,
                                                                       a_empty]}


REPLICA_BATCHES = _replica_batches()

# the model's verdict per batch, in the given order and with every pair swapped: (what
# Context.last_list_walk answers, rounds per replica) — test_case_table_matches_model
REPLICA_EXPECT = {
    "2 replicas, 21 and 4 chunks":
        ((1, [7, 3]), (1, [12, 5])),
    "3 replicas: ascending, sawtooth, A empty":
        ((1, [0, 3, 2]), (1, [0, 3, 2])),
    "4 replicas: one falls, one settles, ascending, A empty":
        ((2, [2, 3, 0, 2]), (1, [4, 7, 0, 2])),
}


# ------------------------------------------------------------------------ the tests
class _Knobs:
    """LASPJ_TUNE_LIST_WALK / LIST_CHUNK for a block, both restored after it."""

    def __init__(self, ctx):
        self.ctx = ctx

    def set(self, walk, chunk=0):
        from lasp_amd import _lib
        self.ctx.set_tuning(_lib.TUNE_LIST_WALK, walk)
        self.ctx.set_tuning(_lib.TUNE_LIST_CHUNK, chunk)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.set(0, 0)


def _pair(ctx, rng, va, vb):
    """(terms, OR-Set list, G-Set key terms, G-Set list) of both sides."""
    from lasp_amd import _lib, engine
    out = []
    for vals in (va, vb):
        t, keys, toff, toks = _list(rng, vals)
        out.append((t, engine.ListBatch(ctx, _lib.KIND_ORSET_LIST).upload(keys, toff, toks),
                    [e[0] for e in t], engine.ListBatch(ctx, _lib.KIND_GSET_LIST).upload(keys)))
    return out


def _modes(order, x, y):
    """The kernel's three modes over the pair (x, y): (name, run, the oracle's answer)."""
    (tx, X, gx, GX), (ty, Y, gy, GY) = x, y
    return (("merge", lambda: decode(X.merge(Y, order), False), lambda: oorset.merge(tx, ty)),
            ("union", lambda: decode(X.union(Y, order), False),
             lambda: ocore.union_body("lasp_orset", tx, ty)),
            ("gset merge", lambda: decode(GX.merge(GY, order), True),
             lambda: ogset.merge(gx, gy)))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c[0] for c in CASES])
def test_chunked_walk_case(env, k):
    ctx, order, _keep = env
    name, va, vb, knobs = CASES[k]
    a, b = _pair(ctx, np.random.default_rng(7000 + k), va, vb)
    with _Knobs(ctx) as knob:
        for swapped, (x, y) in enumerate(((a, b), (b, a))):
            for mode, run, oracle in _modes(order, x, y):
                want = oracle()
                knob.set(1)
                step = run()
                assert ctx.last_list_walk() == 0, (name, mode)
                assert exact_eq(step, want), (name, mode, swapped)
                for chunk in knobs:
                    knob.set(3, chunk)
                    got = run()
                    walk = ctx.last_list_walk()
                    assert exact_eq(got, want), (name, mode, swapped, chunk, walk)
                    assert walk == EXPECT[name][chunk][swapped][0], (name, mode, swapped, chunk)
                    assert exact_eq(got, step), (name, mode, swapped, chunk)


def _decode_replica(lb, r, gset):
    from lasp_amd._lib import LIST_REMOVED
    keys, toff, toks = lb.download(r)
    if gset:
        return [key_term(int(k)) for k in keys]
    return [(key_term(int(k)), [(tok_term(int(t) & 63), bool(int(t) & LIST_REMOVED))
                                for t in toks[int(toff[i]):int(toff[i + 1])]])
            for i, k in enumerate(keys)]


@pytest.mark.parametrize("name", list(REPLICA_BATCHES))
def test_chunked_walk_replicas(env, name):
    """R = 2, 3, 4 in one launch: per-replica round words, chunk counts that differ (whole
    workgroups idle for the short replica), a replica the kernel skips beside one whose
    blocks spin, a replica with no rows in A (the c == 0 && nc == 0 branch writes B's
    tail), and one replica falling back while another settles."""
    from lasp_amd import _lib, engine
    ctx, order, _keep = env
    pairs = REPLICA_BATCHES[name]
    R = len(pairs)
    rng = np.random.default_rng(8000 + R)
    lists = [(_list(rng, va), _list(rng, vb)) for va, vb in pairs]
    cap_e = max(len(v) for p in pairs for v in p)
    cap_t = max(len(l[3]) for p in lists for l in p)
    with _Knobs(ctx) as knob:
        for swapped in (0, 1):
            for gset in (False, True):
                kind = _lib.KIND_GSET_LIST if gset else _lib.KIND_ORSET_LIST
                A = engine.ListBatch(ctx, kind, R, cap_e, cap_t)
                B = engine.ListBatch(ctx, kind, R, cap_e, cap_t)
                want_m, want_u = [], []
                for r, p in enumerate(lists):
                    (ta, *ia), (tb, *ib) = p[::-1] if swapped else p
                    A.upload(*(ia[:1] if gset else ia), replica=r)
                    B.upload(*(ib[:1] if gset else ib), replica=r)
                    if gset:
                        want_m.append(ogset.merge([e[0] for e in ta], [e[0] for e in tb]))
                    else:
                        want_m.append(oorset.merge(ta, tb))
                        want_u.append(ocore.union_body("lasp_orset", ta, tb))
                knob.set(3, 64)
                M = A.merge(B, order)
                assert ctx.last_list_walk() == REPLICA_EXPECT[name][swapped][0], (name, swapped)
                for r in range(R):
                    assert exact_eq(_decode_replica(M, r, gset), want_m[r]), (name, swapped, r)
                if not gset:
                    U = A.union(B, order)
                    assert ctx.last_list_walk() == REPLICA_EXPECT[name][swapped][0]
                    for r in range(R):
                        assert exact_eq(_decode_replica(U, r, False), want_u[r]), (name, swapped, r)


def _case(name):
    return next(c for c in CASES if c[0] == name)


FELL_CASE = "descending 1280, paired edit k=3 200->500"       # (B, A): falls at the cap
SETTLED_CASE = "sawtooth 5194/7, edited copy"                 # 82 chunks against 21


def test_words_left_zero_between_calls(env):
    """One context: a launch that falls back, then one that settles at another chunk count,
    then the first again; and the reverse.  Each answer is the oracle's — the last block of
    every launch, fallen or settled, must have left the round words, the done ticket and
    both buffers of chunk words zero for whatever launch comes next.  Every step is one
    call."""
    ctx, order, _keep = env
    _n, fa, fb, _k = _case(FELL_CASE)
    _n, sa, sb, _k = _case(SETTLED_CASE)
    assert EXPECT[FELL_CASE][64][1] == (2, 16) and EXPECT[SETTLED_CASE][64][0][0] == 1
    rng = np.random.default_rng(9100)
    f = _pair(ctx, rng, fb, fa)
    s = _pair(ctx, rng, sa, sb)
    with _Knobs(ctx) as knob:
        knob.set(3, 64)
        for seq in ((f, s, f), (s, f, s)):
            for x, y in seq:
                for mode, run, oracle in _modes(order, x, y):
                    got = run()
                    assert ctx.last_list_walk() == (2 if x is f[0] else 1), mode
                    assert exact_eq(got, oracle()), mode


def test_bind_hints(env):
    """laspj_list_bind under the default walk (LASPJ_TUNE_LIST_WALK 0), chunk 64, the same
    pair bound three times.  The first bind tries the rank-indexed path, which answers
    "keys do not ascend" and marks the lists (not_asc); the same call then takes the merge
    path with that hint, so it already launches the chunked walk.  For a pair whose walks
    do not meet that launch falls back (2) and marks the lists no_spec, which is sticky:
    the second and third bind launch nothing (0).  For a pair that settles every bind
    launches it (1).  Uploading the inputs again clears both hints: the pair that fell
    launches again.  Statuses and merged lists equal the step walk's bind each time."""
    from lasp_amd import _lib, engine
    ctx, order, _keep = env
    for name, swapped, walks in ((FELL_CASE, 1, [2, 0, 0]),
                                 ("descending 1280, paired edit k=2 1000->1200", 0, [1, 1, 1])):
        _n, va, vb, _k = _case(name)
        assert EXPECT[name][64][swapped][0] == walks[0]
        if swapped:
            va, vb = vb, va
        rng = np.random.default_rng(9200 + swapped)
        (ta, *ia), (tb, *ib) = _list(rng, va), _list(rng, vb)
        up = lambda l: engine.ListBatch(ctx, _lib.KIND_ORSET_LIST).upload(*l)   # noqa: E731
        with _Knobs(ctx) as knob:
            knob.set(1)
            M, st = up(ia).bind(up(ib), order)
            step = (int(st[0]), M.download())
            assert ctx.last_list_walk() == 0
            assert exact_eq(decode(M, False), oorset.merge(ta, tb))
            knob.set(0, 64)
            A, B = up(ia), up(ib)
            seen = []
            for _ in range(3):
                M, st = A.bind(B, order)
                seen.append(ctx.last_list_walk())
                assert int(st[0]) == step[0], name
                assert all(np.array_equal(u, w) for u, w in zip(M.download(), step[1])), name
            assert seen == walks, name
            if walks[0] == 2:
                A.upload(*ia)
                B.upload(*ib)
                M, st = A.bind(B, order)
                assert ctx.last_list_walk() == 2
                assert int(st[0]) == step[0]
                assert all(np.array_equal(u, w) for u, w in zip(M.download(), step[1]))
