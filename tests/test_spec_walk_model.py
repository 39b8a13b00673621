"""tests/spec_walk_model.py — the chunked list walk's control restated — pinned on
hand-worked cases, checked against the oracle's clause walk on every settled case of
tests/test_gpu_spec_walk.py's table, and used to prove that the table reaches every branch
of k_merge_spec the GPU tests are there for.  CPU only."""

import spec_walk_model as M
import test_gpu_spec_walk as T
from oracle import gset as ogset, orset as oorset
from oracle.terms import exact_eq


# ------------------------------------------------------------------- literal cases
def test_launch_shape():
    """merge_enqueue's spL / spC / grid."""
    assert M.launch(5194, 64) == (64, 84, 21)              # 82 chunks with rows, 2 waves idle
    assert M.launch(5194, 100) == (100, 52, 13)
    assert M.launch(2600, 0) == (1024, 4, 1)               # the default chunk: one workgroup
    assert M.launch(8000, 0) == (1024, 8, 2)
    assert M.launch(1, 64) == (64, 4, 1)
    assert M.launch(2_000_000, 64) == (1954, 1024, 256)    # never more than 1024 chunks
    assert M.launch(0, 64) is None
    assert M.launch(100, 64, R=5) is None and M.launch(100, 64, R=4) is not None
    assert M.launch(100, 64, walk=1) is None
    assert M.launch(100, 1 << 20) is None


def test_one_chunk_walk_by_hand():
    """A = [4 9 2 7], B = [1 4 8 9 2] from (0, 0): 1 goes first, 4 pairs, 8 goes first,
    9 pairs, 2 pairs, B is done, 7 goes alone."""
    A, B = [4, 9, 2, 7], [1, 4, 8, 9, 2]
    st = []
    assert M.chunk_walk(A, B, 0, 4, 0, st) == (5, 3, 1)
    assert st == [("B", 0, 0), ("P", 0, 1), ("B", 1, 2), ("P", 1, 3), ("P", 2, 4), ("A", 3, 5)]
    assert M.chunk_walk(A, B, 0, 2, 0) == (4, 2, 2)         # stops once row 1 is placed
    assert M.chunk_walk(A, B, 2, 4, 2) == (2, 0, 1)         # 2 < 8 and 7 < 8: rows alone
    assert M.chunk_walk(A, B, 2, 4, 4) == (5, 1, 1)
    assert M.chunk_walk([5, 3, 1], [5, 3, 1], 1, 3, 1) == (3, 2, 0)      # only pairs: side 0
    assert M.chunk_walk([5], [], 0, 1, 0) == (0, 0, 1)


def test_majority_fall_by_hand():
    """The lists above in chunks of 2 rows: chunk 1 guesses column 2*5//4 = 2 and leaves at
    2; round 1 enters it at chunk 0's exit 4 and it leaves at 5.  One workgroup, its exit
    changed after round 1: 2*1 > 1, the one-wave walk."""
    w = M.run([4, 9, 2, 7], [1, 4, 8, 9, 2], knob=2)
    assert (w.L, w.C, w.grid, w.nc) == (2, 4, 1, 2)
    assert (w.outcome, w.rounds, w.fell_by, w.history) == (M.FELL, 2, "majority", [0, 1])


def test_settles_in_four_rounds_by_hand():
    """12 rows, the last four descending back; B is A behind one extra row.  Chunks of 2:
    6 chunks, 2 workgroups.  Round 0: every guess i0*13//12 = i0 is one column short; in
    ascending keys the walk steps over one B row and is right (exits 3 5 7 9), but chunk
    4 (keys 5 15 against 80) leaves at 8 and chunk 5 at 13.  Round 1: chunk 4 enters at 9
    and leaves at 11, chunk 5 enters at 8 (chunk 4's old exit) and leaves at 8.  Round 2:
    chunk 5 enters at 11 and leaves at 13.  Round 3: nothing changes.  One of two
    workgroups changed each time: no majority."""
    A = [10, 20, 30, 40, 50, 60, 70, 80, 5, 15, 25, 35]
    B = [1] + A
    w = M.run(A, B, knob=2)
    assert (w.L, w.C, w.grid, w.nc) == (2, 8, 2, 6)
    assert (w.outcome, w.rounds, w.history) == (M.SETTLED, 4, [0, 1, 1, 0])
    assert w.words == [(0, 3, 2, 2), (3, 5, 2, 0), (5, 7, 2, 0), (7, 9, 2, 0), (9, 11, 2, 0),
                       (11, 13, 2, 0)]
    f = M.features(w, 12, 13)
    assert f["tie_cross"] and f["full_last"] and f["idle_waves"] and not f["a_cross"]
    assert f["allpair_then_pair"] == 2 and f["longest_b"] == 1
    # the plan: B's 1 first, then twelve pairs, each taking B's item in a G-Set merge
    assert M.merged(w, 12, 13, gset=True) == [("B", 0)] + [("P", i, i + 1, 2) for i in range(12)]
    # the other way round A's extra row goes alone and the pairs take A's item
    w = M.run(B, A, knob=2)
    assert w.outcome == M.SETTLED
    assert M.merged(w, 13, 12, gset=True) == [("A", 0)] + [("P", i + 1, i, 1) for i in range(12)]


def test_cap_and_skipped_replicas():
    """Descending lists, A behind one extra row that goes alone, B with ten more rows at
    its end, chunks of 4: chunk 0 is right and leaves at 3; every other guess i0*90//81 is
    ahead, so the row's key tops every B key left and the walk runs off B's end — and
    entered there it stays there.  Round k corrects chunk k alone (one workgroup changes:
    no majority): 11 chunks settle in 12 rounds, 21 chunks are cut off at 16.  Ascending
    lists are launched over but not walked."""
    D = list(range(99, 19, -1))
    w = M.run([0] + D, D + list(range(15, 5, -1)), knob=4)
    assert (w.nc, w.grid, w.outcome, w.rounds, w.fell_by) == (21, 6, M.FELL, 16, "cap")
    assert w.history == [0] + [1] * 15
    D = D[:40]
    w = M.run([0] + D, D + list(range(15, 5, -1)), knob=4)
    assert (w.nc, w.grid, w.outcome, w.rounds) == (11, 3, M.SETTLED, 12)
    assert w.history == [0] + [1] * 10 + [0]
    assert [x[1] for x in w.words] == [3, 7, 11, 15, 19, 23, 27, 31, 35, 39, 40]
    w = M.run([1, 2, 3], [2, 3, 4], knob=64)
    assert (w.outcome, w.walked, w.rounds) == (M.SETTLED, False, 0)
    assert M.run([], [3, 1], knob=64).outcome == M.NOT_LAUNCHED
    # no rows in A beside a longer replica: two empty rounds, then B's tail
    w = M.run([], [3, 1], knob=64, known_e=100, R=2)
    assert (w.outcome, w.walked, w.rounds, w.nc) == (M.SETTLED, True, 2, 0)
    assert M.merged(w, 0, 2) == [("B", 0), ("B", 1)]


# ------------------------------------------------------------------- the case table
def _triples():
    for name, va, vb, knobs in T.CASES:
        for chunk in knobs:
            for swapped, (x, y) in enumerate(((va, vb), (vb, va))):
                yield name, chunk, swapped, x, y


_RUNS = {}


def _run(name, chunk, swapped, x, y):
    key = (name, chunk, swapped)
    if key not in _RUNS:
        _RUNS[key] = M.run(x, y, chunk)
    return _RUNS[key]


def test_case_table_matches_model():
    """The literals beside the GPU tests' cases are the model's verdicts."""
    assert len({c[0] for c in T.CASES}) == len(T.CASES)
    for name, va, vb, knobs in T.CASES:
        assert max(len(va), len(vb)) <= 6000 and set(knobs) <= set(T.CHUNKS)
        assert set(T.EXPECT[name]) == set(knobs), name
    for name, chunk, swapped, x, y in _triples():
        w = _run(name, chunk, swapped, x, y)
        assert T.EXPECT[name][chunk][swapped] == (w.outcome, w.rounds), (name, chunk, swapped)
        assert w.C <= 256
    for name, pairs in T.REPLICA_BATCHES.items():
        assert 2 <= len(pairs) <= 4
        for swapped in (0, 1):
            ps = [p[::-1] for p in pairs] if swapped else pairs
            ws = [M.run(a, b, 64, known_e=max(len(p[0]) for p in ps), R=len(ps)) for a, b in ps]
            assert T.REPLICA_EXPECT[name][swapped] == (M.batch_outcome(ws), [w.rounds for w in ws])
            assert all(w.C <= 256 for w in ws)


def test_replica_batches_hold_what_they_are_for():
    """Conditions on the replica batches, from the model (given order)."""
    out = {}
    for name, pairs in T.REPLICA_BATCHES.items():
        ke = max(len(a) for a, _b in pairs)
        out[len(pairs)] = [M.run(a, b, 64, known_e=ke, R=len(pairs)) for a, b in pairs], pairs
    ws, _p = out[2]
    assert all(w.outcome == M.SETTLED and w.walked for w in ws)
    assert 0 < -(-ws[1].nc // M.WAVES) < ws[1].grid == ws[0].grid   # workgroups with no chunk
    ws, pairs = out[3]
    assert [w.walked for w in ws] == [False, True, True]          # one replica skipped
    assert pairs[2][0] == [] and ws[2].nc == 0 and ws[2].rounds == 2
    assert all(w.outcome == M.SETTLED for w in ws)
    ws, pairs = out[4]
    assert ws[0].outcome == M.FELL and ws[1].outcome == M.SETTLED and ws[1].rounds > 2
    assert not ws[2].walked and pairs[3][0] == []


def test_final_round_is_the_clauses_walk():
    """For every settled case: the final round's chunk walks, one after the other, are the
    walk of orddict:merge / ordsets:union from (0, 0) — the same rows alone, the same
    pairs, in the same order, and in a G-Set merge the same side's item for every pair.
    Rows are told apart by their tokens (OR-Set) and by int (A) against float (B) keys."""
    n = 0
    for name, chunk, swapped, x, y in _triples():
        w = _run(name, chunk, swapped, x, y)
        if w.outcome != M.SETTLED or not w.walked:
            continue
        n += 1
        # consecutive chunks agree: each enters where the one before left
        assert w.words[0][0] == 0
        assert all(w.words[c][0] == w.words[c - 1][1] for c in range(1, w.nc)), name
        ta = [(k, [(b"a%06d" % i, False)]) for i, k in enumerate(x)]
        tb = [(k, [(b"b%06d" % j, False)]) for j, k in enumerate(y)]
        got = []
        for _key, toks in oorset.merge(ta, tb):
            ids = {t[:1]: int(t[1:]) for t, _f in toks}
            got.append(("P", ids[b"a"], ids[b"b"], 1) if len(ids) == 2 else
                       ("A", ids[b"a"]) if b"a" in ids else ("B", ids[b"b"]))
        assert got == M.merged(w, len(x), len(y)), (name, chunk, swapped)
        want = ogset.merge([int(k) for k in x], [float(k) for k in y])
        mine = []
        for s in M.merged(w, len(x), len(y), gset=True):
            if s[0] == "P":
                mine.append(x[s[1]] if s[3] == 1 else float(y[s[2]]))
            else:
                mine.append(x[s[1]] if s[0] == "A" else float(y[s[1]]))
        assert exact_eq(mine, want), (name, chunk, swapped)
    assert n >= 40


def test_table_reaches_every_branch():
    """Conditions on the case table (not measurements), from the model: what the GPU
    tests' cases make k_merge_spec do."""
    settled, fell, total = [], [], 0
    for name, chunk, swapped, x, y in _triples():
        w = _run(name, chunk, swapped, x, y)
        total += 1
        if w.outcome == M.SETTLED and w.walked:
            settled.append((M.features(w, len(x), len(y)), name, chunk, swapped))
        elif w.outcome == M.FELL:
            fell.append(w)
    F = [f for f, *_ in settled]
    rounds = {f["rounds"] for f in F}
    assert 2 in rounds and 3 in rounds
    assert rounds & set(range(4, 8)) and rounds & set(range(8, 12)) and rounds & set(range(12, 16))
    assert any(w.fell_by == "majority" and w.rounds == 2 for w in fell)
    assert any(w.fell_by == "majority" and 2 < w.rounds < M.ROUNDS for w in fell)
    assert any(w.fell_by == "cap" and w.rounds == M.ROUNDS for w in fell)
    # the pair sum's and the carried side's second trip over the chunks before (k += 64),
    # in a walk that took corrections
    assert any(f["chunks"] > 64 and f["rounds"] > 2 for f in F)
    assert any(f["blocks"] >= 5 and f["rounds"] > 2 for f in F)
    assert any(f["full_last"] for f in F) and any(not f["full_last"] for f in F)
    assert any(f["idle_waves"] for f in F) and any(not f["idle_waves"] for f in F)
    assert any(f["tie_cross"] for f in F) and any(f["a_cross"] for f in F)
    assert any(f["b_at_boundary"] for f in F) and any(f["b_at_group"] for f in F)
    # B runs: the plan writer goes wave-wide above 32, the walk leaves its 256-rank window
    # above 256 and takes a second 1024-rank stream step above 1280
    runs = set()
    for f in F:
        runs |= set(f["b_runs"])
    assert any(32 < r <= 256 for r in runs) and any(256 < r <= 1280 for r in runs)
    assert any(r > 1280 for r in runs)
    assert any(1 <= r <= 32 for r in runs)
    # a chunk that only pairs, B's item carried over it into pairs of the next chunk
    # (16 pairs or more: with int / float slots drawn at random some differ)
    assert any(f["allpair_then_pair"] >= 16 for f in F)
    assert any(f["entered_b_done"] for f in F)
    assert 3 * len(settled) >= 2 * total, (len(settled), total)


def test_older_walk_shapes_at_the_default_chunk():
    """What test_gpu_lists_walk.py's thirteen shapes do at the default chunk (DESIGN.md's
    table, the docstring of its _walks): at most 11 chunks in 3 workgroups, whatever
    settles does so in 2 rounds, whatever falls does so by majority at round 2 — with one
    workgroup, the edited reversed lists among them.  At chunk 256 they stay within 41
    chunks in 11 workgroups."""
    import numpy as np
    import test_gpu_lists_walk as W
    verdicts = {}
    for base in (500, 900):                            # the OR-Set and the G-Set test's draws
        for k in range(13):
            name, va, vb = W.shapes(np.random.default_rng(base + k))[k]
            for swapped, (x, y) in enumerate(((va, vb), (vb, va))):
                w = M.run(x, y, 0)
                assert w.nc <= 11 and w.grid <= 3
                assert (w.rounds, w.fell_by) in ((2, ""), (2, "majority"), (0, "")), name
                verdicts[base, name, swapped] = w.outcome
                w = M.run(x, y, 256)
                assert w.nc <= 41 and w.grid <= 11
    for base in (500, 900):
        assert verdicts[base, "reversed, a few added", 0] == M.FELL
        assert verdicts[base, "reversed, a few added", 1] == M.SETTLED
        assert verdicts[base, "reversed, edited both", 0] == M.FELL
        assert verdicts[base, "reversed, identical", 0] == M.SETTLED
        assert verdicts[base, "one side empty", 1] == M.NOT_LAUNCHED
