"""Every variant of the streaming kernels (lasp_amd/csrc/laspj_kernels.hip), and the
grid-stride tails of the segment kernels, at shapes of a few thousand cells.

The stream knobs (include/laspj_tune.h: STREAM_GRID, STREAM_UNROLL, STREAM_NT) and
REDUCE_KERNEL 3 / 4 select kernel instantiations no other test launches, and a small
STREAM_GRID makes a few thousand cells sweep like a full-size batch: several strides per
lane, a ragged tail, lanes with nothing to do.  Every case uploads host arrays, prefills
the destination with the bitwise complement of the expected result (a skipped cell
shows), downloads the WHOLE result and compares it bit for bit with numpy on the
uploaded arrays (`|`, np.maximum, np.bitwise_or.reduce, np.maximum.reduce, popcounts);
OR-Sets are also checked token for token against the oracle's orddict merge / bodies on
a few replicas.  Nothing is sampled and no device predicate serves as the check.
`test_case_shapes_reach_every_loop` (CPU) restates stream_tune and proves that the cell
counts used below reach the unrolled loop twice, the remainder loop, and idle lanes.

Knob setting -> kernel instantiation (g = STREAM_GRID 1 | 3 unless noted):

  join (OR-Set, G-Set)   UNROLL 0|1 -> k_or16<1,NT>   UNROLL 2 -> k_or16<2,NT>
                         UNROLL 4 -> k_or16<4,NT>     UNROLL 8 -> k_or16<8,NT>
                         NT -1|1 -> NT = true, NT 0 -> NT = false  (all 8 instantiations)
                         UNROLL 0, GRID 64: 2^20 + 257 cells -> k_or16<2,true> (size rule),
                         100 003 cells -> k_or16<1,true>;  odd word count -> + k_or_tail
  join (G-Counter)       k_max16<2> (+ k_max_tail), whatever the knobs
  reduce_from            REDUCE_KERNEL 0, power-of-two length, group 2..4
                             -> k_reduce_or_tile<G,MAX,4>
                         REDUCE_KERNEL 4, the same shapes -> k_reduce_or_flat<G,MAX>
                         REDUCE_KERNEL 1 (and 0 / 3 / 4 otherwise), OR, even words,
                             group 2..4 -> k_reduce_or_g<G>
                         REDUCE_KERNEL 2, or group 5 -> k_reduce_or<true>
                         odd word count (G-Set) -> k_reduce_or<false>
                         G-Counter off the flat path -> k_reduce_max
  reduce_chunks          REDUCE_KERNEL 0, 2..8 chunks: UNROLL 2 -> k_reduce_chunks_tile<M,NC,2>
                             UNROLL 8 -> <M,NC,8>, else <M,NC,4>
                         REDUCE_KERNEL 3, 2..8 chunks -> k_reduce_chunks_n<M,NC,U,NT>,
                             U = 2 at UNROLL 2 else 1
                         REDUCE_KERNEL 2, or 1 chunk -> k_reduce_chunks<M>
                         odd word count -> k_reduce_chunks_scalar<M>
  join_n                 k_reduce_ptrs<M,1..8> (+ k_reduce_ptrs_last<M> at odd words)
  union                  k_orset_union<true>
  precondition_context   UNROLL 1 -> k_orset_context<1,true>, UNROLL 2 -> <2,true>
  fill_synthetic         k_fill_orset, k_fill_gset, k_fill_gcounter
  value_bits             UNROLL 8 -> k_orset_value<REMOVED,8>, else <REMOVED,4>
  gather_inflation       k_gather_inflation<STRICT,SEG=true,KEYED>, GRID 0 | 1 | 3
  stats / equal / inflation / values / threshold_met
                         k_orset_stats<SEG>, k_gset_stats<SEG>, k_equal<SEG,VEC2>,
                         k_orset_inflation<STRICT,SEG>, k_gset_inflation<STRICT,SEG>,
                         k_gcounter_sums<SEG>, k_gcounter_threshold<SEG>,
                         k_gcounter_inflation<STRICT,SEG>; SEG = replica longer than a
                         segment (ticketed), each wave taking >= 2 items
  fragment, filter, increment   k_orset_fragment, k_orset_filter, k_gcounter_incr
"""

import contextlib
import itertools

import numpy as np
import pytest

from oracle import columnar as orc
from oracle import core as ocore
from oracle import lattice as olat
from oracle import orset as oorset
from oracle.terms import exact_eq

from test_gpu_configs import keyfind_threshold, window_orddict
from test_gpu_keyed import FOLDS, MAPS, PREDS, device_list, oracle_list, pipeline

KB = 256                                  # kBlock
MAXU = np.uint64(2**64 - 1)
GUARD = np.uint64(0xA5A5A5A5A5A5A5A5)
GRIDS = (1, 3)
UNROLLS = (0, 1, 2, 4, 8)
NTS = (-1, 0, 1)


# ------------------------------------------------------------------ launch-shape restatement

def stream_shape(n, grid_knob, unroll_knob, nt_knob, cus=256):
    """stream_tune (laspj_kernels.hip) restated: (grid, unroll, nt) for n 16-byte cells."""
    grid = grid_knob if grid_knob > 0 else cus * 64
    unroll = unroll_knob if unroll_knob > 0 else 2
    if unroll_knob <= 0 and n < cus * KB * 8:
        unroll = 1
    nt = True if nt_knob < 0 else nt_knob != 0
    need = -(-n // KB)
    if need < grid:
        grid = max(need, 1)
    return grid, unroll, nt


def kernel_unroll(op, tune_unroll, unroll_knob):
    """Cells per lane per step of the kernel `op` launches, given stream_tune's unroll."""
    if op == "or16":
        return tune_unroll if tune_unroll in (1, 2, 8) else 4
    if op in ("max16", "flat"):          # k_max16<2>; k_reduce_or_flat's double step
        return 2
    if op == "context":
        return 1 if tune_unroll == 1 else 2
    if op == "chunks_n":
        return 2 if unroll_knob == 2 else 1
    return 1                              # union, fills, k_reduce_chunks(_scalar), k_reduce_max


def sweep(n, grid, U):
    """Per lane of a grid-stride sweep `for (; i + (U-1)S < n; i += U S) ...; for (; i < n;
    i += S) ...`: (passes of the unrolled loop, steps of the remainder loop)."""
    S = grid * KB
    i = np.arange(S, dtype=np.int64)
    lim = n - (U - 1) * S - i
    passes = np.where(lim > 0, -(-lim // (U * S)), 0)
    j = i + passes * U * S
    rem = np.where(j < n, -(-(n - j) // S), 0)
    return passes, rem


def cells_for(g, U):
    """The cell counts of one (grid knob, unroll) setting."""
    S = g * KB
    ns = {1, 255, 257, S - 1, S + 1, U * S - 1, U * S, U * S + 1, 2 * U * S + S + 5,
          3 * U * S - 1}
    return sorted(n for n in ns if n > 0)


def join_settings():
    return list(itertools.product(UNROLLS, NTS, GRIDS))


def join_unroll(kind, unroll_knob):
    """The unroll the join kernel of `kind` runs with at these small sizes."""
    if kind == "gcounter":
        return 2
    return unroll_knob if unroll_knob else 1          # size rule: UNROLL 0 -> 1 when small


def test_case_shapes_reach_every_loop():
    """CPU: for every knob setting the GPU tests use, the restated launch shape over that
    setting's cell counts takes >= 2 passes of the unrolled loop, runs the remainder loop,
    and has a launch with n < S (lanes with nothing to do); over the settings every
    U in {1,2,4,8} and both NT values occur.  With U = 1 the two loops of a sweep have the
    same condition, so the remainder loop cannot run: the condition applies to U >= 2.  A
    condition on the cases, not a measurement."""
    seen_u, seen_nt = set(), set()
    for cus in (64, 256, 304, 512):
        for kind, op in (("orset", "or16"), ("gcounter", "max16")):
            for uk, nt, g in join_settings():
                U = join_unroll(kind, uk)
                two, rem_ran, idle = False, False, False
                for n in cells_for(g, U):
                    grid, tu, tnt = stream_shape(n, g, uk, nt, cus)
                    ku = kernel_unroll(op, tu, uk)
                    assert ku == U, (kind, uk, n, cus)      # the case list matches the kernel
                    assert grid == min(g, -(-n // KB))
                    p, r = sweep(n, grid, ku)
                    assert int((p * ku + r).sum()) == n      # every cell exactly once
                    two |= bool(p.max() >= 2)
                    rem_ran |= bool(r.max() >= 1)
                    idle |= n < g * KB
                    if op == "or16":
                        seen_u.add(ku)
                        seen_nt.add(tnt)
                assert two and idle, (kind, uk, nt, g)
                assert rem_ran or U == 1, (kind, uk, nt, g)
        # the default's size rule (UNROLL 0, GRID 64)
        assert stream_shape((1 << 20) + 257, 64, 0, -1, cus) == (64, 2, True)
        assert stream_shape(100_003, 64, 0, -1, cus) == (64, 1, True)
        for n, U in (((1 << 20) + 257, 2), (100_003, 1)):
            p, r = sweep(n, 64, U)
            assert p.min() >= 2 and int((p * U + r).sum()) == n
        assert sweep((1 << 20) + 257, 64, 2)[1].max() >= 1
    assert seen_u == {1, 2, 4, 8} and seen_nt == {False, True}
    # union / fills / context / scalar chunk kernels: U = 1 or 2 under g
    for g in GRIDS:
        for U in (1, 2):
            ps = [sweep(n, min(g, -(-n // KB)), U) for n in cells_for(g, U)]
            assert max(p.max() for p, _ in ps) >= 2
            assert U == 1 or max(r.max() for _, r in ps) >= 1
    # REDUCE_KERNEL 4: k_reduce_or_flat's double step runs twice and its odd remainder runs
    for g in GRIDS:
        for per in FLAT_PER:
            n = REDUCE_GROUPS[per] * per
            p, r = sweep(n, min(g, -(-n // KB)), 2)
            assert r.max() <= 1
            if per == 64:
                assert p.max() >= 2 and r.max() == 1, (g, per)
    # reduce_chunks: the tile kernels see n on, under and over a multiple of T x 256
    for T in (2, 4, 8):
        for d in (-1, 0, 1):
            assert T * KB + d in CHUNK_CELLS
        assert any(n >= 2 * T * KB and n % (T * KB) for n in CHUNK_CELLS)
    # segment kernels: every wave of a g-block launch takes at least two items
    for g in GRIDS:
        for R, n, base in SEG_SHAPES:
            sg = seg_for(R, n, base)
            assert R * (-(-n // sg)) >= 9 * g, (g, R, n)
    assert any(-(-n // seg_for(R, n, base)) > 1 for R, n, base in SEG_SHAPES)
    assert any(-(-n // seg_for(R, n, base)) == 1 for R, n, base in SEG_SHAPES)


def seg_for(R, n, base):
    """seg_for (laspj_kernels.hip) restated: segment length for R replicas of n items."""
    ns = -(-n // base)
    if R * ns >= 2048:
        return base
    want = -(-2048 // R)
    seg = -(-n // want)
    seg = max((seg + 255) & ~255, 256)
    return min(seg, base)


FLAT_PER = (64, 4096)                      # power-of-two replica lengths (cells)
REDUCE_GROUPS = {64: 37, 4096: 5, 100: 37, "odd": 37, 20_000: 3}
CHUNK_CELLS = (1, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 2 * 2048 + 300)
# (replicas, items per replica, base segment) of the segment-kernel cases: cells for
# OR-Sets, words for G-Sets and G-Counters
SEG_SHAPES = ((30, 300, 4096), (3, 20_000, 4096), (40, 100, 4096))


# ------------------------------------------------------------------ fixtures and helpers

@pytest.fixture(scope="module")
def ctx():
    from lasp_amd import engine
    c = engine.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def knobs(ctx, grid=0, unroll=0, nt=-1, reduce=0):
    from lasp_amd import _lib
    try:
        ctx.set_tuning(_lib.TUNE_STREAM_GRID, grid)
        ctx.set_tuning(_lib.TUNE_STREAM_UNROLL, unroll)
        ctx.set_tuning(_lib.TUNE_STREAM_NT, nt)
        ctx.set_tuning(_lib.TUNE_REDUCE_KERNEL, reduce)
        yield
    finally:
        ctx.set_tuning(_lib.TUNE_STREAM_GRID, 0)
        ctx.set_tuning(_lib.TUNE_STREAM_UNROLL, 0)
        ctx.set_tuning(_lib.TUNE_STREAM_NT, -1)    # the default is -1, not 0
        ctx.set_tuning(_lib.TUNE_REDUCE_KERNEL, 0)


def maker(ctx, kind):
    return {"orset": ctx.orset_batch, "gset": ctx.gset_batch,
            "gcounter": ctx.gcounter_batch}[kind]


def shape_for(kind, n, odd=True):
    """(elements) of a 1-replica batch of `kind` with n 16-byte cells: 2n words for
    OR-Sets, 2n + 1 (odd: a tail word) or 2n words for G-Sets / G-Counters."""
    if kind == "orset":
        return n
    w = 2 * n + (1 if odd else 0)
    return 64 * w - 7 if kind == "gset" else w


def bits_words(rng, shape):
    return rng.integers(0, 2**64, size=shape, dtype=np.uint64)


def counts(rng, k, shape):
    """k operands of G-Counter counts that tell an unsigned 64-bit max from a signed or a
    32-bit one: small counts, counts above 2^63 (2^64 - 1 - small), and values that
    differ from a common 64-bit value only in the low or only in the high 32 bits."""
    full = (k,) + tuple(shape)
    c = rng.integers(0, 2**64, size=shape, dtype=np.uint64)
    lo = rng.integers(0, 2**32, size=full, dtype=np.uint64)
    small = rng.integers(0, 6, size=full, dtype=np.uint64)
    sel = rng.integers(0, 4, size=full)
    return np.where(sel == 0, small,
                    np.where(sel == 1, c ^ lo,
                             np.where(sel == 2, c ^ (lo << np.uint64(32)), MAXU - small)))


def operands(rng, kind, k, R, e_n, W):
    """k host images (k, R, W) of `kind`."""
    if kind == "gcounter":
        return counts(rng, k, (R, W))
    h = bits_words(rng, (k, R, W))
    h[rng.random((k, R, W)) < 0.15] = 0
    if kind == "orset":
        h[..., 1::2] &= h[..., 0::2]                  # r within p
    elif e_n % 64:
        h[..., -1] &= np.uint64((1 << (e_n % 64)) - 1)
    return h


def join_np(kind, stack):
    return (np.maximum.reduce if kind == "gcounter" else np.bitwise_or.reduce)(stack, axis=0)


def guarded(make, R, e_n, want, launch):
    """Run launch(dst) with dst a view of a longer batch whose other replicas hold GUARD
    and whose viewed replicas hold ~want; the view must end up == want and the guards
    untouched.  Odd word counts take two leading guard replicas (a view starts 16-byte
    aligned)."""
    W = want.shape[1]
    lead = 1 if W % 2 == 0 else 2
    big = make(R + lead + 1, e_n)
    assert big.words_per_replica == W
    img = np.full((R + lead + 1, W), GUARD, dtype=np.uint64)
    img[lead:lead + R] = ~want
    big.upload(img)
    launch(big.view(lead, R))
    got = big.download_words()
    assert np.array_equal(got[lead:lead + R], want)
    assert (got[:lead] == GUARD).all() and (got[lead + R:] == GUARD).all()


def dirty(dst, want):
    dst.upload(~want)
    return dst


def orddict_merge_check(cells_a, cells_b, got, tokens):
    A = orc.ORDict.from_cells(cells_a, tokens)
    B = orc.ORDict.from_cells(cells_b, tokens)
    assert orc.ORDict.from_cells(got, tokens).equal(A.merge(B))


# ------------------------------------------------------------------ join

@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("kind", ["orset", "gset", "gcounter"])
def test_join_every_variant(ctx, kind, g):
    """d = a ⊔ b for every (UNROLL, NT) at grid g, all cells compared: into a guarded
    view of a complement-filled destination, then in place into either operand."""
    make = maker(ctx, kind)
    rng = np.random.default_rng(1000 + g)
    for uk in UNROLLS:
        U = join_unroll(kind, uk)
        ncells = cells_for(g, U) + ([0] if kind != "orset" and uk == 0 else [])
        for n in ncells:
            e_n = shape_for(kind, n)
            a, b, d = make(1, e_n), make(1, e_n), make(1, e_n)
            W = a.words_per_replica
            ha, hb = operands(rng, kind, 2, 1, e_n, W)
            a.upload(ha)
            b.upload(hb)
            want = join_np(kind, np.stack([ha, hb]))
            for nt in NTS:
                with knobs(ctx, grid=g, unroll=uk, nt=nt):
                    guarded(make, 1, e_n, want, lambda v: v.join(a, b))
                    dirty(d, want).join(a, b)
                    assert np.array_equal(d.download_words(), want), (uk, nt, n)
                    a.join(a, b)
                    assert np.array_equal(a.download_words(), want), (uk, nt, n, "a")
                    a.upload(ha)
                    b.join(a, b)
                    assert np.array_equal(b.download_words(), want), (uk, nt, n, "b")
                    b.upload(hb)
            if kind == "orset" and n <= 1025:
                orddict_merge_check(ha[0].reshape(n, 2), hb[0].reshape(n, 2),
                                    d.download()[0], orc.synth_tokens(n))


@pytest.mark.gpu
@pytest.mark.parametrize("n", [(1 << 20) + 257, 100_003])
def test_join_default_size_rule(ctx, n):
    """UNROLL 0 at GRID 64: 2^20 + 257 cells take k_or16<2,true> by the size rule (for any
    CU count <= 512), 100 003 cells k_or16<1,true>; every lane takes several passes."""
    rng = np.random.default_rng(n)
    a, b = ctx.orset_batch(1, n), ctx.orset_batch(1, n)
    ha, hb = operands(rng, "orset", 2, 1, n, 2 * n)
    a.upload(ha)
    b.upload(hb)
    want = ha | hb
    with knobs(ctx, grid=64):
        guarded(ctx.orset_batch, 1, n, want, lambda v: v.join(a, b))
        a.join(a, b)
    assert np.array_equal(a.download_words(), want)


# ------------------------------------------------------------------ reduce_from

def reduce_lengths(kind):
    """(elements, key into REDUCE_GROUPS) per replica length of the reduce cases."""
    if kind == "orset":
        return [(64, 64), (4096, 4096), (100, 100), (20_000, 20_000)]
    if kind == "gset":                      # odd word counts: 3 and 1
        return [(64 * 3 - 5, "odd"), (40, "odd")]
    return [(128, 64), (8192, 4096), (200, 100), (7, "odd")]


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("kind", ["orset", "gset", "gcounter"])
def test_reduce_from_every_kernel(ctx, kind, g):
    """dst replica i = join of src replicas [i group, (i + 1) group) for REDUCE_KERNEL
    0..4 and groups 2..5 at grid g (the flat sweep, the tiles and the segment kernels)."""
    make = maker(ctx, kind)
    rng = np.random.default_rng(2000 + g)
    for e_n, key in reduce_lengths(kind):
        ng = REDUCE_GROUPS[key]
        for group in (2, 3, 4, 5):
            src, dst = make(ng * group, e_n), make(ng, e_n)
            W = src.words_per_replica
            hs = operands(rng, kind, 1, ng * group, e_n, W)[0]
            src.upload(hs)
            want = join_np(kind, hs.reshape(ng, group, W).swapaxes(0, 1))
            for rk in (0, 1, 2, 3, 4):
                with knobs(ctx, grid=g, reduce=rk):
                    if rk in (0, 4):
                        guarded(make, ng, e_n, want, lambda v: v.reduce_from(src, group))
                    dirty(dst, want).reduce_from(src, group)
                    assert np.array_equal(dst.download_words(), want), (e_n, group, rk)


# ------------------------------------------------------------------ reduce_chunks

@pytest.mark.gpu
@pytest.mark.parametrize("nchunks", range(1, 9))
@pytest.mark.parametrize("kind", ["orset", "gcounter"])
def test_reduce_chunks_every_variant(ctx, kind, nchunks):
    """dst = join over the chunk-major copies, for REDUCE_KERNEL 0 / 2 / 3 x UNROLL x NT x
    grid, at cell counts on, under and over a multiple of T x 256 (T = 2, 4, 8)."""
    make = maker(ctx, kind)
    rng = np.random.default_rng(3000 + nchunks)
    for n in CHUNK_CELLS:
        e_n = shape_for(kind, n, odd=False)
        src, dst = make(nchunks, e_n), make(1, e_n)
        W = src.words_per_replica
        hs = operands(rng, kind, 1, nchunks, e_n, W)[0]
        src.upload(hs)
        want = join_np(kind, hs.reshape(nchunks, 1, W))
        with knobs(ctx, grid=3, reduce=3, unroll=2):
            guarded(make, 1, e_n, want, lambda v: v.reduce_chunks(src, nchunks))
        for rk, uk, nt, g in itertools.product((0, 2, 3), UNROLLS, NTS, GRIDS):
            with knobs(ctx, grid=g, unroll=uk, nt=nt, reduce=rk):
                dirty(dst, want).reduce_chunks(src, nchunks)
                assert np.array_equal(dst.download_words(), want), (n, rk, uk, nt, g)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gset", "gcounter"])
def test_reduce_chunks_odd_words(ctx, kind):
    """An odd word count takes the 8-byte kernel (k_reduce_chunks_scalar), a grid-stride
    sweep over words."""
    make = maker(ctx, kind)
    rng = np.random.default_rng(3100)
    for g in GRIDS:
        S = g * KB
        for w in (1, 255, 257, S - 1, S + 1, 3 * S + 5):
            e_n = 64 * w - 9 if kind == "gset" else w
            for nchunks in (1, 2, 3, 8):
                src, dst = make(nchunks, e_n), make(1, e_n)
                assert src.words_per_replica == w
                hs = operands(rng, kind, 1, nchunks, e_n, w)[0]
                src.upload(hs)
                want = join_np(kind, hs.reshape(nchunks, 1, w))
                for rk in (0, 2, 3):
                    with knobs(ctx, grid=g, reduce=rk):
                        dirty(dst, want).reduce_chunks(src, nchunks)
                        assert np.array_equal(dst.download_words(), want), (w, nchunks, rk)


# ------------------------------------------------------------------ join_n

@pytest.mark.gpu
@pytest.mark.parametrize("nsrc", range(1, 9))
def test_join_n_tiles_and_tails(ctx, nsrc):
    """join_n over 1..8 sources at cell counts around the 1024-cell tile, with and without
    a tail word, into a guarded view and in place into one of the sources."""
    rng = np.random.default_rng(4000 + nsrc)
    for kind, odd in (("orset", False), ("gset", True), ("gcounter", False),
                      ("gcounter", True)):
        make = maker(ctx, kind)
        for n in (1, 1023, 1024, 1025, 5 * 1024 + 7):
            e_n = shape_for(kind, n, odd)
            srcs = [make(1, e_n) for _ in range(nsrc)]
            W = srcs[0].words_per_replica
            hs = operands(rng, kind, nsrc, 1, e_n, W)
            for b, h in zip(srcs, hs):
                b.upload(h)
            want = join_np(kind, hs)
            guarded(make, 1, e_n, want, lambda v: v.join_n(srcs))
            k = nsrc // 2
            srcs[k].join_n(srcs)
            assert np.array_equal(srcs[k].download_words(), want), (kind, n, "alias")


# ------------------------------------------------------------------ union / context / fill

def dec(cells):
    return window_orddict(cells, 0)


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
def test_union_and_context_sweeps(ctx, g):
    """union (keep-left select) and precondition_context (p & ~r, 0) over every cell, and
    against the oracle bodies on the small cases."""
    rng = np.random.default_rng(5000 + g)
    for uk in (1, 2):
        for n in cells_for(g, uk):
            hl, hr = operands(rng, "orset", 2, 1, n, 2 * n)
            hl[:, 0::2][rng.random((1, n)) < 0.3] = 0      # elements only on the right
            hl[:, 1::2] &= hl[:, 0::2]
            hl[..., 0::2] &= np.uint64(0xFF)                 # few tokens: short orddicts
            hl[..., 1::2] &= np.uint64(0xFF)
            hr[..., 0::2] &= np.uint64(0xFF)
            hr[..., 1::2] &= np.uint64(0xFF)
            L, Rb = ctx.orset_batch(1, n), ctx.orset_batch(1, n)
            L.upload(hl)
            Rb.upload(hr)
            cl, cr = hl.reshape(n, 2), hr.reshape(n, 2)
            want_u = np.where((cl[:, :1] != 0), cl, cr).reshape(1, -1)
            want_c = np.stack([cl[:, 0] & ~cl[:, 1], np.zeros(n, np.uint64)],
                              axis=1).reshape(1, -1)
            with knobs(ctx, grid=g, unroll=uk):
                guarded(ctx.orset_batch, 1, n, want_u, lambda v: v.union(L, Rb))
                guarded(ctx.orset_batch, 1, n, want_c, lambda v: v.precondition_context(L))
            if n <= 769:
                assert dec(want_u.reshape(n, 2)) == ocore.union_body("lasp_orset", dec(cl),
                                                                     dec(cr))
                assert exact_eq(dec(want_c.reshape(n, 2)), oorset.precondition_context(dec(cl)))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
def test_fill_synthetic_sweeps(ctx, g):
    """fill_synthetic of every kind under grid g equals the oracle's stream cell for cell
    (a G-Counter count is the low 20 bits of the G-Set stream word of its slot)."""
    with knobs(ctx, grid=g):
        for n in cells_for(g, 1) + [2 * g * KB + 77]:
            for R in (1, 3):
                E = -(-n // R)
                o = ctx.orset_batch(R, E)
                dirty(o, np.zeros((R, 2 * E), np.uint64)).fill_synthetic(7, replica_base=11)
                want = np.stack([orc.synth_orset(7, 11 + i, E) for i in range(R)])
                assert np.array_equal(o.download(), want), (n, R)
                Eg = 64 * E - 13
                s = ctx.gset_batch(R, Eg)
                dirty(s, np.zeros((R, E), np.uint64)).fill_synthetic(8, replica_base=5)
                wg = np.stack([orc.synth_gset(8, 5 + i, Eg) for i in range(R)])
                assert np.array_equal(s.download(), wg), (n, R)
                c = ctx.gcounter_batch(R, E)
                dirty(c, np.zeros((R, E), np.uint64)).fill_synthetic(9, replica_base=2)
                wc = np.stack([orc.synth_gset(9, 2 + i, 64 * E) for i in range(R)]) \
                    & np.uint64(0xFFFFF)
                assert np.array_equal(c.download(), wc), (n, R)


# ------------------------------------------------------------------ value_bits

def pack_rows(pred):
    R, E = pred.shape
    W = (E + 63) // 64
    pad = np.zeros((R, W * 64), np.uint8)
    pad[:, :E] = pred
    return np.ascontiguousarray(np.packbits(pad, axis=1, bitorder="little")).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("R", [1, 3, 70])
def test_value_bits_variants(ctx, R):
    """value / removed bitmaps with 4 and 8 words in flight (UNROLL 8), the default grid
    and grids of 1 and 3 blocks; R = 3 shrinks the segments to 256 cells, R = 70 does not."""
    rng = np.random.default_rng(6000 + R)
    tokens = orc.synth_tokens(257)
    for E in (1, 63, 65, 255, 257, 4095, 4097, 5000):
        h = operands(rng, "orset", 1, R, E, 2 * E)[0]
        b = ctx.orset_batch(R, E)
        b.upload(h)
        cells = h.reshape(R, E, 2)
        want = {False: pack_rows((cells[..., 0] & ~cells[..., 1]) != 0),
                True: pack_rows(cells[..., 1] != 0)}
        for uk, g, removed in itertools.product((0, 8), (0, 1, 3), (False, True)):
            with knobs(ctx, grid=g, unroll=uk):
                assert np.array_equal(b.value_bits(removed=removed), want[removed]), \
                    (E, uk, g, removed)
        if E == 257:
            for i in range(0, R, 23):
                live = np.nonzero(np.unpackbits(want[False][i].view(np.uint8),
                                                bitorder="little")[:E])[0]
                assert np.array_equal(live, orc.ORDict.from_cells(cells[i], tokens).value())


# ------------------------------------------------------------------ gather + inflation

GI_E, GI_R = 3000, 19
GI_PIPES = {
    # keyed: a collapsing map and overlapping fold lists, key chains across slot 4096
    True: (MAPS["div3"], PREDS["drop3"], FOLDS["pair"]),
    # unkeyed: every output key occurs once
    False: (MAPS["id"], PREDS["drop3"], lambda x: [x, x + GI_E]),
}


GI_ONE = 3 * 682 + 2          # element 2048: output slots 4096 / 4097, keys 682 / 683


def gi_replicas(seed):
    """(Prev, Cur) inputs.  Replicas 4.. are dense: an inflation (i % 4 == 0), unrelated
    (1), equal (2) or Prev with further removals (3); under the collapsing map nearly all
    of them fail keyfind's comparison.  Replicas 0..3 hold at most one element of every
    second map group X div 3, so each key has one present slot and keyfind walks absent
    slots down the chain to reach it (for key 682 from slot 4087 to slot 4096, across the
    segment boundary): 0 grows (inflation, strict), 1 is equal (inflation, not strict),
    2 gains element 2046, an earlier slot of key 682 (keyfind meets another element: no
    inflation), 3 only gains removals (inflation, strict)."""
    rng = np.random.default_rng(seed)

    def reps():
        p = rng.integers(1, 8, (GI_R, GI_E)).astype(np.uint64)
        p[rng.random((GI_R, GI_E)) >= 0.8] = 0
        return np.stack([p, p & rng.integers(0, 8, (GI_R, GI_E)).astype(np.uint64)], axis=-1)
    a, x = reps(), reps()
    e = np.arange(GI_E)
    one = ((e // 3) % 2 == 0) & (e % 3 == (e // 6) % 3)
    assert one[GI_ONE] and not one[GI_ONE - 2]
    a[:4, ~one] = 0
    x[:4, ~one] = 0
    a[:4, GI_ONE] = (3, 0)
    b = a | x
    k = np.arange(GI_R) % 4
    b[k == 1] = x[k == 1]
    b[k == 2] = a[k == 2]
    b[k == 3] = a[k == 3]
    b[k == 3, :, 1] = a[k == 3, :, 0] & (a[k == 3, :, 1] | np.uint64(1))
    b[1] = a[1]
    b[2, GI_ONE - 2] = (1, 0)
    return a, b


GI_WANT = {False: [True, True, False, True], True: [True, False, False, True]}


@pytest.fixture(scope="module")
def gi_case():
    """Inputs, indexes and expected cells / verdicts of both pipelines, computed once."""
    out = {}
    for keyed, (F1, pred, F2) in GI_PIPES.items():
        f, comp, okeys = pipeline(GI_E, F1, pred, F2)
        assert len(f) > 4096
        a, b = gi_replicas(70 + keyed)
        sel = np.minimum(comp, GI_E - 1)
        ga = np.where((comp < GI_E)[None, :, None], a[:, sel], 0).astype(np.uint64)
        gb = np.where((comp < GI_E)[None, :, None], b[:, sel], 0).astype(np.uint64)
        zero = np.zeros_like(ga[0])
        want = {"first": [keyfind_threshold(zero, ga[i], comp, okeys, True)
                          for i in range(GI_R)]}
        for s in (False, True):
            want[s] = [keyfind_threshold(ga[i], gb[i], comp, okeys, s) for i in range(GI_R)]
            want["bc", s] = [keyfind_threshold(ga[0], gb[i], comp, okeys, s)
                             for i in range(GI_R)]
        if keyed:                              # the oracle lattice on the four sparse replicas
            for i in range(4):
                la, lb = oracle_list(a[i], F1, pred, F2), oracle_list(b[i], F1, pred, F2)
                assert exact_eq(device_list(ga[i], f, okeys), la)
                assert exact_eq(device_list(gb[i], f, okeys), lb)
                assert want[False][i] == olat.is_inflation("lasp_orset", la, lb), i
                assert want[True][i] == olat.is_strict_inflation("lasp_orset", la, lb), i
            assert want[False][:4] == GI_WANT[False] and want[True][:4] == GI_WANT[True]
        out[keyed] = (a, b, f, comp, okeys, ga, gb, want)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("g", [0, 1, 3])
@pytest.mark.parametrize("keyed", [True, False])
def test_gather_inflation_segments_and_strides(ctx, gi_case, keyed, g):
    """The fused gather + threshold over two 4096-slot segments and three runs of 8
    replicas (the last partial), with a block walking several (run, segment) items under
    grids 1 and 3: cells == numpy indexing, verdicts == the keyfind restatement on every
    replica (pinned to oracle.lattice on three), strict and not, with a per-replica and a
    broadcast Prev; each launch three times, so a partial record left dirty shows."""
    from lasp_amd.engine import key_chains
    a, b, f, comp, okeys, ga, gb, want = gi_case[keyed]
    chains = key_chains(okeys) if keyed else None
    n_out = len(f)
    A, B = ctx.orset_batch(GI_R, GI_E), ctx.orset_batch(GI_R, GI_E)
    A.upload(a.reshape(GI_R, -1))
    B.upload(b.reshape(GI_R, -1))
    fa, fb = ctx.orset_batch(GI_R, n_out), ctx.orset_batch(GI_R, n_out)
    empty = ctx.orset_batch(1, n_out)
    empty.clear()
    wa, wb = ga.reshape(GI_R, -1), gb.reshape(GI_R, -1)
    with knobs(ctx, grid=g):
        for _ in range(3):
            got = dirty(fa, wa).gather_inflation(A, comp, empty, strict=True, chains=chains)
            assert list(got) == want["first"]
            assert np.array_equal(fa.download_words(), wa)
            for s in (False, True):
                got = dirty(fb, wb).gather_inflation(B, comp, fa, strict=s, chains=chains)
                assert list(got) == want[s], s
                assert np.array_equal(fb.download_words(), wb)
                got = dirty(fb, wb).gather_inflation(B, comp, fa.view(0, 1), strict=s,
                                                     chains=chains)
                assert list(got) == want["bc", s], s
                assert np.array_equal(fb.download_words(), wb)


# ------------------------------------------------------------------ segment kernels

def orset_pairs(rng, R, E):
    """(prev, cur) OR-Set replicas: inflation, unrelated, equal, further removals, empty
    Prev, by replica index mod 5."""
    a = operands(rng, "orset", 1, R, E, 2 * E)[0].reshape(R, E, 2)
    x = operands(rng, "orset", 1, R, E, 2 * E)[0].reshape(R, E, 2)
    b = a | x
    k = np.arange(R) % 5
    b[k == 1] = x[k == 1]
    b[k == 2] = a[k == 2]
    b[k == 3] = a[k == 3]
    b[k == 3, :, 1] = a[k == 3, :, 0]
    a[k == 4] = 0
    b[k == 1, E - 1] = 0                       # a dropped last element: in the last segment
    return a, b


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("R,E", [s[:2] for s in SEG_SHAPES])
def test_orset_segment_kernels_stride(ctx, R, E, g):
    """stats / equal / (strict) inflation / filter of OR-Sets with g blocks walking all
    (replica, segment) items: against numpy over every replica and the orddict oracle on
    a few, three launches each."""
    rng = np.random.default_rng(7000 + R)
    prev, cur = orset_pairs(rng, R, E)
    P, Cb, F = ctx.orset_batch(R, E), ctx.orset_batch(R, E), ctx.orset_batch(R, E)
    P.upload(prev.reshape(R, -1))
    Cb.upload(cur.reshape(R, -1))
    pp, rp, pc, rc = prev[..., 0], prev[..., 1], cur[..., 0], cur[..., 1]
    viol = ((pp & ~pc) != 0).any(axis=1)
    changed = ((pp != 0) & (pc != 0) & ((pp != pc) | (rp != rc))).any(axis=1)
    npres, ncres = (pp != 0).sum(axis=1), (pc != 0).sum(axis=1)
    want_i = ~viol
    want_s = ~viol & (changed | (npres < ncres))
    want_st = np.stack([ncres, np.bitwise_count(pc & ~rc).sum(axis=1, dtype=np.int64),
                        np.bitwise_count(rc).sum(axis=1, dtype=np.int64)], axis=1)
    want_eq = (prev == cur).all(axis=(1, 2))
    assert want_i.any() and not want_i.all() and want_eq.any() and want_s.any()
    keep = bits_words(rng, ((E + 63) // 64,))
    kbit = np.unpackbits(keep.view(np.uint8), bitorder="little")[:E].astype(bool)
    want_f = np.where(kbit[None, :, None], cur, 0).astype(np.uint64).reshape(R, -1)
    tokens = orc.synth_tokens(E)
    for i in range(0, R, max(1, R // 3)):
        Dp, Dc = orc.ORDict.from_cells(prev[i], tokens), orc.ORDict.from_cells(cur[i], tokens)
        assert tuple(int(x) for x in want_st[i]) == Dc.stats()
        assert want_eq[i] == Dc.equal(Dp) and want_i[i] == Dc.is_inflation_of(Dp)
        assert want_s[i] == Dc.is_strict_inflation_of(Dp)
    with knobs(ctx, grid=g):
        for _ in range(3):
            assert np.array_equal(Cb.stats().astype(np.int64), want_st)
            assert np.array_equal(Cb.equal(P), want_eq)
            assert np.array_equal(Cb.is_inflation_of(P), want_i)
            assert np.array_equal(Cb.is_inflation_of(P, strict=True), want_s)
            assert Cb.equal(Cb).all()
            dirty(F, want_f).filter(Cb, keep)
            assert np.array_equal(F.download_words(), want_f)
        assert np.array_equal(Cb.is_inflation_of(P.view(0, 1)),     # a broadcast Prev
                              ~((pp[:1] & ~pc) != 0).any(axis=1))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
def test_orset_fragment_and_filter_bodies(ctx, g):
    """fragment with more replicas than 2 g blocks of lanes, and filter against the
    oracle's filter body."""
    rng = np.random.default_rng(7100 + g)
    R, E = 2000, 5
    h = operands(rng, "orset", 1, R, E, 2 * E)[0]
    b = ctx.orset_batch(R, E)
    b.upload(h)
    with knobs(ctx, grid=g):
        for e in (0, 3, 4):
            for _ in range(3):
                assert np.array_equal(b.fragment(e), h.reshape(R, E, 2)[:, e])
        R2, E2 = 12 * g, 70
        cells = operands(rng, "orset", 1, R2, E2, 2 * E2)[0].reshape(R2, E2, 2) & np.uint64(0xFF)
        S, F = ctx.orset_batch(R2, E2), ctx.orset_batch(R2, E2)
        S.upload(cells.reshape(R2, -1))
        keep = pack_rows((np.arange(E2) % 2 == 0)[None, :])[0]
        got = F.filter(S, keep).download()
    for i in range(0, R2, 5):
        assert dec(got[i]) == ocore.filter_body("lasp_orset", lambda x: x % 2 == 0,
                                                dec(cells[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("R,W", [s[:2] for s in SEG_SHAPES])
def test_gset_segment_kernels_stride(ctx, R, W, g):
    """stats / equal / (strict) inflation of G-Sets, g blocks walking all items."""
    rng = np.random.default_rng(7200 + R)
    E = 64 * W - 3
    prev = operands(rng, "gset", 1, R, E, W)[0]
    cur = prev | operands(rng, "gset", 1, R, E, W)[0]
    k = np.arange(R) % 4
    cur[k == 1] = prev[k == 1]
    cur[k == 2, W - 1] = 0                              # drops members of the last word
    prev[k == 2, W - 1] |= np.uint64(1)
    P, Cb = ctx.gset_batch(R, E), ctx.gset_batch(R, E)
    P.upload(prev)
    Cb.upload(cur)
    sub = ~((prev & ~cur) != 0).any(axis=1)
    same = (prev == cur).all(axis=1)
    want_st = np.bitwise_count(cur).sum(axis=1, dtype=np.uint64)
    assert sub.any() and not sub.all() and same.any()
    with knobs(ctx, grid=g):
        for _ in range(3):
            assert np.array_equal(Cb.stats(), want_st)
            assert np.array_equal(Cb.equal(P), same)
            assert np.array_equal(Cb.is_inflation_of(P), sub)
            assert np.array_equal(Cb.is_inflation_of(P, strict=True), sub & ~same)
    for i in range(0, R, max(1, R // 3)):
        assert int(want_st[i]) == len(orc.gset_members(cur[i], E))


@pytest.mark.gpu
@pytest.mark.parametrize("g", GRIDS)
@pytest.mark.parametrize("R,W", [s[:2] for s in SEG_SHAPES])
def test_gcounter_segment_kernels_stride(ctx, R, W, g):
    """values / threshold_met / (strict) inflation / increment of G-Counters, g blocks
    walking all items; counts above 2^63 decide two replicas' inflation."""
    rng = np.random.default_rng(7300 + R)
    prev = rng.integers(0, 1000, (R, W)).astype(np.uint64)
    cur = prev + rng.integers(0, 3, (R, W)).astype(np.uint64)
    k = np.arange(R) % 4
    cur[k == 1] = prev[k == 1]
    cur[k == 2, W - 1] = 0
    prev[k == 2, W - 1] = 5
    big = np.uint64(2**63 + 5)
    prev[0, W - 1], cur[0, W - 1] = 3, big              # unsigned: 3 <= 2^63 + 5
    prev[1, 0], cur[1, 0] = big, 3                      # unsigned: a violation
    P, Cb = ctx.gcounter_batch(R, W), ctx.gcounter_batch(R, W)
    P.upload(prev)
    Cb.upload(cur)
    sp, sc = prev.sum(axis=1, dtype=np.uint64), cur.sum(axis=1, dtype=np.uint64)
    want_i = (prev <= cur).all(axis=1)
    assert want_i[0] and not want_i[1] and want_i.any() and not want_i.all()
    nincs = 2 * 3 * KB + 301
    incs = [(int(r), int(a), int(m)) for r, a, m in zip(rng.integers(0, R, nincs),
                                                         rng.integers(0, min(W, 50), nincs),
                                                         rng.integers(1, 9, nincs))]
    with knobs(ctx, grid=g):
        for _ in range(3):
            assert np.array_equal(Cb.values(), sc)
            for t in (int(np.median(sc)), int(sc[2]), int(sc[2]) + 1, 0):
                assert list(Cb.threshold_met(t)) == [t <= int(x) for x in sc]
                assert list(Cb.threshold_met(t, strict=True)) == [t < int(x) for x in sc]
            assert np.array_equal(Cb.is_inflation_of(P), want_i)
            assert np.array_equal(Cb.is_inflation_of(P, strict=True), sp < sc)
        want_inc = prev.copy()
        np.add.at(want_inc, ([i[0] for i in incs], [i[1] for i in incs]),
                  np.array([i[2] for i in incs], np.uint64))
        P.increment(incs)
        assert np.array_equal(P.download(), want_inc)


# ------------------------------------------------------------------ last: defaults restored

@pytest.mark.gpu
def test_default_knobs_still_join(ctx):
    """Last in the file: with every knob back at its default, the 512 x 256 join of the
    parity tests still equals numpy."""
    R, E = 512, 256
    a, b = ctx.orset_batch(R, E), ctx.orset_batch(R, E)
    a.fill_synthetic(2)
    b.fill_synthetic(3)
    ha, hb = a.download_words(), b.download_words()
    guarded(ctx.orset_batch, R, 256, ha | hb, lambda v: v.join(a, b))
    tokens = orc.synth_tokens(E)
    c = ctx.orset_batch(R, E).join(a, b).download()
    for i in range(0, R, 101):
        orddict_merge_check(ha[i].reshape(E, 2), hb[i].reshape(E, 2), c[i], tokens)
