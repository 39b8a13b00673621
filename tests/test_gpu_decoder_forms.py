"""The two forms of the OR-Set segment decoders (LASPJ_TUNE_ETF_OCC; DESIGN.md §4
"Under-filled segment launches"): the filled form (256 threads at 6 waves per SIMD) and
the under-filled one (one wave per workgroup, no register spills) decode the same segments
with the same code, so every case here runs under both (knob 1, then 2, a fresh context
each) with 256-byte segments (LASPJ_TUNE_ETF_SEG) and must give

  * the oracle's image and verdict (oracle/orset.py's merge and the ETF restatement
    oracle/etf.py — never the library's own output), and
  * each other's nif_stats deltas for registrations, chain_redo_passes and fallbacks.

The cases reach k_orset_etf_read_seg<SMALL> (elements of <= 8 token slots) and <false>
(12 tokens per element: segments in which no element starts), k_orset_etf_read_seg_multi
(bind_many over three namespaces), the edges (a second segment of one byte, [], one
element), the failure paths (an unseen token deep in the image, false element headers
inside tokens, an image cut mid-element) and the wave stride over segments
(LASPJ_TUNE_STREAM_GRID caps these launches' grids).

Reference: lasp_orset.erl:128-134 (merge/2); lasp_core.erl:298-311 (bind/3).
"""

import functools

import pytest

from oracle import etf as oetf
from oracle import orset as oorset
from oracle.terms import compare

pytestmark = pytest.mark.gpu

OK, FALLBACK = 0, 1
FILLED, UNDER = 1, 2
KEYS = ("registrations", "chain_redo_passes", "fallbacks")

_key = functools.cmp_to_key(compare)


def _tb(t) -> bytes:
    return oetf.term_to_binary(t)


def _tok(e: int, k: int) -> bytes:
    """20 bytes, distinct per (element, k), ascending in k within an element."""
    return bytes([k]) + e.to_bytes(2, "big") + bytes([(7 * e + k) % 256]) * 17


def _state(elems, ks, flag=lambda e, k: (e + k) % 3 == 0):
    return [(e, sorted([(_tok(e, k), flag(e, k)) for k in ks], key=lambda x: _key(x[0])))
            for e in elems]


@functools.lru_cache(maxsize=None)
def _small():
    """1,200 elements x 2 tokens against two in three of them x 2 (one shared): elements
    straddle every 256-byte boundary.  (a, b, merge) with their images."""
    a = _state(range(1200), (0, 1))
    b = _state([e for e in range(1200) if e % 3], (1, 2), flag=lambda e, k: e % 5 == 0)
    m = oorset.merge(a, b)
    return a, b, m, _tb(a), _tb(b), _tb(m)


@functools.lru_cache(maxsize=None)
def _many_token():
    """The same with 12 tokens per element (more than 400 bytes each): most 256-byte
    segments hold no element start, and the many-token decoder runs."""
    a = _state(range(1200), range(12))
    b = _state([e for e in range(1200) if e % 3], range(1, 13), flag=lambda e, k: e % 5 == 0)
    m = oorset.merge(a, b)
    return a, b, m, _tb(a), _tb(b), _tb(m)


@functools.lru_cache(maxsize=None)
def _image_257():
    """An orddict whose image is 257 bytes: two segments, the second one byte long."""
    s = _state((3, 5), (0,), flag=lambda e, k: True) + \
        _state((700, 900), (0, 1), flag=lambda e, k: True)
    img = _tb(s)
    assert len(img) == 257, len(img)
    return s, img


def _ctx(form, grid=0):
    from lasp_amd import _lib, engine
    ctx = engine.Context(0)
    ctx.set_tuning(_lib.TUNE_ETF_SEG, 256)
    ctx.set_tuning(_lib.TUNE_ETF_OCC, form)
    if grid:
        ctx.set_tuning(_lib.TUNE_STREAM_GRID, grid)
    return ctx


def _delta(s0, s1):
    return {k: s1[k] - s0[k] for k in KEYS}


def _both(run, **kw):
    """run(ctx) under each form on a fresh context: its stats deltas, which must agree."""
    out = {}
    for form in (FILLED, UNDER):
        ctx = _ctx(form, **kw)
        try:
            out[form] = run(ctx)
        finally:
            ctx.close()
    assert out[FILLED] == out[UNDER], out
    return out[FILLED]


def _merge_and_bind(ctx, case):
    """nif_merge and a resident bind of the case, both against the oracle; the stats
    deltas of the warm merge and of the bind."""
    a, b, m, ia, ib, im = case
    assert ctx.nif_merge(ia, ib) == (OK, im)
    s0 = ctx.nif_stats()
    assert ctx.nif_merge(ia, ib) == (OK, im)                  # warm: every term known
    s1 = ctx.nif_stats()
    var = ctx.var("orset")
    assert var.write(ia) == OK
    assert var.bind(ib) == (OK, 1)
    assert var.read() == (OK, im)
    assert var.bind(im) == (OK, 0)                            # Value0 =:= Value: a no-op
    assert var.read() == (OK, im)
    s2 = ctx.nif_stats()
    var.close()
    return _delta(s0, s1), _delta(s1, s2)


def test_single_dictionary_small():
    assert len(_small()[4]) > 200 * 256                      # > 200 segments in b alone
    warm, bind = _both(lambda ctx: _merge_and_bind(ctx, _small()))
    assert warm == {"registrations": 0, "chain_redo_passes": 0, "fallbacks": 0}
    assert bind["fallbacks"] == 0 and bind["chain_redo_passes"] == 0


def test_single_dictionary_many_token():
    a = _many_token()[0]
    assert len(_tb(a[:1])) - 7 > 400                         # one element's image
    warm, bind = _both(lambda ctx: _merge_and_bind(ctx, _many_token()))
    assert warm == {"registrations": 0, "chain_redo_passes": 0, "fallbacks": 0}
    assert bind["fallbacks"] == 0 and bind["chain_redo_passes"] == 0


def test_stride_over_segments():
    """Two workgroups: each wave takes many segments (the decoders' j += nwaves loop)."""
    warm, bind = _both(lambda ctx: _merge_and_bind(ctx, _small()), grid=2)
    assert warm == {"registrations": 0, "chain_redo_passes": 0, "fallbacks": 0}
    assert bind["fallbacks"] == 0 and bind["chain_redo_passes"] == 0


def test_multi_kernel_bind_many():
    """bind_many over three variables, each in a namespace of its own: a SMALL one, a
    many-token one and one whose image is a single segment."""
    tiny_a = _state((1, 2), (0,))
    tiny_b = _state((2, 4), (0, 1))
    assert len(_tb(tiny_b)) <= 256
    tiny_m = oorset.merge(tiny_a, tiny_b)
    cases = (_small(), _many_token(),
             (tiny_a, tiny_b, tiny_m, _tb(tiny_a), _tb(tiny_b), _tb(tiny_m)))

    def run(ctx):
        vs = [ctx.var("orset") for _ in cases]
        for v, c in zip(vs, cases):
            assert v.write(c[3]) == OK
        s0 = ctx.nif_stats()
        assert ctx.var_bind_many([(v, c[4]) for v, c in zip(vs, cases)]) == [(OK, 1)] * 3
        for v, c in zip(vs, cases):
            assert v.read() == (OK, c[5])
        assert ctx.var_bind_many([(v, c[5]) for v, c in zip(vs, cases)]) == [(OK, 0)] * 3
        for v, c in zip(vs, cases):
            assert v.read() == (OK, c[5])
        d = _delta(s0, ctx.nif_stats())
        for v in vs:
            v.close()
        return d

    d = _both(run)
    assert d["fallbacks"] == 0 and d["chain_redo_passes"] == 0


def test_edges():
    """A 257-byte image (its second segment one byte), [] and a one-element image, merged
    with and bound into the 1,200-element state."""
    a, _b, _m, ia, _ib, _im = _small()
    s257, i257 = _image_257()
    one = _state((77,), (5,))
    edges = [(s257, i257), ([], _tb([])), (one, _tb(one))]
    assert _tb([]) == bytes([131, 106])

    def run(ctx):
        s0 = ctx.nif_stats()
        for s, img in edges:
            assert ctx.nif_merge(ia, img) == (OK, _tb(oorset.merge(a, s)))
            assert ctx.nif_merge(img, ia) == (OK, _tb(oorset.merge(s, a)))
            assert ctx.nif_merge(img, img) == (OK, _tb(oorset.merge(s, s)))
        var = ctx.var("orset")
        assert var.write(ia) == OK
        cur = a
        for s, img in edges:
            nxt = oorset.merge(cur, s)
            # bind/3 is a no-op only when Value0 =:= Value (lasp_core.erl:294-296); any
            # other canonical value is merged and written, [] too
            assert var.bind(img) == (OK, int(s != cur))
            cur = nxt
            assert var.read() == (OK, _tb(cur))
        small = ctx.var("orset")                              # a variable holding 257 bytes
        assert small.write(i257) == OK
        assert small.read() == (OK, i257)
        assert small.bind(_tb(one)) == (OK, 1)
        assert small.read() == (OK, _tb(oorset.merge(s257, one)))
        d = _delta(s0, ctx.nif_stats())
        var.close()
        small.close()
        return d

    d = _both(run)
    assert d["fallbacks"] == 0


def test_unseen_token_deep_in_the_image():
    """A token the namespace has not seen, on element 1,100 of 1,200: the segment's
    UNKNOWN_TERM is exact, one term is registered and the answer is the oracle's — no
    serial pass, no fallback; the resident bind takes the token in its one pass."""
    a, b, _m, ia, ib, im = _small()
    new = (b"\x05" * 20, True)
    b2 = [(e, sorted(ts + [new], key=lambda x: _key(x[0])) if e == 1100 else ts)
          for e, ts in b]
    assert b2 != b
    m2 = oorset.merge(a, b2)

    def run(ctx):
        assert ctx.nif_merge(ia, ib) == (OK, im)
        var = ctx.var("orset")
        assert var.write(ia) == OK and var.bind(ib) == (OK, 1)
        s0 = ctx.nif_stats()
        assert ctx.nif_merge(ia, _tb(b2)) == (OK, _tb(m2))
        s1 = ctx.nif_stats()
        assert var.bind(_tb(b2)) == (OK, 1)
        s2 = ctx.nif_stats()
        assert var.read() == (OK, _tb(m2))
        assert s2["device_passes"] - s1["device_passes"] == 1
        var.close()
        return _delta(s0, s1), _delta(s1, s2)

    merge, bind = _both(run)
    assert merge == {"registrations": 1, "chain_redo_passes": 0, "fallbacks": 0}
    assert bind["fallbacks"] == 0 and bind["chain_redo_passes"] == 0


def test_false_element_headers_break_the_chain():
    """Tokens embedding 106 104 2 97 e 108 plant false segment starts: the chain check
    fails and the serial redo answers the oracle's merge."""
    trap = lambda e, k: bytes([106, 104, 2, 97, e, 108]) + bytes([k]) * 14   # noqa: E731
    tok = lambda e, k: (trap((e + 7) % 200, k) if e % 5 == 0  # noqa: E731
                        else bytes([k, e % 256]) * 10)
    a = [(e, sorted([(tok(e, k), (e + k) % 3 == 0) for k in range(2)],
                    key=lambda x: _key(x[0]))) for e in range(1200)]
    b = [(e, sorted([(tok(e, k), (e + k) % 4 == 0) for k in range(1, 3)],
                    key=lambda x: _key(x[0]))) for e in range(0, 1200, 2)]
    m = oorset.merge(a, b)
    ia, ib, im = _tb(a), _tb(b), _tb(m)

    def run(ctx):
        assert ctx.nif_merge(ia, ib) == (OK, im)
        s0 = ctx.nif_stats()
        assert ctx.nif_merge(ia, ib) == (OK, im)              # warm
        s1 = ctx.nif_stats()
        var = ctx.var("orset")
        assert var.write(ia) == OK
        assert var.bind(ib) == (OK, 1)
        assert var.read() == (OK, im)
        s2 = ctx.nif_stats()
        var.close()
        return _delta(s0, s1), _delta(s1, s2)

    merge, bind = _both(run)
    assert merge["chain_redo_passes"] > 0
    assert merge["registrations"] == 0 and merge["fallbacks"] == 0
    assert bind["fallbacks"] == 0


def test_image_truncated_mid_element():
    """b cut inside its 400th element: binary_to_term fails, the verdict is FALLBACK and
    the variable keeps its value."""
    a, b, _m, ia, ib, _im = _small()
    cut = len(_tb(b[:400])) - 1 + 10                          # 10 bytes into element 400
    trunc = ib[:cut]
    assert ib[cut - 10:cut - 7] == bytes([104, 2, 98])        # that element's header

    def run(ctx):
        assert ctx.nif_merge(ia, ia) == (OK, ia)
        var = ctx.var("orset")
        assert var.write(ia) == OK
        s0 = ctx.nif_stats()
        assert ctx.nif_merge(ia, trunc) == (FALLBACK, None)
        assert ctx.nif_merge(trunc, ia) == (FALLBACK, None)
        assert var.read() == (OK, ia)
        assert var.bind(trunc)[0] == FALLBACK
        assert var.read() == (OK, ia)
        d = _delta(s0, ctx.nif_stats())
        var.close()
        return d

    d = _both(run)
    assert d["fallbacks"] > 0 and d["registrations"] == 0
