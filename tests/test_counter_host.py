"""The counter image codec of the C ABI on the host (no GPU): laspj_gcounter_etf_parse /
_encode / laspj_gcounter_threshold_plan against the oracle's riak_dt_gcounter restatement
(oracle/core.py: _GCounter), its external term format (oracle/etf.py) and
lasp_lattice.erl:87-90 (oracle.lattice.threshold_met)."""

import ctypes as C
import os
import shutil
import subprocess

import pytest
from hypothesis import given, settings, strategies as st

import counters_model as cm
from counters_model import A, tb
from lasp_amd import _lib, build
from oracle import etf as oetf
from oracle import lattice as olat
from oracle import otp
from oracle.terms import eq, exact_eq

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "counter_images.txt")
SOAK = int(os.environ.get("LASPJ_SOAK", "1"))


@pytest.fixture(scope="module")
def lib():
    build.build()
    return _lib.load()


class Dict:
    """A laspj_dict of actor terms and the codec calls over it."""

    def __init__(self, lib):
        self.L, self.h = lib, C.c_void_p()
        assert lib.laspj_dict_create(C.byref(self.h)) == 0

    def close(self):
        self.L.laspj_dict_destroy(self.h)

    def size(self):
        e, eb, tk = C.c_uint32(), C.c_uint64(), C.c_uint64()
        assert self.L.laspj_dict_info(self.h, C.byref(e), C.byref(eb), C.byref(tk)) == 0
        return e.value

    def parse(self, img, cap=4096):
        """(status, [(slot, count)])"""
        slots, counts = (C.c_uint32 * cap)(), (C.c_uint64 * cap)()
        n, stt = C.c_uint32(), C.c_int32(-1)
        rc = self.L.laspj_gcounter_etf_parse(self.h, bytes(img), len(img), slots, counts, cap,
                                             C.byref(n), C.byref(stt))
        assert rc == 0, rc
        return stt.value, [(slots[k], counts[k]) for k in range(n.value)]

    def encode(self, pairs):
        n = len(pairs)
        slots = (C.c_uint32 * max(n, 1))(*[s for s, _c in pairs])
        counts = (C.c_uint64 * max(n, 1))(*[c for _s, c in pairs])
        cap = 1 << 20
        out, ln = C.create_string_buffer(cap), C.c_uint64()
        assert self.L.laspj_gcounter_etf_encode(self.h, slots, counts, n, out, cap,
                                                C.byref(ln)) == 0
        return out.raw[:ln.value]


def plan(lib, img, strict):
    p, t = C.c_int32(-1), C.c_uint64()
    rc = lib.laspj_gcounter_threshold_plan(bytes(img), len(img), int(strict), C.byref(p),
                                           C.byref(t))
    return rc, p.value, t.value


ACTORS = st.one_of(
    st.integers(min_value=-(1 << 70), max_value=1 << 70),
    st.sampled_from([A("a"), A("b"), A("client1"), A("")]),
    st.binary(max_size=6),
    st.tuples(st.integers(0, 9), st.sampled_from([A("t"), A("u")])))


@st.composite
def orddicts(draw):
    actors = draw(st.lists(ACTORS, max_size=12))
    c = []
    for a in actors:
        if otp.orddict_find(a, c) is None:
            c = otp.orddict_store(a, draw(st.sampled_from(cm.COUNTS)), c)
    return c


@settings(max_examples=150 * SOAK, deadline=None)
@given(orddicts(), orddicts())
def test_parse_and_encode_round_trip(lib, c, other):
    """parse(tb(c)) gives the counter back through the dictionary, and encode reproduces
    term_to_binary(c) byte for byte — over a dictionary that already holds another
    counter's actors (slots are not in term order)."""
    d = Dict(lib)
    try:
        # (an actor `==` to one of c's under another image would be EQUAL_TERMS: not here)
        other = [(a, n) for a, n in other
                 if not any(eq(a, b) and not exact_eq(a, b) for b, _ in c)]
        assert d.parse(tb(other))[0] == 0
        stt, pairs = d.parse(tb(c))
        assert stt == 0
        assert [n for _s, n in pairs] == [n for _a, n in c]
        assert len({s for s, _n in pairs}) == len(c)
        assert d.encode(pairs) == tb(c)
        # the same actors get the same slots again, and nothing new is registered
        size = d.size()
        assert d.parse(tb(c)) == (0, pairs) and d.size() == size
    finally:
        d.close()


def test_every_count_encoding(lib):
    d = Dict(lib)
    c = [(k, n) for k, n in enumerate(cm.COUNTS)]
    stt, pairs = d.parse(tb(c))
    assert stt == 0 and [n for _s, n in pairs] == cm.COUNTS
    img = d.encode(pairs)
    assert img == tb(c)
    assert {oetf._enc(n)[0] for n in cm.COUNTS} == {97, 98, 110}
    # zero counts are absent actors: skipped
    assert d.encode([(s, 0) for s, _n in pairs]) == tb([])
    # any ETF integer encoding is read: a small count as INTEGER_EXT / SMALL_BIG / LARGE_BIG
    for enc in (bytes([98, 0, 0, 0, 7]), bytes([110, 3, 0, 7, 0, 0]),
                bytes([111, 0, 0, 0, 9, 0, 7, 0, 0, 0, 0, 0, 0, 0, 0])):
        raw = bytes([131, 108, 0, 0, 0, 1, 104, 2, 97, 0]) + enc + bytes([106])
        assert d.parse(raw) == (0, [(pairs[0][0], 7)])
    d.close()


@pytest.mark.parametrize("name", sorted(cm.REFUSED))
def test_refused_images_register_nothing(lib, name):
    d = Dict(lib)
    assert d.parse(tb([(A("known"), 3), (A("other"), 4)]))[0] == 0
    size = d.size()
    stt, pairs = d.parse(cm.REFUSED[name])
    assert stt != 0 and pairs == [] and d.size() == size
    # and the dictionary still serves: the journal undid exactly that call
    assert d.parse(tb([(A("known"), 5), (A("zz"), 1)]))[0] == 0 and d.size() == size + 1
    d.close()


def test_equal_terms_under_another_image(lib):
    """an actor `==` to a registered term under another image (1 vs 1.0)"""
    d = Dict(lib)
    assert d.parse(tb([(1, 2)]))[0] == 0
    size = d.size()
    assert d.parse(tb([(1.0, 2), (A("new"), 1)])) == (6, [])      # LASPJ_DEC_EQUAL_TERMS
    assert d.size() == size
    d.close()


def test_truncated_at_every_cut(lib):
    d = Dict(lib)
    for img in cm.truncated():
        stt, pairs = d.parse(img)
        assert stt != 0 and pairs == [] and d.size() == 0, len(img)
    d.close()


def test_more_pairs_than_room(lib):
    d = Dict(lib)
    slots, counts = (C.c_uint32 * 2)(), (C.c_uint64 * 2)()
    n, stt = C.c_uint32(), C.c_int32()
    img = tb([(k, 1) for k in range(5)])
    assert lib.laspj_gcounter_etf_parse(d.h, img, len(img), slots, counts, 2, C.byref(n),
                                        C.byref(stt)) == _lib.E_RANGE
    assert n.value == 5
    d.close()


@pytest.mark.parametrize("strict", [False, True])
@pytest.mark.parametrize("th", cm.THRESHOLDS, ids=repr)
def test_threshold_plan_against_the_lattice(lib, th, strict):
    rc, p, t = plan(lib, tb(th), strict)
    assert rc == 0 and p in (_lib.GC_NEVER, _lib.GC_ALWAYS, _lib.GC_T)
    for v in cm.SUMS:
        want = olat.threshold_met(cm.TYPE, [(A("a"), v)] if v else [],
                                  ("strict", th) if strict else th)
        got = p == _lib.GC_ALWAYS or (p == _lib.GC_T and t <= v)
        assert got == want, (th, strict, v, p, t)


@settings(max_examples=300 * SOAK, deadline=None)
@given(st.one_of(st.integers(min_value=-(1 << 70), max_value=1 << 70),
                 st.floats(allow_nan=False, allow_infinity=True, width=64)),
       st.booleans())
def test_threshold_plan_is_the_mirrors(lib, th, strict):
    """the C plan is lasp_amd/gcounter.py:threshold_plan's, and both are term order's"""
    from lasp_amd import gcounter as dg
    rc, p, t = plan(lib, tb(th), strict)
    const, dev_t = dg.threshold_plan(th, strict)
    assert rc == 0
    if const is None:
        assert (p, t) == (_lib.GC_T, dev_t)
    else:
        assert p == (_lib.GC_ALWAYS if const else _lib.GC_NEVER)


def test_threshold_plan_refuses_what_is_no_term(lib):
    for img in (b"", b"\x83", tb(5)[:-1], tb(1 << 40)[:-2], tb(5) + b"\x00"):
        assert plan(lib, img, False)[0] == _lib.E_INVAL


def test_fixture_is_the_models():
    """tests/golden/counter_images.txt is counters_model.fixture_lines() (regenerate it from
    there when the cases change)"""
    assert open(FIXTURE).read().split("\n") == cm.fixture_lines() + [""]


def test_codec_under_host_sanitizers(tmp_path):
    """A stand-alone program over the two host sources, built with the address and
    undefined-behaviour sanitizers, reads the fixture's valid, refused and truncated images
    (each from a heap block of exactly its length) and must end clean.  Nothing loaded into
    Python runs under a sanitizer."""
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(build.HIPCC)))
    cands = [os.path.join(rocm, "llvm", "bin", "clang++"),
             os.path.join(rocm, "lib", "llvm", "bin", "clang++"), shutil.which("clang++")]
    cxx = next((c for c in cands if c and os.path.exists(c)), None)
    assert cxx is not None, "no host clang++ beside hipcc"
    exe = str(tmp_path / "counter_host_check")
    # plain host C++ (the sources hold no kernels): the HIP headers only declare
    cmd = [cxx, "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
           "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined",
           os.path.join(ROOT, "tests", "c", "counter_host_check.cpp"),
           os.path.join(build.CSRC, "laspj_counter_host.cpp"),
           os.path.join(build.CSRC, "laspj_host.cpp"), "-o", exe]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-4000:]
    res = subprocess.run([exe, FIXTURE], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    assert " 0 bad" in res.stdout
