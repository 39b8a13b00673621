"""A reference model of riak_dt_gcounter variables at the drop-in boundary, shared by
tests/test_counter_host.py (no GPU) and tests/test_gpu_counters.py.

The value model is oracle/core.py's _GCounter (update/3, merge/2: the orddict Actor -> Count,
per-actor max); thresholds are oracle.lattice.threshold_met("riak_dt_gcounter", ...)
(lasp_lattice.erl:87-90); the waiting list is reply_to_all's (lasp_core.erl:765-825), as
tests/waiters_model.py models it for sets: met waiters leave in list order, the rest stay.
"""

from oracle import core as ocore
from oracle import etf as oetf
from oracle import lattice as olat
from oracle.terms import Atom, exact_eq

A = Atom
OK, FALLBACK = 0, 1
NOOP, WRITTEN = 0, 1
GC = ocore._GCounter
TYPE = "riak_dt_gcounter"
M64 = (1 << 64) - 1

# the counts the encodings turn on: SMALL_INTEGER_EXT up to 255, INTEGER_EXT up to 2^31 - 1,
# SMALL_BIG_EXT of 4 .. 8 bytes above
COUNTS = [1, 255, 256, (1 << 31) - 1, 1 << 31, 1 << 32, 1 << 63, M64]


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def total(c) -> int:
    """riak_dt_gcounter:value/1 as the device sums it: modulo 2^64."""
    return GC.value(c) & M64


class CounterModel:
    """One replica: its orddict and its waiting_threads, (id, strict, threshold) in order."""

    def __init__(self):
        self.value = []
        self.waiting = []

    def increment(self, op, actor):
        """lasp_core:update/4: {ok, V} = update(Op, Actor, V0), then bind(V)."""
        self.value = GC.update(op, actor, self.value)[1]

    def bind(self, other):
        """bind/3 (lasp_core.erl:291-312): NOOP iff Value0 =:= Value, else the merge is
        written (also when it equals Value0)."""
        if exact_eq(self.value, other):
            return NOOP
        self.value = GC.merge(self.value, other)
        return WRITTEN

    def met(self, strict, th):
        v = [(A("sum"), total(self.value))] if total(self.value) else []
        return olat.threshold_met(TYPE, v, ("strict", th) if strict else th)

    def wait(self, th, strict, wid):
        if self.met(strict, th):
            return True
        self.waiting.append((wid, bool(strict), th))
        return False

    def reply(self):
        """reply_to_all/3: the ids of the waiters met, in list order; they leave."""
        flags = [self.met(s, th) for _i, s, th in self.waiting]
        fired = [w[0] for w, f in zip(self.waiting, flags) if f]
        self.waiting = [w for w, f in zip(self.waiting, flags) if not f]
        return fired

    def cancel(self, wid):
        for k, w in enumerate(self.waiting):
            if w[0] == wid:
                del self.waiting[k]
                return True
        return False

    def listing(self):
        return [(i, s, tb(th)) for i, s, th in self.waiting]


def improper_list() -> bytes:
    """[{a, 1} | 1]: LIST_EXT whose tail is not NIL."""
    return bytes([131, 108, 0, 0, 0, 1]) + oetf._enc((A("a"), 1)) + bytes([97, 1])


# images the parser takes, and what it must refuse (name -> image)
VALID = [
    [],
    [(A("a"), 1)],
    [(1, 255), (2, 256), (A("a"), (1 << 31) - 1), (A("b"), 1 << 31), ((1, A("t")), 1 << 32),
     (b"bin", 1 << 63), (b"bio", M64)],
    [(k, k + 1) for k in range(70)],
    [(1.0, 3), (A("x"), 4)],
]

REFUSED = {
    "descending": tb([(2, 1), (1, 1)]),
    "duplicate": tb([(A("a"), 1), (A("a"), 2)]),
    "zero": tb([(A("a"), 0)]),
    "negative": tb([(A("a"), -1)]),
    "negative_big": tb([(A("a"), -(1 << 40))]),
    "two64": tb([(A("a"), 1 << 64)]),
    "float": tb([(A("a"), 1.5)]),
    "improper": improper_list(),
    "triple": tb([(A("a"), 1, 2)]),
    "int_and_float": tb([(1, 1), (1.0, 2)]),
    "float_and_int": tb([(1.0, 1), (1, 2)]),
    "not_tuples": tb([A("a"), A("b")]),
    "string": tb([1, 2, 3]),
    "atom": tb(A("a")),
    "second_bad": tb([(A("a"), 1), (A("b"), 0)]),
}


def truncated():
    """every proper prefix of an image with every integer encoding in it"""
    img = tb(VALID[2])
    return [img[:k] for k in range(len(img))]


def fixture_lines():
    """tests/golden/counter_images.txt, line by line: V / R / T and the image in hex."""
    out = [f"V {tb(c).hex()}" for c in VALID]
    out += [f"R {img.hex()}" for _n, img in sorted(REFUSED.items())]
    out += [f"T {img.hex() or '-'}" for img in truncated()]
    return out


# thresholds of the planner's cases (lasp_lattice.erl:87-90), and the sums they are put to
THRESHOLDS = [-1, 0, 5, 5.0, 4.5, (1 << 53) + 1, float(1 << 64), 1 << 64, [], A("undefined")]
SUMS = [0, 1, 5, 1 << 53, M64]
