"""A pure-Python model of the resident map process (include/laspj.h "resident map
processes"), over the oracle.

The device keeps, per map, F's result for every element it has been asked about; a re-run
reports the held elements it has no result for (`pending`) and leaves the output alone, or —
none pending — binds map/6's AccValue (oracle.core.map_body with the recorded results,
lasp_core.erl:641-667) into the list-valued output the way tests/lvars_model.bind does
(bind/3, lasp_core.erl:291-312).

A map is refused (its results rolled back, FALLBACK from then on) when a result is `==` to a
registered term under another image, is a term kind the dictionary does not hold, or would
put more than 64 tokens under one output key.  The model tracks the namespace's registered
terms for that: `terms` (image -> term, elements) and `tokens` (key image -> token images).
"""

import lvars_model as lm
from oracle import core as ocore
from oracle import etf as oetf
from oracle.terms import Atom

NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
TOK_CAP = 64


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def holdable(t) -> bool:
    """The term kinds the host dictionary holds: integers, floats, atoms, binaries, tuples
    and lists of those."""
    if isinstance(t, (bool, int, float, bytes, Atom)):
        return True
    if isinstance(t, (tuple, list)):
        return all(holdable(x) for x in t)
    return False


def eq_class(t):
    """A hashable stand-in that is equal exactly when Erlang's `==` holds: Python compares
    1 and 1.0 equal (with one hash), tuples element-wise; lists become tagged tuples."""
    if isinstance(t, list):
        return ("$list",) + tuple(eq_class(x) for x in t)
    if isinstance(t, tuple):
        return tuple(eq_class(x) for x in t)
    return t


class MapModel:
    def __init__(self, fun):
        self.fun = fun
        self.results = {}        # image of an evaluated element -> F's result
        self.calls = []          # every argument F was called with, in order
        self.terms = {}          # the namespace's element terms by image
        self.classes = {}        # their `==` classes: eq_class(term) -> image
        self.tokens = {}         # element image -> set of token images registered under it
        self.mine = {}           # element image -> token images only this map put under it
        self.refused = False

    # -- the namespace's registrations (what write/update/bind of any variable walked in)
    def note_value(self, value):
        """A value some variable of the namespace has held: its keys and tokens are registered."""
        for k, toks in value:
            ki = tb(k)
            self.terms.setdefault(ki, k)
            self.classes.setdefault(eq_class(k), ki)
            self.tokens.setdefault(ki, set()).update(tb(t) for t, _f in toks)

    def pending(self, value):
        return [k for k, _toks in value if tb(k) not in self.results]

    def args(self, value):
        return self.pending(value)

    def _refusal(self, pend, res):
        """Whether recording res for pend refuses the map; else the registrations it makes."""
        terms, classes = dict(self.terms), dict(self.classes)
        tokens = {k: set(v) for k, v in self.tokens.items()}
        for x, y in zip(pend, res):
            if not holdable(y):
                return True, None
            yi = tb(y)
            if yi not in terms:
                if classes.setdefault(eq_class(y), yi) != yi:
                    return True, None
                terms[yi] = y
                tokens.setdefault(yi, set())
        # the tokens each X had registered when F was asked, now also under F(X); those the
        # map itself put under X stand for another input's and are not passed on
        mine = {k: set(v) for k, v in self.mine.items()}
        for x, y in zip(pend, res):
            xi, yi = tb(x), tb(y)
            own = set(self.tokens.get(xi, ())) - mine.get(xi, set())
            mine.setdefault(yi, set()).update(own - tokens[yi])
            tokens[yi] |= own
            if len(tokens[yi]) > TOK_CAP:
                return True, None
        return False, (terms, classes, tokens, mine)

    def evaluate(self, value):
        """F called on every pending element (args -> results): False when the map is
        refused by it (nothing recorded)."""
        pend = self.pending(value)
        res = []
        for x in pend:
            self.calls.append(x)
            res.append(self.fun(x))
        bad, regs = self._refusal(pend, res)
        if bad:
            self.refused = True
            return False
        self.terms, self.classes, self.tokens, self.mine = regs
        for x, y in zip(pend, res):
            self.results[tb(x)] = y
        return True

    def reset(self):
        """A dictionary reset: the device forgets every result, and a refusal."""
        self.results.clear()
        self.terms.clear()
        self.classes.clear()
        self.tokens.clear()
        self.mine.clear()
        self.refused = False

    def acc(self, value):
        """map/6's AccValue with the recorded results (nothing may be pending)."""
        return ocore.map_body(lm.TYPE, lambda x: self.results[tb(x)], value)

    def run(self, value, out):
        """One laspj_map_run: (status, pending, new out)."""
        pend = len(self.pending(value))
        if pend:
            return NOOP, pend, out
        acc = self.acc(value)
        st, new = lm.bind(out, acc)
        # minted tokens are named under their keys by the run itself
        for k, toks in acc:
            ki = tb(k)
            got = {tb(t) for t, _f in toks}
            self.mine.setdefault(ki, set()).update(got - self.tokens.setdefault(ki, set()))
            self.tokens[ki] |= got
        return st, 0, new

    def step(self, value, out):
        """NifMap.step: (status, pending of the first run, new out); None when refused."""
        self.note_value(value)
        first = len(self.pending(value))
        if first and not self.evaluate(value):
            return None
        st, _p, new = self.run(value, out)
        return st, first, new
