"""A pure-Python model of the resident filter process and the resident G-Set intersection
(include/laspj.h "resident filter processes"), over the oracle.

The device keeps, per filter, which elements Function has been called for and what it
answered; a re-run reports the held elements it has no answer for (`pending`) and leaves the
output alone, or — none pending — binds filter/6's AccValue (oracle.core.filter_body with
the recorded answers) the way bind/3 does: `Value0 =:= AccValue` decides the status, then
Type:merge/2.  The model does the same with a dict of element images.
"""

from oracle import core as ocore
from oracle import etf as oetf
from oracle import gset as ogset
from oracle import orset as oorset
from oracle.terms import exact_eq

NOOP, WRITTEN = 0, 1
_MERGE = {"lasp_orset": oorset.merge, "lasp_gset": ogset.merge}


def bind(type_, out, acc):
    """bind/3 (lasp_core.erl:291-312) of acc into out: (status, new out)."""
    if exact_eq(out, acc):
        return NOOP, out
    return WRITTEN, _MERGE[type_](out, acc)


class FilterModel:
    def __init__(self, type_, fun):
        self.type_, self.fun = type_, fun
        self.results = {}        # image of an evaluated element -> Function's answer
        self.calls = []          # every argument Function was called with, in order

    def elements(self, value):
        """The entries the body folds over, in the value's (term) order."""
        return [k for k, _toks in value] if self.type_ == "lasp_orset" else list(value)

    def arg(self, element):
        """What the body hands to Function: the OR-Set key; a G-Set element, or the first
        component of one that is a 2-tuple (`{X, _} -> X`, lasp_core.erl:688-695)."""
        if self.type_ == "lasp_gset" and isinstance(element, tuple) and len(element) == 2:
            return element[0]
        return element

    def pending(self, value):
        return [e for e in self.elements(value) if oetf.term_to_binary(e) not in self.results]

    def args(self, value):
        return [self.arg(e) for e in self.pending(value)]

    def evaluate(self, value):
        """Function called on every pending element (args -> results)."""
        for e in self.pending(value):
            a = self.arg(e)
            self.calls.append(a)
            self.results[oetf.term_to_binary(e)] = self.fun(a)

    def reset(self):
        """A dictionary reset: the device forgets every answer."""
        self.results.clear()

    def acc(self, value):
        """filter/6's AccValue with the recorded answers (nothing may be pending)."""
        it = iter(self.elements(value))
        return ocore.filter_body(self.type_,
                                 lambda _v: self.results[oetf.term_to_binary(next(it))], value)

    def run(self, value, out):
        """One laspj_filter_run: (status, pending, new out)."""
        pend = len(self.pending(value))
        if pend:
            return NOOP, pend, out
        st, new = bind(self.type_, out, self.acc(value))
        return st, 0, new

    def step(self, value, out):
        """NifFilter.step: (status, pending of the first run, new out)."""
        first = len(self.pending(value))
        self.evaluate(value)
        st, _p, new = self.run(value, out)
        return st, first, new


def intersection(l, r, out):
    """laspj_var_intersection on G-Sets: (status, new out)."""
    return bind("lasp_gset", out, ocore.intersection_body("lasp_gset", l, r))
