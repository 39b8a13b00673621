"""A pure-Python model of a list-valued resident variable (include/laspj.h "list-valued
resident variables"), clause by clause over the oracle.

The variable holds any list of {Key, [{Token, Bool}]}.  bind/3 (lasp_core.erl:291-312) on
it: `Value0 =:= Value` answers NOOP; otherwise Merged = lasp_orset:merge(Value0, Value)
(orddict:merge run as written over lists that need not be orddicts) is written only when
is_inflation(Value0, Merged) holds (:301-307) — on such lists it may not, which canonical
values never show: REFUSED.  The intersection re-run binds intersection/7's OR-Set body
(:559-568, 583).
"""

from oracle import core as ocore
from oracle import lattice as olattice
from oracle import orset as oorset
from oracle.terms import Atom, exact_eq

NOOP, WRITTEN, REFUSED = 0, 1, 2
TYPE = "lasp_orset"

# bind/3 refuses VALUE into VALUE0: orddict:merge walks VALUE0's descending keys as if they
# ascended, so the merged list meets key 1 first with VALUE's token only, and is_inflation's
# lists:keyfind takes that first match (lasp_lattice.erl:153-161)
REFUSED_VALUE0 = [(2, [(b"a", False)]), (1, [(b"b", False)])]
REFUSED_VALUE = [(1, [(b"c", False)])]
# written from []: the keys descend, so the value is no orddict and leaves the rank-indexed
# bind at its next re-run
DESCENDING = [(Atom("z"), [(b"t1", False)]), (7, [(b"t2", True)]), (3, [(b"t0", False), (b"t3", False)])]


def bind(value0, value):
    """bind/3 of value into value0: (status, new value)."""
    if exact_eq(value0, value):
        return NOOP, value0
    merged = oorset.merge(value0, value)
    if olattice.is_inflation(TYPE, value0, merged):
        return WRITTEN, merged
    return REFUSED, value0


def acc_value(l, r):
    """intersection/7's AccValue over two OR-Set values: {X, Cx ++ Cy} per hit."""
    return ocore.intersection_body(TYPE, l, r)


def intersection(l, r, out):
    """laspj_lvar_intersection: (status, new out)."""
    return bind(out, acc_value(l, r))


def value(v):
    """lasp_orset:value/1 (lasp_orset.erl:67-73) on the list."""
    return oorset.value(v)


def counts(v):
    return len(v), sum(len(toks) for _k, toks in v)


def threshold(v, t, strict=False):
    """threshold_met(lasp_orset, v, t | {strict, t}) — lasp_lattice.erl:62-75."""
    return olattice.threshold_met(TYPE, v, ("strict", t) if strict else t)
