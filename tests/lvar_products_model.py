"""A pure-Python model of the resident product/7 (include/laspj.h "pair-keyed list
variables", laspj_lvar_product), clause by clause over the oracle.

product/7's OR-Set branch (lasp_core.erl:499-533) builds AccValue = [{{X, Y},
orset_causal_product(Cx, Cy)} || {X, Cx} <- L, {Y, Cy} <- R] (lasp_lattice.erl:303-308: both
foldls reversed, so a run comes out descending for sorted inputs) and binds it with bind/3
(:291-312) into a variable whose keys are 2-tuples and whose tokens are 2-lists: the pair-keyed
list variable, bound as tests/lvars_model.bind binds.
"""

import lvars_model as lm
from oracle import core as ocore

NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
TYPE = lm.TYPE

# the pair-keyed refused bind (tests/lvars_model.REFUSED_VALUE0 with pair keys and 2-list
# tokens): VALUE0's keys descend, orddict:merge walks them as if they ascended, and
# is_inflation's keyfind meets key {1, 0} first with VALUE's token only
REFUSED_VALUE0 = [((2, 0), [([b"a", b"x"], False)]), ((1, 0), [([b"b", b"x"], False)])]
REFUSED_VALUE = [((1, 0), [([b"c", b"x"], False)])]

bind = lm.bind
value = lm.value
counts = lm.counts
threshold = lm.threshold


def acc_value(l, r):
    """product/7's AccValue over two OR-Set values."""
    return ocore.product_body(TYPE, l, r)


def product(l, r, out):
    """laspj_lvar_product: (status, new out)."""
    return lm.bind(out, acc_value(l, r))


def closed_form(l, r):
    """AccValue for orddicts l and r as the producer lays it out (include/laspj.h
    laspj_lvar_product): entry i nr + j keyed {x_i, y_j}; token u b_j + v of it is
    [Cx_i[a_i - 1 - u], Cy_j[b_j - 1 - v]] with the two flags ORed."""
    out = []
    for x, cx in l:
        for y, cy in r:
            toks = []
            for tx, dx in reversed(cx):
                for ty, dy in reversed(cy):
                    toks.append(([tx, ty], dx or dy))
            out.append(((x, y), toks))
    return out
