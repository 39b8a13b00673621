"""A pure-Python model of the resident fold process (include/laspj.h "resident fold
processes"), over the oracle: tests/maps_model.MapModel with list results.

The device keeps, per fold, F's result list for every element it has been asked about; a
re-run reports the held elements it has no result for (`pending`) and leaves the output alone,
or — none pending — binds fold/6's AccValue (oracle.core.fold_body with the recorded results,
lasp_core.erl:460-486) into the list-valued output the way tests/lvars_model.bind does
(bind/3, lasp_core.erl:291-312).

A fold is refused (its results rolled back, FALLBACK from then on) when some V of a result
is `==` to a registered term under another image, is a term kind the dictionary does not
hold, or would put more than 64 tokens under one output key.
"""

import lvars_model as lm
import maps_model as mm
from oracle import core as ocore

NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
TOK_CAP = mm.TOK_CAP
tb = mm.tb


class FoldModel(mm.MapModel):
    """MapModel whose fun answers a list: `results` holds lists, every V of one is registered
    and takes its X's tokens."""

    def _refusal(self, pend, res):
        terms, classes = dict(self.terms), dict(self.classes)
        tokens = {k: set(v) for k, v in self.tokens.items()}
        for ys in res:
            if not isinstance(ys, list):
                raise TypeError("bad generator: a list comprehension over a non-list")
            for y in ys:
                if not mm.holdable(y):
                    return True, None
                yi = tb(y)
                if yi not in terms:
                    if classes.setdefault(mm.eq_class(y), yi) != yi:
                        return True, None
                    terms[yi] = y
                    tokens.setdefault(yi, set())
        # the tokens each X had registered when F was asked, now also under every V of F(X);
        # those the fold itself put under X stand for another input's and are not passed on
        mine = {k: set(v) for k, v in self.mine.items()}
        for x, ys in zip(pend, res):
            xi = tb(x)
            own = set(self.tokens.get(xi, ())) - mine.get(xi, set())
            for y in ys:
                yi = tb(y)
                mine.setdefault(yi, set()).update(own - tokens[yi])
                tokens[yi] |= own
                if len(tokens[yi]) > TOK_CAP:
                    return True, None
        return False, (terms, classes, tokens, mine)

    def acc(self, value):
        """fold/6's AccValue with the recorded results (nothing may be pending)."""
        return ocore.fold_body(lm.TYPE, lambda x: self.results[tb(x)], value)
