"""A reference model of blocking reads on a list-valued variable, and the random scenario the
list waiter tests run (tests/test_lvar_waiters_model.py on the model alone,
tests/test_gpu_lvar_waiters.py against the device).

read/6 (lasp_core.erl:331-364) on a list value blocks in waiting_threads until write/4
(:839-844) runs reply_to_all/3 (:765-825); threshold_met(lasp_orset, Value, T) is
is_inflation(T, Value), is_strict_inflation for {strict, T} (lasp_lattice.erl:72-75), on
lists that need not be orddicts (:153-161, 235-253).  ListReplyModel is tests/waiters_model's
ReplyModel over tests/lvars_model.threshold.
"""

import lvars_model as lm
import update4_model as um
import waiters_model as wm
from oracle.terms import Atom

A = Atom
OK, FALLBACK = wm.OK, wm.FALLBACK
NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
tb = wm.tb


class ListReplyModel(wm.ReplyModel):
    """waiting_threads of one list-valued lasp_orset variable."""

    def __init__(self):
        super().__init__("orset")

    def met(self, strict, th):
        return lm.threshold(self.value, th, strict)


# ---- the literals the model is pinned on: (value, threshold, strict, met) -----------------
T0, T1, TA, TB_, TC = b"t0", b"t1", b"a", b"b", b"c"
FIRST_MATCH_VALUE = [(5, [(TA, False)]), (3, [(TB_, False)]), (5, [(TA, False), (TC, False)])]
RUN_VALUE = [(1, [(T0, False), (T1, False)])]
TWO_VALUE = [(1, [(T0, False)]), (2, [(T1, False)])]
LITERALS = [
    # lists:keyfind takes the first entry with an equal key
    ("first match: a token only the later entry holds", FIRST_MATCH_VALUE,
     [(5, [(TC, False)])], False, False),
    ("first match: the first entry's token", FIRST_MATCH_VALUE, [(5, [(TA, False)])], False, True),
    # Ids =/= Ids1 is order- and flag-sensitive, ids_inflated is neither
    ("tokens in another order, strict", RUN_VALUE, [(1, [(T1, False), (T0, False)])], True, True),
    ("equal to the value, strict", RUN_VALUE, RUN_VALUE, True, False),
    ("equal to the value", RUN_VALUE, RUN_VALUE, False, True),
    ("a flag false against true", RUN_VALUE, [(1, [(T0, False), (T1, True)])], False, True),
    ("a flag false against true, strict", RUN_VALUE, [(1, [(T0, False), (T1, True)])], True,
     True),
    ("a flag true against false", [(1, [(T0, True), (T1, False)])], RUN_VALUE, False, True),
    ("a flag true against false, strict", [(1, [(T0, True), (T1, False)])], RUN_VALUE, True,
     True),
    # ([], Current)
    ("strict [] on []", [], [], True, False),
    ("strict [] on a value", RUN_VALUE, [], True, True),
    ("[] on []", [], [], False, True),
    ("[] on a value", RUN_VALUE, [], False, True),
    # NewElements: length(Previous) < length(Current)
    ("the first entry of two, strict", TWO_VALUE, TWO_VALUE[:1], True, True),
    ("a repeated key, longer than the value", TWO_VALUE, TWO_VALUE[:1] * 3, False, True),
    ("a repeated key, longer than the value, strict", TWO_VALUE, TWO_VALUE[:1] * 3, True,
     False),
]


class ListScenario(wm.Scenario):
    """~`steps` random steps on l, r and the list variable out that intersection/7 re-runs
    into: add_by_token / remove on l or r, the re-run (alone, or fused with the re-check), a
    foreign bind of a list whose keys descend or repeat, a write, wait, cancel; a re-check
    after every write and every WRITTEN.  dev: None (the model alone) or an object with l, r
    (engine.NifVar of one namespace) and out (engine.NifListVar), every answer of which is
    asserted against the model.  Tokens are the generator's (add_by_token), so the run is the
    same with and without a device."""

    ELEMS = list(range(9)) + [A("e0"), A("e1"), (1, A("t")), b"bin"]
    FOREIGN = [A("zz0"), A("zz1"), 900, 901]

    def __init__(self, seed, dev=None, passes=None):
        super().__init__(seed, "orset", None, passes)
        self.m = ListReplyModel()
        self.devs = dev
        self.dev = dev.out if dev is not None else None
        self.lval, self.rval = [], []
        self.toks = {}                 # per key, the tokens the namespace has seen
        self.status = {NOOP: 0, WRITTEN: 0, REFUSED: 0}
        self.fused = 0

    # ---- generators
    def tok_for(self, e, fresh=0.5):
        seen = self.toks.setdefault(repr(e), [])
        if seen and self.rng.random() >= fresh:
            return self.rng.choice(seen)
        t = self.tok()
        seen.append(t)
        return t

    def descending(self):
        """a foreign state: a few keys, descending or shuffled, one perhaps repeated"""
        rng = self.rng
        keys = rng.sample(self.ELEMS, rng.randint(1, 4))
        if rng.random() < 0.4:
            keys.append(keys[0])
        return [(k, [(self.tok_for(k), rng.random() < 0.3) for _ in range(rng.randint(1, 3))])
                for k in keys]

    def mutate(self, s):
        rng = self.rng
        r = rng.random()
        s = [(k, list(toks)) for k, toks in s]
        if r < 0.30:
            return self.sub_list(s)
        if r < 0.40 and s:
            k = rng.randrange(len(s))
            s[k] = (s[k][0], s[k][1][::-1])                         # the run in another order
            return s
        if r < 0.50 and s:
            k = rng.randrange(len(s))
            j = rng.randrange(len(s[k][1]))
            t, f = s[k][1][j]
            s[k][1][j] = (t, not f)                                 # a flag flipped
            return s
        if r < 0.58:
            f = rng.choice(self.FOREIGN)
            return self.sub_list(s) + [(f, [(self.tok_for(f), False)])]
        if r < 0.64 and s:
            return s + [rng.choice(s)]                              # a key repeated
        if r < 0.70:
            return []
        return s

    def threshold(self):
        rng = self.rng
        r = rng.random()
        if r < 0.50:
            # where the next re-run may take the value
            s = lm.bind(self.m.value, lm.acc_value(self.lval, self.rval))[1]
            if rng.random() < 0.5:
                e = rng.choice(self.ELEMS)
                s = lm.bind(s, [(e, [(self.tok_for(e), False)])])[1]
        elif r < 0.80:
            s = self.m.value
        else:
            s = rng.choice(self.history)
        return self.mutate(s)

    # ---- steps
    def recheck(self, step, got=None):
        """reply_to_all on the model; the device's answer is `got` (the fused call's fired
        ids and count left) or asked with laspj_lvar_recheck here."""
        before = list(self.uids)
        fired, flags = self.m.write()
        self.rechecks += 1
        if not before:
            self.empty_rechecks += 1
        idx = [k for k, f in enumerate(flags) if f]
        if len(idx) >= 2 and idx[-1] - idx[0] + 1 > len(idx):
            self.gap_writes += 1
        for k, u in enumerate(before):
            strict = self.live[u]
            if flags[k]:
                self.counts["fired_later"][strict] += 1
                del self.live[u]
            elif u not in self.survived:
                self.survived.add(u)
                self.counts["survived"][strict] += 1
        self.uids = [u for k, u in enumerate(before) if not flags[k]]
        if self.dev is None:
            return fired
        if got is not None:
            assert got == (fired, len(self.m.waiting)), (step, got, fired)
        else:
            p0 = self.passes() if self.passes else 0
            ans = self.dev.recheck(cap=2)
            assert ans == (OK, fired, len(self.m.waiting)), (step, ans, fired)
            if self.passes:
                # one device pass per laspj_lvar_recheck with waiters (a second call when
                # more than cap = 2 are met), none without
                want = 0 if not before else 2 if len(fired) > 2 else 1
                assert self.passes() - p0 == want, (step, len(before), fired)
        assert self.dev.waiters() == self.m.listing(), step
        return fired

    def update(self, step):
        rng = self.rng
        left = rng.random() < 0.5
        cur = self.lval if left else self.rval
        present = [e for e, _t in cur]
        if present and rng.random() < 0.25:
            op = (A("remove"), rng.choice(present))
        else:
            e = rng.choice(self.ELEMS)
            op = (A("add_by_token"), self.tok_for(e, 0.8), e)
        want = um.update4("orset", op, cur, [])
        if self.devs is not None:
            var = self.devs.l if left else self.devs.r
            verd, res, _err, _minted = var.update(tb(op))
            assert verd == OK and res == (0 if want[0] == "ok" else 1), (step, op)
        if want[0] == "ok":
            if left:
                self.lval = want[1]
            else:
                self.rval = want[1]

    def rerun(self, step):
        st, new = lm.intersection(self.lval, self.rval, self.m.value)
        self.status[st] += 1
        d = self.devs
        fused = self.rng.random() < 0.5
        if d is None:
            if st == WRITTEN:
                self.changed(new, step)
            return
        if not fused:
            assert d.out.intersection(d.l, d.r) == (OK, st), step
            if st == WRITTEN:
                self.changed(new, step)
            return
        self.fused += 1
        nwait = len(self.m.waiting)
        p0 = self.passes() if self.passes else 0
        verd, got_st, ids, left = d.out.intersection_recheck(d.l, d.r, cap=2)
        assert (verd, got_st) == (OK, st), (step, verd, got_st, st)
        dp = (self.passes() - p0) if self.passes else None
        if st != WRITTEN:
            assert (ids, left) == ([], nwait), step
            assert dp is None or dp <= 1, (step, dp)
            return
        self.m.value = new
        self.history.append(new)
        fired = self.recheck(step, got=(ids, left))
        # the re-check rode inside the bind's pass (more than cap = 2 met: asked again)
        assert dp is None or dp == (2 if len(fired) > 2 else 1), (step, dp, fired)

    def step(self, step):
        rng, d = self.rng, self.devs
        r = rng.random()
        if r < 0.30:
            self.update(step)
        elif r < 0.52:
            self.rerun(step)
        elif r < 0.56:
            v = self.descending()
            st, new = lm.bind(self.m.value, v)
            self.status[st] += 1
            if d is not None:
                assert d.out.bind(tb(v)) == (OK, st), (step, v)
            if st == WRITTEN:
                self.changed(new, step)
        elif r < 0.62:
            # write/4: the body's own output (an orddict again), or any list
            k = rng.random()
            v = lm.acc_value(self.lval, self.rval) if k < 0.6 else \
                self.mutate(self.m.value) if k < 0.9 else self.descending()
            if d is not None:
                assert d.out.write(tb(v)) == OK, (step, v)
            self.changed(v, step)                                   # write/4 always replies
        elif r < 0.96:
            th, strict = self.threshold(), rng.random() < 0.5
            if self.m.waiting and rng.random() < 0.1:
                wid = rng.choice(self.m.waiting)[0]                 # the same From waiting twice
            else:
                wid, self.next_id = self.next_id, self.next_id + 1
            met = self.m.wait(th, strict, wid)
            if met:
                self.counts["met_at_wait"][strict] += 1
            else:
                self.uid += 1
                self.uids.append(self.uid)
                self.live[self.uid] = strict
            if d is not None:
                assert d.out.wait(tb(th), strict, wid) == (OK, met), (step, strict, th)
                assert d.out.waiters() == self.m.listing(), step
        else:
            wid = rng.choice(self.m.waiting)[0] if self.m.waiting and rng.random() < 0.7 else 10 ** 9
            k = next((k for k, w in enumerate(self.m.waiting) if w[0] == wid), None)
            found = self.m.cancel(wid)
            self.cancels[found] += 1
            if found:
                del self.live[self.uids.pop(k)]
            if d is not None:
                assert d.out.cancel(wid) is found, step
                assert d.out.waiters() == self.m.listing(), step
        if d is not None:
            assert d.out.read() == (OK, tb(self.m.value)), step

    def run(self, steps=260):
        for step in range(steps):
            self.step(step)
        # (an element past 64 tokens would take the device's namespace wide)
        assert max(len(v) for v in self.toks.values()) < 60
        return self


# the seed at which the model's run is not vacuous (tests/test_lvar_waiters_model.py asserts it)
SEED = 32
