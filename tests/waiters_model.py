"""A reference model of the reference's blocking reads, and the random scenario the waiter
tests run (tests/test_waiters_abi.py on the model alone, tests/test_gpu_waiters.py against
the device).

read/6 (lasp_core.erl:331-364) appends {threshold, read, From, Type, Threshold} to the
variable's waiting_threads when threshold_met/3 (lasp_lattice.erl:62-75) fails; write/4
(:839-844) runs reply_to_all/3 (:765-825) over that list: every waiter now met is replied
to, in list order, and the rest stay in order.  ReplyModel is that, over oracle.lattice.
"""

import random

import update4_model as um
from oracle import etf as oetf
from oracle import gset as ogset
from oracle import lattice as olat
from oracle import orset as oorset
from oracle.terms import Atom, exact_eq

A = Atom
OK, FALLBACK = 0, 1
TYPES = {"orset": "lasp_orset", "gset": "lasp_gset"}


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


class ReplyModel:
    """waiting_threads of one variable: (id, strict, threshold) in list order."""

    def __init__(self, kind):
        self.type = TYPES[kind]
        self.value = []
        self.waiting = []

    def met(self, strict, th):
        return olat.threshold_met(self.type, self.value, ("strict", th) if strict else th)

    def wait(self, th, strict, wid):
        """read/6: met now -> True and nothing is kept, else appended at the tail."""
        if self.met(strict, th):
            return True
        self.waiting.append((wid, bool(strict), th))
        return False

    def write(self):
        """reply_to_all/3: the flags of the waiters met, in list order; they leave."""
        flags = [self.met(s, th) for _i, s, th in self.waiting]
        fired = [w[0] for w, f in zip(self.waiting, flags) if f]
        self.waiting = [w for w, f in zip(self.waiting, flags) if not f]
        return fired, flags

    def cancel(self, wid):
        for k, w in enumerate(self.waiting):
            if w[0] == wid:
                del self.waiting[k]
                return True
        return False

    def listing(self):
        return [(i, s, tb(th)) for i, s, th in self.waiting]


def oracle_update(kind, op, state, minted):
    """update/4 (tests/update4_model.py): Type:update/3, then the bind's merge with `state`."""
    return um.update4(kind, op, state, minted)


def merge(kind, a, b):
    return ogset.merge(a, b) if kind == "gset" else oorset.merge(a, b)


def count_mints(op):
    if op[0] == "add":
        return 1
    if op[0] == "add_all":
        return len(op[1])
    if op[0] == "update":
        return sum(count_mints(o) for o in op[1])
    return 0


class Scenario:
    """~`steps` random steps on one variable: update / a peer state made by the oracle /
    bind of one / wait / cancel, a re-check after every write.  dev: None (the model alone,
    tokens minted by the generator) or a lasp_amd.engine.NifVar, every answer of which is
    asserted against the model.  The counts say what the run covered."""

    ELEMS = list(range(14)) + [A("e0"), A("e1"), (1, A("t")), b"bin"]
    GSET_ELEMS = list(range(120)) + [A("e0"), A("e1"), (1, A("t")), b"bin"]
    FOREIGN = [A("zz0"), A("zz1"), 900, 901]

    def __init__(self, seed, kind, dev=None, passes=None):
        self.rng = random.Random(seed)
        self.kind, self.dev = kind, dev
        self.passes = passes       # () -> the context's device pass counter, or None
        if kind == "gset":
            self.ELEMS = self.GSET_ELEMS      # (adds only: a larger pool stays unsaturated)
        self.m = ReplyModel(kind)
        self.history = [[]]
        self.pending = []
        self.next_id = 1
        self.uid = 0
        self.live = {}             # uid per waiting entry, parallel to m.waiting
        self.uids = []
        self.survived = set()
        self.counts = {k: {False: 0, True: 0} for k in ("met_at_wait", "fired_later", "survived")}
        self.gap_writes = 0        # writes firing two waiters around one that stays
        self.rechecks = self.empty_rechecks = 0
        self.cancels = {True: 0, False: 0}

    # ---- generators
    def tok(self):
        return bytes(self.rng.getrandbits(8) for _ in range(20))

    def rand_op(self, depth=0):
        rng, cur = self.rng, self.m.value
        present = [e for e, _t in cur] if self.kind == "orset" else list(cur)
        e = rng.choice(self.ELEMS)
        if self.kind == "gset":
            if rng.random() < 0.6:
                return (A("add"), e)
            return (A("add_all"), [rng.choice(self.ELEMS) for _ in range(rng.randint(0, 3))])
        k = rng.randrange(8 if depth == 0 else 6)
        gone = rng.choice(present) if present and rng.random() < 0.85 else e
        if k in (0, 1):
            return (A("add"), e)
        if k == 2:
            return (A("add_all"), [rng.choice(self.ELEMS) for _ in range(rng.randint(0, 3))])
        if k in (3, 4):
            return (A("remove"), gone)
        if k == 5:
            return (A("remove_all"), [gone] if rng.random() < 0.7 else [gone, e])
        return (A("update"), [self.rand_op(depth + 1) for _ in range(rng.randint(0, 3))])

    def make_peer(self):
        """another replica's state: the current value after a few of its own updates"""
        s = self.m.value
        for _ in range(self.rng.randint(1, 3)):
            op = self.rand_op(1)
            r = oracle_update(self.kind, op, s, [self.tok() for _ in range(count_mints(op))])
            if r[0] == "ok":
                s = r[1]
        return s

    def sub_list(self, s):
        rng = self.rng
        if self.kind == "gset":
            return [e for e in s if rng.random() < 0.6]
        out = []
        for e, toks in s:
            if rng.random() < 0.6:
                keep = [t for t in toks if rng.random() < 0.7] or [toks[0]]
                out.append((e, keep))
        return out

    def threshold(self):
        rng = self.rng
        r = rng.random()
        if r < 0.55:
            if not self.pending:
                self.pending.append(self.make_peer())
            s = rng.choice(self.pending)
        elif r < 0.75:
            s = self.m.value
        else:
            s = rng.choice(self.history)
        r = rng.random()
        if r < 0.4:
            s = self.sub_list(s)
        elif r < 0.5:
            f = rng.choice(self.FOREIGN)
            extra = [f] if self.kind == "gset" else [(f, [(self.tok(), False)])]
            s = merge(self.kind, self.sub_list(s), extra)
        return s

    # ---- steps
    def recheck(self, step):
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
        if self.dev is not None:
            p0 = self.passes() if self.passes else 0
            got = self.dev.recheck(cap=2)
            assert got == (OK, fired, len(self.m.waiting)), (step, got, fired)
            if self.passes:
                # one device pass per laspj_var_recheck with waiters (a second call when
                # more than cap = 2 are met), none without
                want = 0 if not before else 2 if len(fired) > 2 else 1
                assert self.passes() - p0 == want, (step, len(before), fired)
            assert self.dev.waiters() == self.m.listing(), step

    def changed(self, value, step):
        self.m.value = value
        self.history.append(value)
        self.recheck(step)

    def step(self, step):
        rng, dev, kind = self.rng, self.dev, self.kind
        r = rng.random()
        if r < 0.28:
            op = self.rand_op()
            if dev is not None:
                verd, res, _err, minted = dev.update(tb(op))
                assert verd == OK, (step, op)
            else:
                minted = [self.tok() for _ in range(count_mints(op))]
            want = oracle_update(kind, op, self.m.value, minted)
            if dev is not None:
                assert res == (0 if want[0] == "ok" else 1), (step, op)
            if want[0] == "ok":
                self.changed(want[1], step)
        elif r < 0.40:
            self.pending.append(self.make_peer())
        elif r < 0.54:
            if self.pending and rng.random() < 0.85:
                peer = self.pending.pop(rng.randrange(len(self.pending)))
            else:
                peer = self.m.value                       # Value0 =:= Value: a no-op bind
            noop = exact_eq(peer, self.m.value)
            if dev is not None:
                assert dev.bind(tb(peer)) == (OK, 0 if noop else 1), step
            if not noop:
                self.changed(merge(kind, self.m.value, peer), step)
        elif r < 0.97:
            th, strict = self.threshold(), rng.random() < 0.5
            if self.m.waiting and rng.random() < 0.1:
                wid = rng.choice(self.m.waiting)[0]       # the same From waiting twice
            else:
                wid, self.next_id = self.next_id, self.next_id + 1
            met = self.m.wait(th, strict, wid)
            if met:
                self.counts["met_at_wait"][strict] += 1
            else:
                self.uid += 1
                self.uids.append(self.uid)
                self.live[self.uid] = strict
            if dev is not None:
                assert dev.wait(tb(th), strict, wid) == (OK, met), (step, strict, th)
                assert dev.waiters() == self.m.listing(), step
        else:
            wid = rng.choice(self.m.waiting)[0] if self.m.waiting and rng.random() < 0.7 else 10 ** 9
            k = next((k for k, w in enumerate(self.m.waiting) if w[0] == wid), None)
            found = self.m.cancel(wid)
            self.cancels[found] += 1
            if found:
                del self.live[self.uids.pop(k)]
            if dev is not None:
                assert dev.cancel(wid) is found, step
                assert dev.waiters() == self.m.listing(), step

    def run(self, steps=300):
        for step in range(steps):
            self.step(step)
        if self.dev is not None:
            assert self.dev.read() == (OK, tb(self.m.value))
        return self


# seeds at which the model's run is not vacuous (tests/test_waiters_abi.py asserts it)
SEEDS = {"orset": 8, "gset": 1}
