"""A reference model of lasp_core:update/4 on one variable, and the random scenario the
update/4 tests run (tests/test_update4_model.py on the model alone, tests/test_gpu_update4.py
against the device).

update/4 (lasp_core.erl:283-287) is `{ok, Value} = Type:update(Op, Actor, Value0)` and then
bind(Id, Value, Store), which writes Type:merge(Value0, Value) (:291-312).  lasp_orset:merge/2
ORs the removed flags of a token both sides hold (lasp_orset.erl:128-136) while add_elem stores
the token with `false` (:222-230): an {add_by_token, T, E} by a token Value0 holds removed
leaves it removed, and a variable's value never goes backwards.  update4 is that, over the
oracle; every replay of a device update in the suite goes through it.
"""

import random

from oracle import etf as oetf
from oracle import gset as ogset
from oracle import lattice as olat
from oracle import orset as oorset
from oracle import otp
from oracle.terms import Atom, exact_eq

A = Atom
OK, FALLBACK = 0, 1
UPD_OK, NOT_PRESENT = 0, 1
GSET_KINDS = ("gset", "lasp_gset")


def tb(t) -> bytes:
    return oetf.term_to_binary(t)


def update4(kind, op, cur, minted):
    """lasp_core:update/4 of `op` on a variable holding `cur`, with the tokens the device
    minted (in op order): ("ok", merge(cur, Value)) where Value is Type:update/3's, or
    update/3's {error, {precondition, ..}} as the oracle gives it — the value is then kept."""
    if kind in GSET_KINDS:
        res = ogset.update(op, A("a"), cur)
        return ("ok", ogset.merge(cur, res[1]))
    it = iter(minted)
    res = oorset.update(op, A("a"), cur, tokens=lambda _actor: next(it))
    if res[0] != "ok":
        return res
    return ("ok", oorset.merge(cur, res[1]))


def applied(kind, op, cur, minted):
    """The variable's value after the call: update4's on ok, `cur` kept on an error."""
    res = update4(kind, op, cur, minted)
    return res[1] if res[0] == "ok" else cur


def count_mints(op):
    if op[0] == "add":
        return 1
    if op[0] == "add_all":
        return len(op[1])
    if op[0] == "update":
        return sum(count_mints(o) for o in op[1])
    return 0


def flatten(op):
    """The call's atomic ops in order: ("add", E, T or None for a minted token) and
    ("remove", E)."""
    k = op[0]
    if k == "add":
        return [("add", op[1], None)]
    if k == "add_by_token":
        return [("add", op[2], op[1])]
    if k == "add_all":
        return [("add", e, None) for e in op[1]]
    if k == "remove":
        return [("remove", op[1])]
    if k == "remove_all":
        return [("remove", e) for e in op[1]]
    return [f for sub in op[1] for f in flatten(sub)]


def flag_of(cur, e, t):
    """The removed flag `cur` holds for token t of element e; None when it holds none."""
    found = otp.orddict_find(e, cur)
    if found is None:
        return None
    ft = otp.orddict_find(t, found[1])
    return None if ft is None else ft[1]


# ---- two wrong semantics, in place over the oracle's lists ------------------------------
def _in_place(op, cur, minted, add_flag):
    """The call's atomic ops applied in order to `cur`; add_flag(flag now held or None) is
    what an add stores.  None when a remove's element is absent (the call is void)."""
    it = iter(minted)
    s = cur
    for f in flatten(op):
        found = otp.orddict_find(f[1], s)
        if f[0] == "remove":
            if found is None:
                return None
            s = otp.orddict_store(f[1], [(t, True) for t, _r in found[1]], s)
            continue
        t = f[2] if f[2] is not None else next(it)
        toks = found[1] if found is not None else otp.orddict_new()
        held = otp.orddict_find(t, toks)
        s = otp.orddict_store(f[1], otp.orddict_store(
            t, add_flag(None if held is None else held[1]), toks), s)
    return s


def update3_only(op, cur, minted):
    """update/3 without the bind's merge: an add stores `false` whatever the variable held."""
    return _in_place(op, cur, minted, lambda _held: False)


def add_keeps_flag(op, cur, minted):
    """"An add never touches the removed flag", applied in place: a remove earlier in the
    same call has already set it."""
    return _in_place(op, cur, minted, lambda held: bool(held))


class Scenario:
    """~`steps` random update/4 calls on one OR-Set variable: every op form, a small element
    pool with three reusable tokens per element plus fresh ones, biased towards re-adds by a
    removed token and towards calls with a remove before an add_by_token of the same
    element.  dev: None (the model alone, tokens minted by the generator) or a
    lasp_amd.engine.NifVar, every answer of which is asserted byte for byte against update4.
    The counts say what the run covered."""

    ELEMS = [0, 1, 2, 7, 300, -2, A("e0"), A("e1"), b"bin", b"", (1, A("t")), (A("k"), 2)]
    NEVER = [A("zz"), 901, (2, A("t"))]

    def __init__(self, seed, dev=None):
        self.rng = random.Random(seed)
        self.dev = dev
        self.pool = {repr(e): [self.tok() for _ in range(3)] for e in self.ELEMS}
        self.value = []
        self.order = {}
        self.history = [[]]
        self.trace = []            # (op, minted, value before, value after) per step
        self.readds = 0            # add_by_token ops by a token the variable held removed
        self.remove_then_add = 0   # calls with a remove before an add_by_token of its element
        self.voided = 0
        self.reads = 0

    # ---- generators
    def tok(self):
        return bytes(self.rng.getrandbits(8) for _ in range(20))

    def held(self, e):
        """e's tokens in the variable, in the order they were first added (the same choice
        with the generator's tokens and with the device's)"""
        return self.order.get(repr(e), [])

    def token_for(self, e):
        """a token for an add_by_token of e: mostly one the variable holds removed"""
        rng = self.rng
        gone = [t for t in self.held(e) if flag_of(self.value, e, t)]
        r = rng.random()
        if gone and r < 0.5:
            return rng.choice(gone)
        if r < 0.8:
            return rng.choice(self.pool[repr(e)])
        return self.tok()

    def some_elem(self, absent=0.25):
        """an element for a remove: mostly one the variable holds, else any of the pool or
        one no call ever adds (the precondition fails)"""
        rng = self.rng
        present = [e for e, _t in self.value]
        if present and rng.random() >= absent:
            return rng.choice(present)
        return rng.choice(self.ELEMS + self.NEVER)

    def pair_call(self):
        """{update, Ops} with a remove and an add_by_token of one element"""
        rng = self.rng
        e = self.some_elem(0.0) if self.value else rng.choice(self.ELEMS)
        alive = [t for t in self.held(e) if not flag_of(self.value, e, t)]
        t = rng.choice(alive) if alive and rng.random() < 0.6 else self.token_for(e)
        add, rem = (A("add_by_token"), t, e), (A("remove"), e)
        form = rng.randrange(4)
        ops = [[rem, add], [add, rem], [add, rem, add], [rem, add, rem]][form]
        if rng.random() < 0.4:
            ops = ops[:1] + [self.rand_op(1)] + ops[1:]
        return (A("update"), ops)

    def rand_op(self, depth=0):
        rng = self.rng
        r = rng.random()
        if depth:
            r *= 0.8
        e = rng.choice(self.ELEMS)
        if r < 0.10:
            return (A("add"), e)
        if r < 0.40:
            if self.value and rng.random() < 0.7:
                e = rng.choice([e for e, _t in self.value])
            return (A("add_by_token"), self.token_for(e), e)
        if r < 0.47:
            return (A("add_all"), [rng.choice(self.ELEMS) for _ in range(rng.randint(0, 3))])
        if r < 0.70:
            return (A("remove"), self.some_elem())
        if r < 0.80:
            return (A("remove_all"), [self.some_elem() for _ in range(rng.randint(0, 2))])
        if r < 0.90:
            return self.pair_call()
        return (A("update"), [self.rand_op(depth + 1) for _ in range(rng.randint(0, 4))])

    # ---- one step
    def note(self, op):
        """what the call covers, against the value before it"""
        hit, removed = 0, []
        pair = False
        for f in flatten(op):
            if f[0] == "remove":
                removed.append(f[1])
            elif f[2] is not None:
                hit += flag_of(self.value, f[1], f[2]) is True
                pair |= any(exact_eq(f[1], e) for e in removed)
        self.readds += hit
        self.remove_then_add += pair
        return hit

    def check_value(self, where):
        self.reads += 1
        assert self.dev.read() == (OK, tb(self.value)), where
        assert self.dev.value() == (OK, tb(oorset.value(self.value))), where

    def step(self, step):
        rng, dev = self.rng, self.dev
        op = self.rand_op()
        hit = self.note(op)
        prev = self.value
        minted = [self.tok() for _ in range(count_mints(op))]
        if dev is not None:
            verd, res, err, minted = dev.update(tb(op))
            assert verd == OK, (step, op)
            assert len(minted) == count_mints(op) and all(len(t) == 20 for t in minted), (step, op)
        want = update4("orset", op, prev, minted)
        if want[0] == "ok":
            self.value = want[1]
            self.history.append(self.value)
            it = iter(minted)
            for f in flatten(op):
                if f[0] == "add":
                    t = f[2] if f[2] is not None else next(it)
                    if t not in self.held(f[1]):
                        self.order.setdefault(repr(f[1]), []).append(t)
        else:
            self.voided += 1
        self.trace.append((op, minted, prev, self.value))
        old = rng.choice(self.history)         # (drawn with and without a device: one run)
        if dev is None:
            return
        if want[0] == "ok":
            assert (res, err) == (UPD_OK, None), (step, op)
            # the value inflates: what it was stays met, and so does any earlier value
            assert dev.threshold(tb(prev)) == (OK, True), (step, op)
            assert olat.threshold_met("lasp_orset", self.value, old), (step, op)
            assert dev.threshold(tb(old)) == (OK, True), (step, op)
        else:
            assert res == NOT_PRESENT, (step, op)
            assert err == tb(want[1][1][1])[1:], (step, op)
        if hit or want[0] != "ok" or step % 5 == 0:
            self.check_value((step, op))

    def run(self, steps=300):
        for step in range(steps):
            self.step(step)
        if self.dev is not None:
            self.check_value("end")
        # (an element past 64 tokens would take the device's namespace wide: its own test)
        assert max(len(toks) for _e, toks in self.value) < 60
        return self


# the seed at which the model's run is not vacuous (tests/test_update4_model.py asserts it)
SEED = 5
