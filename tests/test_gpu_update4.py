"""lasp_core:update/4 on resident variables (laspj_var_etf_update; lasp_amd/csrc/
laspj_nif_vars.hip k_var_update / k_var_adds) as update-then-bind, against
tests/update4_model.py.

update/4 is Type:update/3 and then bind/3 of its Value, which writes merge(Value0, Value)
(lasp_core.erl:283-312).  lasp_orset:merge/2 ORs the removed flags (lasp_orset.erl:128-136), so
an {add_by_token, T, E} by a token the variable holds removed leaves T removed, while an
add_by_token after a remove of E in the same call gives T the flag Value0 had — neither
`false` always (update/3 alone) nor whatever an in-place remove left there.  Every answer is
compared byte for byte: read(), value(), the result code and the error element."""

import pytest

import update4_model as um
import waiters_model as wm
from oracle import orset as oorset
from oracle.terms import Atom

OK, FALLBACK = 0, 1
UPD_OK, NOT_PRESENT = um.UPD_OK, um.NOT_PRESENT
A = Atom
tb = um.tb

pytestmark = pytest.mark.gpu

E = A("e")
T, T1, T2 = b"\x11" * 20, b"\x01" * 20, b"\x02" * 20


def _ctx():
    from lasp_amd import engine
    return engine.Context(0)


def tok(k: int) -> bytes:
    """A 20-byte token (the length unique/1 mints); k orders them."""
    return k.to_bytes(4, "big") + bytes(16)


def call(var, cur, op, kind="orset"):
    """One update/4 on the device variable and on the model: the result code, the error
    element, read() and value() compared; the value after the call."""
    verd, res, err, minted = var.update(tb(op))
    assert verd == OK, op
    want = um.update4(kind, op, cur, minted)
    if want[0] == "ok":
        assert (res, err) == (UPD_OK, None), op
        cur = want[1]
    else:
        assert res == NOT_PRESENT and err == tb(want[1][1][1])[1:], op
    assert var.read() == (OK, tb(cur)), op
    assert var.value() == (OK, tb(cur if kind == "gset" else oorset.value(cur))), op
    return cur


def pads(n, base=0):
    """n adds of other elements, by token"""
    return [(A("add_by_token"), tok(500 + base + k), 1000 + base + k) for k in range(n)]


def padded(ops, n):
    """{update, Ops} of exactly n ops: `ops` in order, other elements' adds around them"""
    k = n - len(ops)
    assert k >= 0
    return (A("update"), pads(k // 2) + ops + pads(k - k // 2, 100))


def test_scenario_on_a_device_variable():
    """The model's 300-step scenario on a resident variable (tests/update4_model.py): the
    result code and the error element of every call, read() and value() after every call
    that re-adds a removed token or is voided (and every fifth), the value before each call
    and a random earlier value still met after it; nothing falls back."""
    ctx = _ctx()
    try:
        var = ctx.var("orset")
        sc = um.Scenario(um.SEED, dev=var).run(300)
        assert sc.readds >= 20 and sc.remove_then_add >= 10 and sc.voided >= 5
        assert sc.reads >= 60
        assert ctx.nif_stats()["fallbacks"] == 0
    finally:
        ctx.close()


def _start(var, state):
    """E's tokens brought to `state` ({token: removed}) by separate calls"""
    cur = []
    gone = [t for t, r in state.items() if r]
    for t in gone:
        cur = call(var, cur, (A("add_by_token"), t, E))
    if gone:
        cur = call(var, cur, (A("remove"), E))
    for t, r in state.items():
        if not r:
            cur = call(var, cur, (A("add_by_token"), t, E))
    assert cur == ([(E, sorted(state.items()))] if state else [])
    return cur


# (name, E's tokens before the call, the call's ops on E, E's tokens after it)
ADD_T, ADD_T1, REM = (A("add_by_token"), T, E), (A("add_by_token"), T1, E), (A("remove"), E)
KNOWN = [
    ("re-add by a removed token", {T: True}, [ADD_T], {T: True}),
    ("add by an alive token", {T: False}, [ADD_T], {T: False}),
    ("remove, then add by an alive token", {T1: False, T2: False}, [REM, ADD_T1],
     {T1: False, T2: True}),
    ("remove, then add by a removed token", {T1: True, T2: False}, [REM, ADD_T1],
     {T1: True, T2: True}),
    ("add by a new token, then remove", {T2: False}, [ADD_T, REM], {T: True, T2: True}),
    ("add by a removed token, then remove", {T: True}, [ADD_T, REM], {T: True}),
    ("a new token before and after a remove", {T2: False}, [ADD_T, REM, ADD_T],
     {T: False, T2: True}),
    ("an alive token before and after a remove", {T: False, T2: False}, [ADD_T, REM, ADD_T],
     {T: False, T2: True}),
    ("a removed token before and after a remove", {T: True, T2: False}, [ADD_T, REM, ADD_T],
     {T: True, T2: True}),
    ("remove, add, remove", {T: False}, [REM, ADD_T, REM], {T: True}),
]


@pytest.mark.parametrize("nops", [0, 24, 25])
def test_known_answers_in_the_three_kernel_forms(nops):
    """The known answers of tests/test_update4_model.py, each with the token alive and
    already removed, as a call of the bare ops, of 24 ops (kernel arguments) and of 25
    (uploaded ops: k_var_update when the call holds a remove, k_var_adds when it is all
    adds), padded with adds of other elements.  E's tokens after the call are the literal
    ones; the whole value is the model's."""
    ctx = _ctx()
    try:
        for name, before, ops, after in KNOWN:
            var = ctx.var("orset")
            cur = _start(var, before)
            op = padded(ops, nops) if nops else (A("update"), ops)
            cur = call(var, cur, op)
            assert [ts for e, ts in cur if e == E] == [sorted(after.items())], (name, nops)
            assert len(cur) == 1 + max(nops - len(ops), 0), (name, nops)
            var.close()
        assert ctx.nif_stats()["fallbacks"] == 0
    finally:
        ctx.close()


def test_thirty_adds_by_token_in_one_call():
    """One {update, [30 x add_by_token]} (k_var_adds, one op per lane): 15 of its tokens are
    held removed and stay removed, one of those is named twice, the others are alive or new;
    the tokens of an element share one {p, r} word pair, which the lanes update atomically."""
    ctx = _ctx()
    try:
        var = ctx.var("orset")
        t = lambda e, j: tok(10 * e + j)                 # noqa: E731
        cur = call(var, [], (A("update"), [(A("add_by_token"), t(e, j), e)
                                           for e in range(5) for j in range(6) if e != 2 or j < 3]))
        cur = call(var, cur, (A("remove_all"), [0, 1, 2]))
        cur = call(var, cur, (A("add_all"), [2, 2, 2]))
        removed = [(e, t(e, j)) for e in range(3) for j in range(6) if e != 2 or j < 3]
        assert len(removed) == 15 and all(um.flag_of(cur, e, k) is True for e, k in removed)
        alive = [(e, t(e, j)) for e in (3, 4) for j in range(4)]
        new = [(e, t(e, 7 + j)) for e in (0, 1, 3) for j in range(2)]
        ops = removed + alive[:7] + new + removed[4:5] + alive[7:]
        assert len(ops) == 30 and len(set(ops)) == 29
        mixed = [ops[(7 * k) % 30] for k in range(30)]   # removed, alive and new interleaved
        cur = call(var, cur, (A("update"), [(A("add_by_token"), k, e) for e, k in mixed]))
        assert all(um.flag_of(cur, e, k) is True for e, k in removed)
        assert all(um.flag_of(cur, e, k) is False for e, k in alive + new)
        assert oorset.value(cur) == [0, 1, 2, 3, 4]
        assert ctx.nif_stats()["fallbacks"] == 0
    finally:
        ctx.close()


def test_wide_namespace_slots_on_both_sides_of_the_pair_boundary():
    """An element of 70 tokens (the 65th widens the namespace: two {p, r} pairs per cell;
    token slots follow registration order, laspj_host.cpp reg_tok): removed, then re-added by
    the tokens in slots 0, 63, 64 and 69 — the last of pair 0, the first of pair 1 (slot bits
    8.. travel in the op's pad byte) — every one stays removed.  On a replica holding them
    alive, a remove and an add_by_token in one call leaves exactly that token alive; the
    same in a call of 25 ops (uploaded)."""
    ctx = _ctx()
    try:
        var = ctx.var("orset")
        w = [tok(7000 - 13 * k) for k in range(70)]          # registered out of term order
        cur = call(var, [], (A("add_by_token"), tok(1), A("other")))
        for k in range(0, 70, 7):
            cur = call(var, cur, (A("update"), [(A("add_by_token"), t, E) for t in w[k:k + 7]]))
        assert ctx.nif_stats()["namespaces_widened"] == 1
        rep = var.replica()
        assert rep.bind(tb(cur)) == (OK, 1)
        alive = cur
        cur = call(var, cur, (A("remove"), E))
        picks = [w[0], w[63], w[64], w[69]]
        for t in picks:
            cur = call(var, cur, (A("add_by_token"), t, E))
            assert all(r for _t, r in dict(cur)[E])
        assert oorset.value(cur) == [A("other")]
        for t in picks:
            cur = call(var, cur, (A("update"), [(A("remove"), E), (A("add_by_token"), t, E)]))
            assert all(r for _t, r in dict(cur)[E])
        # the replica: every token alive before each call
        for n, t in zip((2, 2, 25, 25), picks):
            assert rep.write(tb(alive)) == OK
            got = call(rep, alive, padded([(A("remove"), E), (A("add_by_token"), t, E)], n))
            assert [k for k, r in dict(got)[E] if not r] == [t], n
        # consecutive calls: the first leaves its token alive, and that one is removed by
        # the second call, whose own token the first call removed
        assert rep.write(tb(alive)) == OK
        got = alive
        for t in picks:
            got = call(rep, got, (A("update"), [(A("remove"), E), (A("add_by_token"), t, E)]))
            assert [k for k, r in dict(got)[E] if not r] == ([t] if t == picks[0] else [])
        assert ctx.nif_stats()["fallbacks"] == 0
    finally:
        ctx.close()


def test_waiters_stay_met_after_a_readd():
    """A strict read of the value as it is blocks (nothing has changed); the remove fires it.
    After the re-add by the same token the value has not moved: the threshold is still met
    and value/1 does not list the element.  (A read of the value as it will be after the
    remove is met at once: is_inflation takes no notice of the flags,
    lasp_lattice.erl:153-161 — the model decides.)"""
    ctx = _ctx()
    try:
        var = ctx.var("orset")
        m = wm.ReplyModel("orset")
        cur = call(var, [], (A("add_by_token"), T, E))
        cur = call(var, cur, (A("add_by_token"), T2, A("f")))
        m.value = cur
        after = um.update4("orset", (A("remove"), E), cur, [])[1]
        assert after == [(E, [(T, True)]), (A("f"), [(T2, False)])]
        met = m.wait(after, False, 1)
        assert var.wait(tb(after), False, 1) == (OK, met)
        assert not m.wait(cur, True, 2)
        assert var.wait(tb(cur), True, 2) == (OK, False)
        assert var.recheck() == (OK, [], 1)
        cur = call(var, cur, (A("remove"), E))
        assert cur == after
        m.value = cur
        fired, _flags = m.write()
        assert fired == [2]
        assert var.recheck() == (OK, [2], 0)
        before = cur
        cur = call(var, cur, (A("add_by_token"), T, E))
        assert cur == after
        assert var.threshold(tb(after)) == (OK, True)
        assert var.threshold(tb(before), True) == (OK, False)       # nothing new since
        assert var.threshold(tb([(E, [(T, False)])]), True) == (OK, True)
        assert var.value() == (OK, tb([A("f")]))
    finally:
        ctx.close()


def test_replicas_agree_after_a_readd():
    """A re-add by a removed token on one replica, then each replica's image bound into the
    other: both binds are no-ops, both read the oracle's value, and the first replica's image
    is the same before and after the exchange."""
    ctx = _ctx()
    try:
        a = ctx.var("orset")
        b = a.replica()
        cur = call(a, [], (A("add_by_token"), T, E))
        cur = call(a, cur, (A("add_by_token"), T2, E))
        cur = call(a, cur, (A("remove"), E))
        cur = call(a, cur, (A("add_by_token"), T1, A("f")))
        assert b.bind(tb(cur)) == (OK, 1)
        cur = call(a, cur, (A("add_by_token"), T, E))
        img = a.read()
        assert img == (OK, tb([(E, [(T2, True), (T, True)]), (A("f"), [(T1, False)])]))
        assert b.bind(img[1]) == (OK, 0)
        assert a.bind(b.read()[1]) == (OK, 0)
        assert a.read() == img and b.read() == img
        assert a.value() == b.value() == (OK, tb([A("f")]))
    finally:
        ctx.close()


def test_gset_updates_through_the_model():
    """A G-Set's merge is the union, so update/4 is update/3: adds and add_alls of 0, 24, 25
    and 40 elements (kernel arguments, uploaded ops) through the same model."""
    ctx = _ctx()
    try:
        g = ctx.var("gset")
        cur = []
        for k, n in enumerate((1, 0, 24, 25, 40, 3)):
            cur = call(g, cur, (A("add"), A(f"g{k}")), "gset")
            cur = call(g, cur, (A("add_all"), [(7 * k + 3 * j) % 90 for j in range(n)]), "gset")
        assert len(cur) > 40
        assert ctx.nif_stats()["fallbacks"] == 0
    finally:
        ctx.close()
