"""tests/update4_model.py pinned on the CPU: update4 is lasp_core:update/4 (update/3, then
bind/3's merge with the value the variable held, lasp_core.erl:283-312) as oracle.core.Store
runs it, every step of its scenario inflates, three known answers, and the scenario tells
update/4 apart from the two in-place semantics a device kernel could have instead."""

import update4_model as um
from oracle import core as ocore
from oracle import lattice as olat
from oracle.terms import Atom, exact_eq

A = Atom
T, T1, T2 = b"\x11" * 20, b"\x01" * 20, b"\x02" * 20
E = A("e")


def _scenario():
    return um.Scenario(um.SEED).run(300)


def test_update4_agrees_with_the_oracle_store():
    """Step for step over the scenario: Store.update (update/3, then bind/3) with the same
    minted tokens leaves the value update4 gives; a voided call is Store's badmatch."""
    sc = _scenario()
    store = ocore.Store()
    _ok, vid = store.declare("lasp_orset")
    for k, (op, minted, prev, new) in enumerate(sc.trace):
        it = iter(minted)
        store.tokens = lambda _actor: next(it)       # noqa: B023
        want = um.update4("orset", op, prev, minted)
        try:
            store.update(vid, op, A("a"))
            assert want[0] == "ok", (k, op)
        except RuntimeError:
            assert want[0] == "error", (k, op)
        assert exact_eq(store.value(vid), new), (k, op)
        assert exact_eq(um.applied("orset", op, prev, minted), new), (k, op)


def test_every_step_is_an_inflation():
    """The value never goes backwards: is_inflation of every step, and no token's removed
    flag goes from true to false."""
    for k, (op, _minted, prev, new) in enumerate(_scenario().trace):
        assert olat.is_inflation("lasp_orset", prev, new), (k, op)
        for e, toks in prev:
            for t, removed in toks:
                assert um.flag_of(new, e, t) is not None, (k, op)
                assert um.flag_of(new, e, t) or not removed, (k, op)


def test_three_known_answers():
    """Fixed 20-byte tokens: a re-add by a removed token leaves it removed; a remove before
    an add_by_token of an alive token gives it back `false` and removes the others; an
    add_by_token before the remove is removed."""
    cur = um.applied("orset", (A("add_by_token"), T, E), [], [])
    cur = um.applied("orset", (A("remove"), E), cur, [])
    assert cur == [(E, [(T, True)])]
    assert um.update4("orset", (A("add_by_token"), T, E), cur, []) == ("ok", [(E, [(T, True)])])
    alive = [(E, [(T1, False), (T2, False)])]
    op = (A("update"), [(A("remove"), E), (A("add_by_token"), T1, E)])
    assert um.update4("orset", op, alive, []) == ("ok", [(E, [(T1, False), (T2, True)])])
    op = (A("update"), [(A("add_by_token"), T, E), (A("remove"), E)])
    assert um.update4("orset", op, [], []) == ("ok", [(E, [(T, True)])])
    assert um.update4("orset", op, [(E, [(T, False)])], []) == ("ok", [(E, [(T, True)])])
    # the two wrong semantics on the same calls
    assert um.update3_only((A("add_by_token"), T, E), cur, []) == [(E, [(T, False)])]
    op = (A("update"), [(A("remove"), E), (A("add_by_token"), T1, E)])
    assert um.add_keeps_flag(op, alive, []) == [(E, [(T1, True), (T2, True)])]
    # a G-Set's merge is the union: update4 is update/3
    assert um.update4("gset", (A("add_all"), [3, 1]), [2], []) == ("ok", [1, 2, 3])
    assert um.update4("lasp_gset", (A("add"), 2), [2], []) == ("ok", [2])


def test_scenario_discriminates_and_covers():
    """update/3 alone (an add stores `false`) and "an add never touches the flag" (in place,
    after a remove in the same call has set it) each part from update4 inside the scenario,
    which holds at least 20 re-adds of a removed token, 10 calls with a remove before an
    add_by_token of the same element and 5 voided calls."""
    sc = _scenario()
    diverged = {"update3_only": 0, "add_keeps_flag": 0}
    for op, minted, prev, new in sc.trace:
        want = um.update4("orset", op, prev, minted)
        for name in diverged:
            got = getattr(um, name)(op, prev, minted)
            assert (got is None) == (want[0] != "ok"), op       # the precondition is shared
            if got is not None and not exact_eq(got, new):
                diverged[name] += 1
    assert diverged["update3_only"] > 0 and diverged["add_keeps_flag"] > 0, diverged
    assert sc.readds >= 20, sc.readds
    assert sc.remove_then_add >= 10, sc.remove_then_add
    assert sc.voided >= 5, sc.voided
    # every op form was generated
    forms = {str(f[0]) for op, *_ in sc.trace for f in _forms(op)}
    assert forms == {"add", "add_by_token", "add_all", "remove", "remove_all", "update"}
    assert len(sc.value) >= 8


def _forms(op):
    yield op
    if op[0] == "update":
        for sub in op[1]:
            yield from _forms(sub)
