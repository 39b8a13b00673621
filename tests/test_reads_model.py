"""tests/reads_model.py pinned to the text of lasp_core.erl:331-420, 730-758, 795-813 and
839-844: each test is one quirk the device entry points (laspj_var_read / _read_any /
_wait_needed) reproduce and tests/test_gpu_reads.py checks against this model."""

import pytest

import reads_model as rm
from reads_model import Dv, ReferenceRaises


def tok(k, s=0):
    return bytes([s, k]) + b"\x11" * 18


def st(ks, s=0):
    return [(k, [(tok(k, s), False)]) for k in ks]


def _with_lazy():
    """value {0, 1}; lazy thresholds: 10 wants {0,1,2}, 11 wants {0,1,5}, 12 wants {0,1,2,3}"""
    dv = Dv("orset")
    dv.value = st([0, 1])
    assert dv.wait_needed(st([0, 1, 2]), False, 10) is False
    assert dv.wait_needed(st([0, 1, 5]), False, 11) is False
    assert dv.wait_needed(st([0, 1, 2, 3]), False, 12) is False
    assert [i for i, _ in dv.lazy] == [10, 11, 12]
    return dv


def test_met_read_leaves_fired_lazy_entries_in_place():
    """:353-354 reply to the lazy threads and do not store StillLazy"""
    dv = _with_lazy()
    before = list(dv.lazy)
    assert dv.read(st([0]), False, 1) == (True, [10, 11, 12])
    assert dv.lazy == before and dv.waiting == []
    assert dv.read(st([0]), False, 2) == (True, [10, 11, 12])      # they fire again


def test_blocking_read_removes_fired_lazy_entries():
    """:362 stores StillLazy beside the new waiter; a lazy entry fires when the read's
    threshold -> its own is an inflation (:798)"""
    dv = _with_lazy()
    assert dv.read(st([0, 1, 2]), False, 1) == (False, [10, 12])
    assert [i for i, _ in dv.lazy] == [11]
    assert dv.waiting == [(1, False, st([0, 1, 2]))]
    # strict: 10's threshold equals the read's — no strict inflation
    dv = _with_lazy()
    assert dv.read(st([0, 1, 2]), True, 1) == (False, [12])
    assert [i for i, _ in dv.lazy] == [10, 11]


def test_wait_needed_answers_at_once_when_somebody_reads():
    """:739-741: a non-empty waiting_threads; :735-737: the threshold is met"""
    dv = Dv("gset")
    dv.value = [1, 2]
    assert dv.wait_needed([1], False, 5) is True and dv.lazy == []
    assert dv.wait_needed([1, 2], True, 5) is False          # strict: not met, registers
    dv = Dv("gset")
    dv.value = [1, 2]
    assert dv.read([1, 2, 3], False, 1) == (False, [])
    assert dv.wait_needed([1, 2, 9], False, 5) is True and dv.lazy == []


def test_write_empties_lazy_threads():
    """:842-843: V1 = #dv{type, value, waiting_threads} — lazy_threads is the default"""
    dv = _with_lazy()
    dv.waiting = [(1, False, st([0, 1, 2])), (2, True, st([0, 1]))]
    assert dv.write(st([0, 1, 2])) == [1, 2]
    assert dv.lazy == [] and dv.waiting == []


def test_read_any_registers_waiters_ahead_of_the_first_met_read():
    a, b, c = Dv("orset"), Dv("gset"), Dv("orset")
    a.value, b.value, c.value = st([0]), [1, 2], st([7])
    reads = [(a, st([0, 1]), False), (b, [1], False), (c, st([8]), False)]
    assert rm.read_any(reads, 9) == (1, [[], [], []])
    assert a.waiting == [(9, False, st([0, 1]))] and b.waiting == [] and c.waiting == []
    # none met: every read leaves its waiter
    reads = [(a, st([0, 1]), True), (b, [3], False), (c, st([8]), False)]
    assert rm.read_any(reads, 10) == (-1, [[], [], []])
    assert [len(x.waiting) for x in (a, b, c)] == [2, 1, 1]


def test_read_any_names_one_variable_twice():
    """the second read of the variable sees the waiter (wait_needed would answer at once)
    and the lazy removals of the first; a met read stores nothing"""
    dv = _with_lazy()
    reads = [(dv, st([0, 1, 2]), False), (dv, st([0, 1, 2, 3]), False), (dv, st([0]), False)]
    assert rm.read_any(reads, 4) == (2, [[10, 12], [], [11]])
    assert [i for i, _ in dv.lazy] == [11]
    assert [w[0] for w in dv.waiting] == [4, 4]
    # met first: the lazy list is walked once and kept, nothing after it runs
    dv = _with_lazy()
    assert rm.read_any([(dv, st([0]), False), (dv, st([0, 1, 2]), False)], 4) == \
        (0, [[10, 11, 12], []])
    assert len(dv.lazy) == 3 and dv.waiting == []


@pytest.mark.parametrize("kind", ["orset", "gset"])
def test_strict_lazy_threshold_raises_at_the_next_nonempty_read(kind):
    """wait_needed/6 stores {strict, T} (:747-753); reply_to_all hands it to is_inflation
    as a value (:798): lists:keyfind/3 / sets:from_list/1 of a tuple"""
    dv = Dv(kind)
    cur = st([0, 1]) if kind == "orset" else [0, 1]
    dv.value = cur
    assert dv.wait_needed(cur, True, 3) is False
    assert dv.lazy == [(3, ("strict", cur))]
    with pytest.raises(ReferenceRaises):
        dv.read(cur, False, 1)
    if kind == "orset":
        # lists:foldl over [] never looks at the tuple (:153-161, 235-236)
        assert dv.read([], False, 1) == (True, [3])
        assert dv.read([], True, 1) == (True, [3])
    else:
        with pytest.raises(ReferenceRaises):
            dv.read([], False, 1)


def test_gset_integer_path_is_the_oracles():
    """the model's shortcut for G-Sets of integers against oracle.lattice.threshold_met on
    random sorted, unsorted and repeating lists, strict and not"""
    import random

    from oracle import lattice as olat
    rng = random.Random(5)
    seen = set()
    for _ in range(600):
        a = [rng.randrange(12) for _ in range(rng.randrange(7))]
        b = rng.choice([a, sorted(set(a)), a + [rng.randrange(12)], a[1:], a[::-1],
                        [rng.randrange(12) for _ in range(rng.randrange(7))]])
        for th in (a, ("strict", a)):
            want = olat.threshold_met("lasp_gset", b, th)
            assert rm._gset_of_ints(b, th) is want, (a, b, th)
            seen.add((want, th is a))
    assert len(seen) == 4
    assert rm._gset_of_ints([1, 2.0], [1]) is None and rm._gset_of_ints([True], []) is None


def test_counter_lazy_threshold_raises_at_the_next_read():
    """a counter's lazy threshold is a number; reply_to_all hands it to
    riak_dt_gcounter:value/1 as a value (:798 over lasp_lattice.erl:87-90)"""
    dv = Dv("riak_dt_gcounter")
    dv.value = [(b"a", 2)]
    assert dv.wait_needed(5, False, 1) is False and dv.lazy == [(1, 5)]
    with pytest.raises(ReferenceRaises):
        dv.read(1, False, 2)
