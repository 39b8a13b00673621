"""tests/lvar_reads_model.py pinned on literals transcribed from the reference's clauses
(lasp_core.erl:331-364 read/6, :371-420 read_any/3, :730-758 wait_needed/6, :795-813
reply_to_all's wait clause, :839-844 write/4, over lasp_lattice.erl:72-75, 153-161, 235-253 on
list values), and the committed seed's run shown not to be vacuous.  No GPU."""

import lvar_reads_model as rm

T0, T1, TA, TC = b"t0", b"t1", b"a", b"c"
V1 = [(1, [(T0, False)])]
V12 = [(1, [(T0, False)]), (2, [(T1, False)])]
AHEAD = [(1, [(T0, False)]), (2, [(T1, False)]), (3, [(TA, False)])]


def lazy_var(value, *lazy):
    dv = rm.ListDv()
    dv.value = value
    dv.lazy = list(lazy)
    return dv


def test_met_read_keeps_fired_lazy_entries_and_they_fire_again():
    # :353-354 reply and do not store StillLazy
    dv = lazy_var(V12, (7, AHEAD), (8, V1))
    assert dv.read(V1, False, 100) == (True, [7, 8])
    assert dv.lazy == [(7, AHEAD), (8, V1)] and dv.waiting == []
    assert dv.read(V12, False, 101) == (True, [7])          # V1 does not inflate V12
    assert dv.read(V1, False, 102) == (True, [7, 8])


def test_unmet_read_removes_fired_entries_and_blocks():
    # :356-362: the waiter is appended, lazy_threads := StillLazy
    dv = lazy_var(V1, (7, AHEAD), (8, V1), (9, AHEAD))
    assert dv.read(V12, True, 100) == (False, [7, 9])
    assert dv.lazy == [(8, V1)]
    assert dv.waiting == [(100, True, V12)]


def test_wait_needed_clauses():
    dv = lazy_var(V1)
    assert dv.wait_needed(V1, False, 1) is True             # :735-737 met
    assert dv.wait_needed(V12, False, 2) is False           # :747-755 registered
    assert dv.lazy == [(2, V12)]
    dv.waiting = [(50, False, AHEAD)]
    assert dv.wait_needed(AHEAD, False, 3) is True          # :739-741 somebody reads already
    assert dv.lazy == [(2, V12)]
    dv.waiting = []
    assert dv.wait_needed(AHEAD, True, 4) is None           # {strict, T} would be stored
    assert dv.lazy == [(2, V12)]


def test_strict_wait_needed_that_is_met_answers_needed():
    dv = lazy_var(V12)
    assert dv.wait_needed(V1, True, 1) is True
    assert dv.lazy == []


def test_write_empties_the_lazy_list():
    # :842-843: a fresh #dv
    dv = lazy_var(V1, (7, AHEAD))
    dv.waiting = [(50, False, V12), (51, False, AHEAD)]
    dv.wrote(V12)
    assert dv.lazy == []
    assert dv.write()[0] == [50] and dv.waiting == [(51, False, AHEAD)]


def test_strict_read_against_an_equal_lazy_threshold_does_not_fire():
    dv = lazy_var(AHEAD, (7, V12))
    assert dv.read(V12, True, 100) == (True, [])            # the value is strictly ahead
    assert dv.read(V12, False, 101) == (True, [7])


def test_strict_empty_read_fires_a_non_empty_lazy_threshold_only():
    # is_strict_inflation([], Current) when Current =/= [] (lasp_lattice.erl:235-236)
    dv = lazy_var(V1, (7, V12), (8, []))
    assert dv.read([], True, 100) == (True, [7])
    assert dv.read([], False, 101) == (True, [7, 8])


def test_keyfind_takes_the_first_match_of_a_repeated_lazy_key():
    lazy = [(5, [(TA, False)]), (3, [(T0, False)]), (5, [(TA, False), (TC, False)])]
    dv = lazy_var(lazy, (7, lazy))
    assert dv.read([(5, [(TC, False)])], False, 100) == (False, [])     # only the later holds c
    assert dv.read([(5, [(TA, False)])], False, 101) == (True, [7])


def test_read_any_naming_one_variable_twice():
    # the second read of the variable sees the first read's removals and its waiter
    dv = lazy_var(V1, (7, AHEAD), (8, V1))
    found, fired = rm.read_any([(dv, V12, False), (dv, V1, False), (dv, AHEAD, False)], 100)
    assert (found, fired) == (1, [[7], [8], []])
    assert dv.lazy == [(8, V1)]
    assert dv.waiting == [(100, False, V12)]
    other = lazy_var([], (9, V1))
    found, fired = rm.read_any([(other, V1, False), (dv, AHEAD, True)], 101)
    assert (found, fired) == (-1, [[9], []])
    assert other.lazy == [] and other.waiting == [(101, False, V1)]
    assert dv.waiting[-1] == (101, True, AHEAD)


def test_the_committed_seed_is_not_vacuous():
    sc = rm.ListReadScenario(rm.SEED).run()
    c = sc.c
    assert c["fired_reads"] >= 10, c
    assert c["met_kept"] >= 3, c
    assert c["unmet_removed"] >= 3, c
    assert c["writes_emptied"] >= 3, c
    assert c["needed_by_waiter"] >= 3, c
    assert c["any_found"] >= 2, c
    assert c["any_twice_removed"] >= 1, c
    assert c["registered"] >= 5 and c["strict_fallback"] >= 1, c
    assert all(sc.status[s] >= 3 for s in (rm.NOOP, rm.WRITTEN, rm.REFUSED)), sc.status
