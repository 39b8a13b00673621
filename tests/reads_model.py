"""A reference model of `#dv{value, waiting_threads, lazy_threads}` (include/lasp.hrl:60-63)
and the calls of lasp_core.erl that touch the two lists, transcribed clause by clause over
oracle.lattice.threshold_met and the oracle's set types (tests/test_reads_model.py pins it
to the reference's text, tests/test_gpu_reads.py compares the device with it).

  read/6         lasp_core.erl:331-364     Dv.read
  read_any/3     :371-420                  read_any
  wait_needed/6  :730-758                  Dv.wait_needed
  reply_to_all   :765-825                  _reply_waiting (read entries), _reply_lazy (wait)
  write/4        :839-844                  Dv.write

Ids stand for the `From` of an entry.  Where the reference raises, the model raises
ReferenceRaises; the device answers FALLBACK there (the NIF then runs the reference's own
clause, crash included).
"""

from oracle import lattice as olat

from waiters_model import TYPES, tb

OK, FALLBACK = 0, 1


class ReferenceRaises(Exception):
    """the reference's clause crashes here (badarg / function_clause)"""


def _is_strict(th):
    return isinstance(th, tuple) and len(th) == 2 and th[0] == "strict"


def threshold_met(type_, value, threshold):
    """lasp_lattice:threshold_met/3 (:62-75, 87-90) with the crashes of a `value` that is no
    state of the type: a `{strict, T}` tuple (a lazy threshold stored by wait_needed/6 and
    handed back as a value, lasp_core.erl:798) and, for riak_dt_gcounter, a number."""
    if type_ == "riak_dt_gcounter":
        if not isinstance(value, list):
            raise ReferenceRaises("riak_dt_gcounter:value/1 of a number")
        return olat.threshold_met(type_, value, threshold)
    if _is_strict(value):
        prev = threshold[1] if _is_strict(threshold) else threshold
        if type_ == "lasp_gset":
            raise ReferenceRaises("sets:from_list/1 of a tuple")            # :137-140
        if prev == []:
            # lists:foldl over [] never looks at Current (:153-161); the strict clause's
            # guard `Current =/= []` holds (:235-236)
            return True
        raise ReferenceRaises("lists:keyfind/3 in a tuple")                 # :155, :245
    if type_ == "lasp_gset":
        fast = _gset_of_ints(value, threshold)
        if fast is not None:
            return fast
    return olat.threshold_met(type_, value, threshold)


def _gset_of_ints(value, threshold):
    """threshold_met(lasp_gset, ...) over lists of plain integers, or None when either holds
    anything else.  For integers `==`, `=:=` and Python's equality coincide, so :137-140 is
    a subset test and :212-215 adds `the sets differ`; the shape tests compare G-Sets of
    tens of thousands of integers, which oracle.lattice walks term by term
    (tests/test_reads_model.py holds the two equal on random inputs)."""
    strict = _is_strict(threshold)
    prev = threshold[1] if strict else threshold
    if not (isinstance(prev, list) and isinstance(value, list)) or \
            not all(type(e) is int for e in prev) or not all(type(e) is int for e in value):
        return None
    p, c = set(prev), set(value)
    return p <= c and (not strict or p != c)


class Dv:
    """one variable: value, waiting_threads [(id, strict, threshold)] and lazy_threads
    [(id, threshold)] — a lazy threshold is the term wait_needed/6 was given, `("strict",
    T)` included — in list order"""

    def __init__(self, kind):
        self.kind = kind
        self.type = TYPES.get(kind, kind)
        self.value = []
        self.waiting = []
        self.lazy = []
        self._images = {}

    # reply_to_all/3's {threshold, wait, ...} clause (:795-813) over lazy_threads
    def _reply_lazy(self, rthreshold):
        fired, still = [], []
        for lid, lth in self.lazy:
            if threshold_met(self.type, lth, rthreshold):
                fired.append(lid)
            else:
                still.append((lid, lth))
        return fired, still

    # reply_to_all/3's {threshold, read, ...} clause (:774-794) over waiting_threads
    def _reply_waiting(self, value):
        fired, still = [], []
        for wid, strict, th in self.waiting:
            if threshold_met(self.type, value, ("strict", th) if strict else th):
                fired.append(wid)
            else:
                still.append((wid, strict, th))
        return fired, still

    def read(self, th, strict, rid):
        """read/6 (:331-364): (met, [lazy ids replied to]).  The caller has replaced
        `undefined` by Type:new() (:339-346)."""
        threshold = ("strict", th) if strict else th
        fired, still_lazy = self._reply_lazy(threshold)                     # :348-349
        if threshold_met(self.type, self.value, threshold):                 # :352
            return True, fired              # :353-354: ReplyFun only — StillLazy is dropped
        self.waiting = self.waiting + [(rid, bool(strict), th)]             # :356-361
        self.lazy = still_lazy                                              # :362
        return False, fired

    def wait_needed(self, th, strict, wid):
        """wait_needed/6 (:730-758): True — ReplyFun(Threshold) at once; False — the entry
        is appended to lazy_threads and the caller blocks."""
        threshold = ("strict", th) if strict else th
        if threshold_met(self.type, self.value, threshold):                 # :735-737
            return True
        if self.waiting:                                                    # :739-741
            return True
        self.lazy = self.lazy + [(wid, threshold)]                          # :747-755
        return False

    def write(self, value):
        """write/4 (:839-844): the waiters met by `value` are replied to; the stored record
        is a fresh #dv — lazy_threads is the record's default, []."""
        fired, still = self._reply_waiting(value)                           # :840-841
        self.value = value
        self.waiting = still
        self.lazy = []                                                      # :842-843
        return fired

    def image(self, th):
        """tb(th), encoded once per threshold object (the listings are compared after
        every call, and a threshold may be tens of thousands of elements)"""
        hit = self._images.get(id(th))
        if hit is None or hit[0] is not th:
            hit = self._images[id(th)] = (th, tb(th))
        return hit[1]

    def waiting_listing(self):
        return [(i, s, self.image(th)) for i, s, th in self.waiting]

    def lazy_listing(self):
        return [(i, self.image(th)) for i, th in self.lazy]


def read_any(reads, rid):
    """read_any/3 (:371-420) over [(Dv, threshold, strict)]: (index of the first read met or
    -1, [[lazy ids replied to] per read]).  The fold visits a read only while none before
    it was met (:373-374, 411-412)."""
    found, fired = -1, []
    for k, (dv, th, strict) in enumerate(reads):
        if found >= 0:
            fired.append([])
            continue
        met, ids = dv.read(th, strict, rid)                                 # :375-410
        fired.append(ids)
        if met:
            found = k
    return found, fired
