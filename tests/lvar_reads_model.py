"""A reference model of `#dv{value, waiting_threads, lazy_threads}` (include/lasp.hrl:60-63)
on a list value, and the random scenario the list read tests run
(tests/test_lvar_reads_model.py on the model alone, tests/test_gpu_lvar_reads.py against the
device).

  read/6         lasp_core.erl:331-364     ListDv.read
  read_any/3     :371-420                  read_any
  wait_needed/6  :730-758                  ListDv.wait_needed
  reply_to_all   :765-825                  ListDv.write (read entries), _reply_lazy (wait)
  write/4        :839-844                  ListDv.wrote (the fresh #dv), then ListDv.write

It is tests/reads_model.Dv over tests/lvars_model.threshold: threshold_met(lasp_orset, V, T) on
lists that need not be orddicts (lasp_lattice.erl:72-75, 153-161, 235-253).  One difference:
wait_needed/6 with {strict, T} that would register answers None and keeps nothing — the
reference stores the tuple and crashes in lists:keyfind when a later read hands it to the
list clauses as a value (:798), so the device answers FALLBACK there and the NIF runs the
reference's own clause.
"""

import lvar_waiters_model as lwm
import lvars_model as lm
import waiters_model as wm

OK, FALLBACK = wm.OK, wm.FALLBACK
NOOP, WRITTEN, REFUSED = lm.NOOP, lm.WRITTEN, lm.REFUSED
tb = wm.tb


class ListDv(lwm.ListReplyModel):
    """one list-valued variable: value, waiting_threads [(id, strict, threshold)] (the
    inherited wait / write / cancel / listing) and lazy_threads [(id, threshold)]"""

    def __init__(self):
        super().__init__()
        self.lazy = []

    # reply_to_all/3's {threshold, wait, ...} clause (:795-813) over lazy_threads: the read's
    # threshold is the previous state, the lazy one the current
    def _reply_lazy(self, th, strict):
        fired, still = [], []
        for lid, lth in self.lazy:
            if lm.threshold(lth, th, strict):
                fired.append(lid)
            else:
                still.append((lid, lth))
        return fired, still

    def read(self, th, strict, rid):
        """read/6 (:331-364): (met, [lazy ids replied to])."""
        fired, still = self._reply_lazy(th, strict)                         # :348-349
        if lm.threshold(self.value, th, strict):                            # :352
            return True, fired              # :353-354: ReplyFun only — StillLazy is dropped
        self.waiting.append((rid, bool(strict), th))                        # :356-361
        self.lazy = still                                                   # :362
        return False, fired

    def wait_needed(self, th, strict, wid):
        """wait_needed/6 (:730-758): True — reply at once; False — appended to lazy_threads;
        None — {strict, T} would be stored (see the module's text)."""
        if lm.threshold(self.value, th, strict):                            # :735-737
            return True
        if self.waiting:                                                    # :739-741
            return True
        if strict:
            return None
        self.lazy = self.lazy + [(wid, th)]                                 # :747-755
        return False

    def wrote(self, value):
        """write/4's stored record (:842-843): a fresh #dv — lazy_threads is [] again; the
        waiters are replied to by write() (reply_to_all, :840-841)."""
        self.value = value
        self.lazy = []

    def lazy_cancel(self, lid):
        for k, z in enumerate(self.lazy):
            if z[0] == lid:
                del self.lazy[k]
                return True
        return False

    def lazy_listing(self):
        return [(i, tb(th)) for i, th in self.lazy]


def read_any(reads, rid):
    """read_any/3 (:371-420) over [(ListDv, threshold, strict)]: (index of the first read met
    or -1, [[lazy ids replied to] per read]).  The fold visits a read only while none before
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


class ListReadScenario(lwm.ListScenario):
    """~`steps` random steps on l, r, the list variable out that intersection/7 re-runs into
    and a second list variable out2 of the namespace: updates on l and r, the re-run (plain or
    fused with the re-check), a foreign bind, a write, wait_needed, read, read_any over out
    and out2 (sometimes naming out twice), lazy_cancel, wait, cancel; a re-check after every
    write and every WRITTEN.  dev: None (the model alone) or an object with l, r
    (engine.NifVar of one namespace), out and out2 (engine.NifListVar) and read_any
    (engine.list_read_any), every answer of which is asserted against the model."""

    def __init__(self, seed, dev=None, passes=None):
        super().__init__(seed, dev, passes)
        self.m = ListDv()
        self.m2 = ListDv()
        self.c = dict(fired_reads=0, met_kept=0, unmet_removed=0, writes_emptied=0,
                      needed_by_waiter=0, needed_met=0, registered=0, strict_fallback=0,
                      any_found=0, any_none=0, any_twice_removed=0, lazy_cancels=0)

    # ---- bookkeeping the inherited re-check needs: one uid per entry of m.waiting
    def note_waiter(self, strict):
        self.uid += 1
        self.uids.append(self.uid)
        self.live[self.uid] = bool(strict)

    def compare(self, step):
        d = self.devs
        if d is None:
            return
        assert d.out.lazy() == self.m.lazy_listing(), step
        assert d.out.waiters() == self.m.listing(), step
        assert d.out2.lazy() == self.m2.lazy_listing(), step
        assert d.out2.waiters() == self.m2.listing(), step
        assert d.out.read() == (OK, tb(self.m.value)), step
        assert d.out2.read() == (OK, tb(self.m2.value)), step

    def recheck(self, step, got=None):
        """every WRITTEN and every write comes here: the stored record is a fresh #dv"""
        if self.m.lazy:
            self.c["writes_emptied"] += 1
        self.m.lazy = []
        if self.devs is not None:
            assert self.devs.out.lazy() == [], step
        return super().recheck(step, got)

    # ---- generators
    def read_threshold(self, m):
        """near a lazy threshold (so that it fires), near the value, or anything"""
        rng = self.rng
        if m.lazy and rng.random() < 0.55:
            s = rng.choice(m.lazy)[1]
            r = rng.random()
            if r < 0.5:
                return self.sub_list(s)
            if r < 0.7:
                return [(k, list(t)) for k, t in s]
            return self.mutate(s)
        if m is self.m:
            return self.threshold()
        return self.mutate(m.value)

    def lazy_threshold(self, m):
        """mostly ahead of the value, so that it registers"""
        rng = self.rng
        if m is self.m and rng.random() < 0.5:
            return self.threshold()
        e = rng.choice(self.ELEMS)
        s = lm.bind(m.value, [(e, [(self.tok_for(e), False)])])[1]
        if rng.random() < 0.3 and s:
            s = s + [rng.choice(s)]
        return s if rng.random() < 0.7 else self.sub_list(s)

    # ---- steps
    def readers_leave(self, step):
        """every waiter of out is cancelled (its process died), so that wait_needed registers"""
        for wid in [w[0] for w in self.m.waiting]:
            assert self.m.cancel(wid)
            del self.live[self.uids.pop(0)]
            if self.devs is not None:
                assert self.devs.out.cancel(wid) is True, step

    def do_wait_needed(self, step, m, dev):
        if m is self.m and m.waiting and self.rng.random() < 0.6:
            self.readers_leave(step)
        th, strict = self.lazy_threshold(m), self.rng.random() < 0.15
        wid, self.next_id = self.next_id, self.next_id + 1
        unmet = not lm.threshold(m.value, th, strict)
        want = m.wait_needed(th, strict, wid)
        if want is None:
            self.c["strict_fallback"] += 1
        elif not want:
            self.c["registered"] += 1
        elif unmet:
            self.c["needed_by_waiter"] += 1
        else:
            self.c["needed_met"] += 1
        if dev is not None:
            assert dev.wait_needed(tb(th), strict, wid) is want, (step, strict, th)

    def do_read(self, step):
        m = self.m
        th, strict = self.read_threshold(m), self.rng.random() < 0.4
        rid, self.next_id = self.next_id, self.next_id + 1
        had = len(m.lazy)
        met, fired = m.read(th, strict, rid)
        if fired:
            self.c["fired_reads"] += 1
        if met and had:
            self.c["met_kept"] += 1
        if not met:
            self.note_waiter(strict)
            if fired:
                self.c["unmet_removed"] += 1
        if self.devs is not None:
            got = self.devs.out.read(tb(th), strict, rid, cap=2)
            assert got == (met, fired), (step, got, met, fired)

    def do_read_any(self, step):
        rng = self.rng
        which = [rng.random() < 0.6 for _ in range(rng.randint(2, 4))]      # True: out
        if rng.random() < 0.4:
            which[0] = which[-1] = True                                     # out named twice
        reads = []
        for w in which:
            m = self.m if w else self.m2
            reads.append((m, self.read_threshold(m), rng.random() < 0.4))
        rid, self.next_id = self.next_id, self.next_id + 1
        found, fired = read_any(reads, rid)
        for m, _th, strict in reads[:found] if found >= 0 else reads:
            if m is self.m:
                self.note_waiter(strict)                            # an unmet read blocks
        if found >= 1:
            self.c["any_found"] += 1
        if found < 0:
            self.c["any_none"] += 1
        outs = [k for k, w in enumerate(which) if w]
        if len(outs) >= 2 and fired[outs[0]] and (found < 0 or found >= outs[1]):
            self.c["any_twice_removed"] += 1    # the second read of out saw the removal
        if self.devs is not None:
            d = self.devs
            dreads = [(d.out if w else d.out2, tb(th), s) for w, (_m, th, s) in zip(which, reads)]
            got = d.read_any(dreads, rid, cap=2)
            assert got == (found, fired), (step, got, found, fired)

    def write2(self, step):
        """out2 takes a value of its own: written, or bound from a foreign list"""
        rng, m2, d = self.rng, self.m2, self.devs
        if rng.random() < 0.5:
            v = self.mutate(self.m.value) if rng.random() < 0.6 else self.descending()
            if d is not None:
                assert d.out2.write(tb(v)) == OK, (step, v)
            st = WRITTEN
        else:
            foreign = self.descending()
            st, v = lm.bind(m2.value, foreign)
            if d is not None:
                assert d.out2.bind(tb(foreign)) == (OK, st), (step, foreign)
        if st != WRITTEN:
            return
        m2.wrote(v)
        fired, _flags = m2.write()
        if d is not None:
            assert d.out2.lazy() == [], step
            assert d.out2.recheck(cap=8) == (OK, fired, len(m2.waiting)), step

    def step(self, step):
        rng, d = self.rng, self.devs
        r = rng.random()
        if r < 0.14:
            self.update(step)
        elif r < 0.23:
            self.rerun(step)
        elif r < 0.25:
            v = self.descending()
            st, new = lm.bind(self.m.value, v)
            self.status[st] += 1
            if d is not None:
                assert d.out.bind(tb(v)) == (OK, st), (step, v)
            if st == WRITTEN:
                self.changed(new, step)
        elif r < 0.28:
            k = rng.random()
            v = lm.acc_value(self.lval, self.rval) if k < 0.6 else \
                self.mutate(self.m.value) if k < 0.9 else self.descending()
            if d is not None:
                assert d.out.write(tb(v)) == OK, (step, v)
            self.changed(v, step)                                   # write/4 always replies
        elif r < 0.50:
            if rng.random() < 0.75:
                self.do_wait_needed(step, self.m, d.out if d is not None else None)
            else:
                self.do_wait_needed(step, self.m2, d.out2 if d is not None else None)
        elif r < 0.75:
            self.do_read(step)
        elif r < 0.85:
            self.do_read_any(step)
        elif r < 0.88:
            lid = rng.choice(self.m.lazy)[0] if self.m.lazy and rng.random() < 0.7 else 10 ** 9
            found = self.m.lazy_cancel(lid)
            self.c["lazy_cancels"] += found
            if d is not None:
                assert d.out.lazy_cancel(lid) is found, step
        elif r < 0.91:
            th, strict = self.threshold(), rng.random() < 0.5
            wid, self.next_id = self.next_id, self.next_id + 1
            met = self.m.wait(th, strict, wid)
            if not met:
                self.note_waiter(strict)
            if d is not None:
                assert d.out.wait(tb(th), strict, wid) == (OK, met), (step, strict, th)
        elif r < 0.96:
            # a waiter leaves (so that wait_needed registers again)
            wid = rng.choice(self.m.waiting)[0] if self.m.waiting else 10 ** 9
            k = next((k for k, w in enumerate(self.m.waiting) if w[0] == wid), None)
            found = self.m.cancel(wid)
            if found:
                del self.live[self.uids.pop(k)]
            if d is not None:
                assert d.out.cancel(wid) is found, step
        else:
            self.write2(step)
        self.compare(step)


# the seed at which the model's run is not vacuous (tests/test_lvar_reads_model.py asserts it)
SEED = 0
