"""What one re-run of a filter process costs at the drop-in boundary (lasp_process.erl:61-95,
lasp_core.erl:681-712), resident against the image path.  A 10,000-element OR-Set `in`, a
predicate keeping half; every step one {add, E} of an element the filter has seen.  Four
legs, timed in this one process after a warm-up with a host clock around C calls that end in
a device synchronisation; (a) and (b) run on the same values, one after the other, every
round:

  (a) laspj_filter_run on the resident filter (one or two launches, one synchronisation);
  (b) today's path: laspj_var_etf_read(in) + laspj_list_etf_args + laspj_list_etf_filter +
      laspj_var_etf_bind(out) — the C calls only: calling the fun 10,000 times and copying
      the images between the calls are left out, in (b)'s favour;
  (c) laspj_filter_run_many over 16 such filters (16 inputs of 10,000 elements, each updated
      before the call), per filter;
  (d) a step whose update adds a never-seen element: run (1 pending) / args / fun /
      results / run.

Medians with the 10th and 90th percentiles.  The last line is JSON; the report is also
written to profiles/filter_probe.txt (or --out PATH).

    python tools/filter_probe.py [rounds] [--out PATH]
"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasp_amd import _lib, engine, etf  # noqa: E402
from lasp_amd._lib import check  # noqa: E402
from lasp_amd.terms import Atom  # noqa: E402

N, MANY = 10000, 16


def tb(t):
    return etf.term_to_binary(t)


def keep(e):
    return e % 2 == 0


def stats_us(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]  # noqa: E731
    return {"median_us": round(statistics.median(xs) * 1e6, 2),
            "p10_us": round(q(0.10) * 1e6, 2), "p90_us": round(q(0.90) * 1e6, 2)}


def add(var, e):
    if var.update(tb((Atom("add"), e)))[:2] != (0, 0):
        raise RuntimeError("probe: update fell back")


def filled(ctx):
    """A variable holding 0..N-1 and a filter over it that has seen them all."""
    v = ctx.var("orset")
    if v.update(tb((Atom("add_all"), list(range(N)))))[:2] != (0, 0):
        raise RuntimeError("probe: add_all fell back")
    f = ctx.filter(v, v.replica())
    if f.step(keep) != (0, 1, 0):
        raise RuntimeError("probe: the first step answered wrongly")
    return v, f


class Timed:
    """The C calls of the legs, each returning its own seconds."""

    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.st, self.pend, self.vd = C.c_int32(), C.c_uint32(), C.c_int32()
        self.out, self.olen, self.cnt = C.c_void_p(), C.c_uint64(), C.c_uint32()

    def run(self, f):
        t0 = time.perf_counter()
        check(self.L.laspj_filter_run(f.h, C.byref(self.st), C.byref(self.pend),
                                      C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: filter_run fell back")
        return t, self.st.value, self.pend.value

    def image(self, fn, *args):
        """An image-answering call: (seconds, a copy of the answer taken off the clock)."""
        t0 = time.perf_counter()
        check(fn(*args, C.byref(self.out), C.byref(self.olen), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: an image call fell back")
        return t, C.string_at(self.out, self.olen.value)


def legs_ab_d(ctx, rounds, warm):
    L, T = ctx.L, Timed(ctx)
    v, f = filled(ctx)
    out_b = v.replica()
    results = None
    ta, tb_, td = [], [], []
    for r in range(warm + rounds):
        add(v, (7 * r) % N)
        # (a)
        t, st_a, pend = T.run(f)
        if pend:
            raise RuntimeError("probe: a seen element was pending")
        # (b) on the same value
        t1, img = T.image(L.laspj_var_etf_read, v.h)
        t2, args = T.image(L.laspj_list_etf_args, ctx.h, _lib.KIND_ORSET, img, len(img))
        if results is None:             # the elements never change: F's answers neither
            results = tb([keep(x) for x in etf.binary_to_term(args)])
        t3, acc = T.image(L.laspj_list_etf_filter, ctx.h, _lib.KIND_ORSET, img, len(img), results,
                          len(results))
        t0 = time.perf_counter()
        check(L.laspj_var_etf_bind(out_b.h, acc, len(acc), C.byref(T.st), C.byref(T.vd)), ctx.h)
        t4 = time.perf_counter() - t0
        if T.vd.value != 0 or T.st.value != st_a:
            raise RuntimeError("probe: the two paths answered differently")
        if r >= warm:
            ta.append(t)
            tb_.append(t1 + t2 + t3 + t4)
    if f.out_var.read() != out_b.read():
        raise RuntimeError("probe: the two paths' outputs differ")
    # (d): a never-seen element per step
    for r in range(warm + rounds):
        add(v, N + r)
        t0 = time.perf_counter()
        _t, _st, pend = T.run(f)
        check(L.laspj_filter_args(f.h, C.byref(T.out), C.byref(T.olen), C.byref(T.cnt),
                                  C.byref(T.vd)), ctx.h)
        res = tb([keep(x) for x in etf.binary_to_term(C.string_at(T.out, T.olen.value))])
        check(L.laspj_filter_results(f.h, res, len(res)), ctx.h)
        _t, st, pend2 = T.run(f)
        t = time.perf_counter() - t0
        if (pend, T.cnt.value, pend2) != (1, 1, 0) or st != int(keep(N + r)):
            raise RuntimeError("probe: the pending round answered wrongly")
        if r >= warm:
            td.append(t)
    return ta, tb_, td


def leg_c(ctx, rounds, warm):
    L = ctx.L
    made = [filled(ctx) for _ in range(MANY)]
    fs = (C.c_void_p * MANY)(*[f.h.value for _v, f in made])
    st, pend, vd = (C.c_int32 * MANY)(), (C.c_uint32 * MANY)(), (C.c_int32 * MANY)()
    tc = []
    for r in range(warm + rounds):
        for k, (v, _f) in enumerate(made):
            add(v, (7 * r + k) % N)
        t0 = time.perf_counter()
        check(L.laspj_filter_run_many(ctx.h, MANY, fs, st, pend, vd), ctx.h)
        t = (time.perf_counter() - t0) / MANY
        if any(vd) or any(pend) or [int(x) for x in st] != [int(keep((7 * r + k) % N))
                                                            for k in range(MANY)]:
            raise RuntimeError("probe: run_many answered wrongly")
        if r >= warm:
            tc.append(t)
    return tc


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "filter_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    ctx = engine.Context(0)
    ta, tb_, td = legs_ab_d(ctx, rounds, warm=30)
    tc = leg_c(ctx, rounds, warm=30)
    fallbacks = ctx.nif_stats()["fallbacks"]
    ctx.close()
    res = {"rounds": rounds, "elements": N, "a_filter_run": stats_us(ta),
           "b_image_path": stats_us(tb_), "c_run_many_per_filter": stats_us(tc),
           "d_pending_round": stats_us(td), "fallbacks": fallbacks}
    res["b_over_a"] = round(res["b_image_path"]["median_us"] / res["a_filter_run"]["median_us"], 2)
    res["a_over_c"] = round(res["a_filter_run"]["median_us"] /
                            res["c_run_many_per_filter"]["median_us"], 2)
    line = lambda name, s: (f"{name:<58} {s['median_us']:>10} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    text = "\n".join([
        f"filter_probe: {N}-element OR-Set, predicate keeps half, {rounds} rounds, medians",
        line("(a) laspj_filter_run, a seen element re-added", res["a_filter_run"]),
        line("(b) etf_read + list_etf_args + list_etf_filter + etf_bind", res["b_image_path"]),
        line(f"(c) laspj_filter_run_many over {MANY} filters, per filter",
             res["c_run_many_per_filter"]),
        line("(d) a never-seen element: run / args / results / run", res["d_pending_round"]),
        f"b / a = {res['b_over_a']}    a / c = {res['a_over_c']}",
        json.dumps(res)])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
