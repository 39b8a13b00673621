"""What a blocking read on a list-valued variable costs with its lazy threads beside it
(lasp_core.erl:331-364, 371-420, 795-813), against laspj_lvar_wait.  The value is the lvar
probe's: out = the intersection of l and r, 10,000 elements each sharing 5,000; the thresholds
are prefixes of it (all but its last entry, so every read is met and nothing is kept).  Legs,
timed in this one process after a warm-up with a host clock around the C calls, one after the
other every round:

  (a) laspj_lvar_wait — and, with --parent PATH (a built checkout of the parent commit, its
      library loaded beside this tree's), the same call there;
  (b) laspj_lvar_read with no lazy entries;
  (c) laspj_lvar_read with 16 lazy entries of 5,000 entries each (all 16 fire and stay);
  (d) laspj_lvar_read_any of 4 reads (the pass checks all four, the fold stops at the first);
  (e) 4 laspj_lvar_read calls in sequence.

Medians with the 10th and 90th percentiles.  The last line is JSON; the report is also
written to profiles/lvar_reads_probe.txt (or --out PATH).

    python tools/lvar_reads_probe.py [rounds] [--parent PATH] [--out PATH]
"""
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from lasp_amd import engine, etf  # noqa: E402
from lasp_amd._lib import check  # noqa: E402
from lasp_amd.terms import Atom  # noqa: E402

N = 10000
HALF = N // 2
LAZY = 16


def tb(t):
    return etf.term_to_binary(t)


def stats_us(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]  # noqa: E731
    return {"median_us": round(statistics.median(xs) * 1e6, 2),
            "p10_us": round(q(0.10) * 1e6, 2), "p90_us": round(q(0.90) * 1e6, 2)}


def parent_engine(path):
    """the parent checkout's package under a name of its own (its library is its own file)"""
    pkg = os.path.join(path, "lasp_amd")
    spec = importlib.util.spec_from_file_location(
        "lasp_amd_parent", os.path.join(pkg, "__init__.py"), submodule_search_locations=[pkg])
    mod = importlib.util.module_from_spec(spec)
    sys.modules["lasp_amd_parent"] = mod
    spec.loader.exec_module(mod)
    return importlib.import_module("lasp_amd_parent.engine")


def setup(eng):
    """(ctx, out): out = the intersection of l = 0 .. N-1 and r = N/2 .. 3N/2-1"""
    ctx = eng.Context(0)
    l = ctx.var("orset")
    r = l.replica()
    for var, first in ((l, 0), (r, HALF)):
        if var.update(tb((Atom("add_all"), list(range(first, first + N)))))[:2] != (0, 0):
            raise RuntimeError("probe: update fell back")
    out = ctx.list_var(l)
    if out.intersection(l, r) != (0, 1):
        raise RuntimeError("probe: the intersection was not written")
    return ctx, out, (l, r)


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.met, self.vd = C.c_int32(), C.c_int32()
        self.nl, self.still, self.found = C.c_uint32(), C.c_uint32(), C.c_int32()
        self.ids = (C.c_uint64 * 64)()
        self.nls = (C.c_uint32 * 4)()

    def wait(self, out, th):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_wait(out.h, th, len(th), 0, 1, C.byref(self.met),
                                     C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if (self.vd.value, self.met.value) != (0, 1):
            raise RuntimeError("probe: lvar_wait was not met")
        return t

    def read(self, out, th, fired):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_read(out.h, th, len(th), 0, 1, C.byref(self.met), self.ids, 64,
                                     C.byref(self.nl), C.byref(self.still), C.byref(self.vd)),
              self.ctx.h)
        t = time.perf_counter() - t0
        if (self.vd.value, self.met.value, self.nl.value, self.still.value) != (0, 1, fired, fired):
            raise RuntimeError("probe: lvar_read answered wrongly")
        return t

    def read_any(self, out, th):
        vs = (C.c_void_p * 4)(*[out.h.value] * 4)
        pv = (C.c_char_p * 4)(*[th] * 4)
        nv = (C.c_uint64 * 4)(*[len(th)] * 4)
        st = (C.c_int32 * 4)(0, 0, 0, 0)
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_read_any(self.ctx.h, 4, vs, pv, nv, st, 1, C.byref(self.found),
                                         self.ids, 64, self.nls, C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if (self.vd.value, self.found.value) != (0, 0):
            raise RuntimeError("probe: lvar_read_any answered wrongly")
        return t


def main():
    argv = sys.argv[1:]
    path, parent = os.path.join(ROOT, "profiles", "lvar_reads_probe.txt"), None
    for flag in ("--out", "--parent"):
        if flag in argv:
            i = argv.index(flag)
            if flag == "--out":
                path = argv[i + 1]
            else:
                parent = argv[i + 1]
            del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    warm = 30
    ctx, out, _keep = setup(engine)
    T = Timed(ctx)
    value = etf.binary_to_term(out.read()[1])
    if len(value) != HALF:
        raise RuntimeError("probe: the value is not the shared half")
    th = tb(value[:-1])
    # (c): the same value in a variable of its own with 16 lazy thresholds of 5,000 entries,
    # each unmet by a last entry of its own that the value does not hold
    out_c = ctx.list_var(_keep[0])
    if out_c.write(out.read()[1]) != 0:
        raise RuntimeError("probe: the write fell back")
    for k in range(LAZY):
        gate = (3 * N + k, [(bytes(19) + bytes([k]), False)])
        if out_c.wait_needed(tb(value[:-1] + [gate]), False, 100 + k) is not False:
            raise RuntimeError("probe: a lazy threshold did not register")
    P = None
    if parent:
        pctx, pout, _pkeep = setup(parent_engine(parent))
        P = Timed(pctx)
        pth = tb(etf.binary_to_term(pout.read()[1])[:-1])     # (its tokens are its own)
    ta, tp, tb_, tc, td, te = [], [], [], [], [], []
    for k in range(warm + rounds):
        a = T.wait(out, th)
        p = P.wait(pout, pth) if P else 0.0
        b = T.read(out, th, 0)
        c = T.read(out_c, th, LAZY)
        d = T.read_any(out, th)
        e = sum(T.read(out, th, 0) for _ in range(4))
        if k >= warm:
            ta.append(a)
            tp.append(p)
            tb_.append(b)
            tc.append(c)
            td.append(d)
            te.append(e)
    stats = ctx.nif_stats()
    if out.waiters() or out_c.waiters() or len(out_c.lazy()) != LAZY:
        raise RuntimeError("probe: a read left something behind")
    ctx.close()
    if P:
        P.ctx.close()
    res = {"rounds": rounds, "value_entries": HALF, "threshold_entries": HALF - 1,
           "a_wait": stats_us(ta), "b_read_0_lazy": stats_us(tb_),
           "c_read_16_lazy": stats_us(tc), "d_read_any_4": stats_us(td),
           "e_4_reads": stats_us(te), "fallbacks": stats["fallbacks"]}
    if P:
        res["a_wait_parent"] = stats_us(tp)
    res["b_over_a"] = round(res["b_read_0_lazy"]["median_us"] / res["a_wait"]["median_us"], 2)
    res["d_over_e"] = round(res["d_read_any_4"]["median_us"] / res["e_4_reads"]["median_us"], 2)
    line = lambda name, s: (f"{name:<62} {s['median_us']:>10} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    rows = [f"lvar_reads_probe: a value of {HALF} entries (l, r of {N} sharing {HALF}), "
            f"thresholds of {HALF - 1}, {rounds} rounds, medians",
            line("(a) laspj_lvar_wait, met", res["a_wait"])]
    if P:
        rows.append(line("    the same on the parent commit", res["a_wait_parent"]))
    rows += [line("(b) laspj_lvar_read, no lazy entries", res["b_read_0_lazy"]),
             line("(c) laspj_lvar_read, 16 lazy entries of 5,000, all fire", res["c_read_16_lazy"]),
             line("(d) laspj_lvar_read_any of 4 reads", res["d_read_any_4"]),
             line("(e) 4 x laspj_lvar_read", res["e_4_reads"]),
             f"b / a = {res['b_over_a']}    d / e = {res['d_over_e']}",
             json.dumps(res)]
    text = "\n".join(rows)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
