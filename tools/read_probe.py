"""What a blocking read costs at the drop-in boundary (lasp_core.erl:331-420), the one-pass
reads against laspj_var_wait.  10,000-element OR-Set variables; every threshold is
`{strict, Value}` of the variable's own value — unmet, so the read blocks, and made of terms
its namespace knows.  Timed in this one process after a warm-up with a host clock around C
calls that end in a device synchronisation; the two sides of (a) and of (b) run one after
the other every round, on twin variables; the waiter a read leaves is cancelled off the
clock.

  (a) laspj_var_read that blocks, against laspj_var_wait that blocks (the path as it was:
      the threshold as an image call, then its decode into the waiter's cells);
  (b) laspj_var_read_any over 16 variables, none met, against 16 blocking laspj_var_wait;
  (c) laspj_var_read on a variable holding 16 lazy threads of 10,000 elements each (none
      fires, so they stay), against (a): the lazy walk's increment;
  (d) laspj_nif_stats [1] (device passes) per call of each leg.

Medians with the 10th and 90th percentiles.  The last line is JSON; the report is also
written to profiles/read_probe.txt (or --out PATH).

    python tools/read_probe.py [rounds] [--out PATH]
"""
import ctypes as C
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

N, MANY, LAZY = 10000, 16, 16


def tb(t):
    return etf.term_to_binary(t)


def stats_us(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]  # noqa: E731
    return {"median_us": round(statistics.median(xs) * 1e6, 2),
            "p10_us": round(q(0.10) * 1e6, 2), "p90_us": round(q(0.90) * 1e6, 2)}


def filled(ctx):
    """A variable holding 0..N-1 and its value's image."""
    v = ctx.var("orset")
    if v.update(tb((Atom("add_all"), list(range(N)))))[:2] != (0, 0):
        raise RuntimeError("probe: add_all fell back")
    verd, img = v.read()
    if verd != 0:
        raise RuntimeError("probe: the value's read fell back")
    return v, img


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.met, self.vd, self.found = C.c_int32(), C.c_int32(), C.c_int32()
        self.nl, self.still = C.c_uint32(), C.c_uint32()
        self.ids = (C.c_uint64 * 64)()

    def passes(self):
        return self.ctx.nif_stats()["device_passes"]

    def read(self, v, img, wid):
        t0 = time.perf_counter()
        check(self.L.laspj_var_read(v.h, img, len(img), 1, wid, C.byref(self.met), self.ids, 64,
                                    C.byref(self.nl), C.byref(self.still), C.byref(self.vd)),
              self.ctx.h)
        t = time.perf_counter() - t0
        if (self.vd.value, self.met.value, self.nl.value) != (0, 0, 0):
            raise RuntimeError("probe: laspj_var_read did not block")
        return t

    def wait(self, v, img, wid):
        t0 = time.perf_counter()
        check(self.L.laspj_var_wait(v.h, img, len(img), 1, wid, C.byref(self.met),
                                    C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if (self.vd.value, self.met.value) != (0, 0):
            raise RuntimeError("probe: laspj_var_wait did not block")
        return t


def legs_ac(ctx, rounds, warm):
    T = Timed(ctx)
    a, img_a = filled(ctx)
    w, img_w = filled(ctx)
    c, img_c = filled(ctx)
    # 16 lazy thresholds the read's does not reach: each lacks element 0 and wants a token
    # on its own element that the value does not hold
    val = etf.binary_to_term(img_c)
    for j in range(LAZY):
        th = [(e, toks + [(bytes(20), False)] if e == j + 1 else toks) for e, toks in val[1:]]
        th = [(e, sorted(toks)) for e, toks in th]
        if c.wait_needed(tb(th), False, 100 + j) is not False:
            raise RuntimeError("probe: a lazy thread did not register")
    ta, tw, tc = [], [], []
    pa = pw = pc = 0
    for r in range(warm + rounds):
        p0 = T.passes()
        t1 = T.read(a, img_a, 1)
        p1 = T.passes()
        t2 = T.wait(w, img_w, 1)
        p2 = T.passes()
        t3 = T.read(c, img_c, 1)
        p3 = T.passes()
        if T.still.value != LAZY:
            raise RuntimeError("probe: the lazy threads left")
        for v in (a, w, c):
            if not v.cancel(1):
                raise RuntimeError("probe: no waiter was left")
        if r >= warm:
            ta.append(t1)
            tw.append(t2)
            tc.append(t3)
            pa, pw, pc = pa + p1 - p0, pw + p2 - p1, pc + p3 - p2
    return ta, tw, tc, [pa / rounds, pw / rounds, pc / rounds]


def leg_b(ctx, rounds, warm):
    T, L = Timed(ctx), ctx.L
    ra = [filled(ctx) for _ in range(MANY)]
    wa = [filled(ctx) for _ in range(MANY)]
    vs = (C.c_void_p * MANY)(*[v.h.value for v, _i in ra])
    pv = (C.c_char_p * MANY)(*[i for _v, i in ra])
    nv = (C.c_uint64 * MANY)(*[len(i) for _v, i in ra])
    st = (C.c_int32 * MANY)(*([1] * MANY))
    nl = (C.c_uint32 * MANY)()
    tr, tw = [], []
    pr = pw = 0
    for r in range(warm + rounds):
        p0 = T.passes()
        t0 = time.perf_counter()
        check(L.laspj_var_read_any(ctx.h, MANY, vs, pv, nv, st, 1, C.byref(T.found), T.ids, 64,
                                   nl, C.byref(T.vd)), ctx.h)
        t1 = time.perf_counter() - t0
        if (T.vd.value, T.found.value) != (0, -1):
            raise RuntimeError("probe: read_any did not block")
        p1 = T.passes()
        t2 = sum(T.wait(v, img, 1) for v, img in wa)
        p2 = T.passes()
        for v, _i in ra + wa:
            if not v.cancel(1):
                raise RuntimeError("probe: no waiter was left")
        if r >= warm:
            tr.append(t1)
            tw.append(t2)
            pr, pw = pr + p1 - p0, pw + p2 - p1
    return tr, tw, [pr / rounds, pw / rounds]


def main():
    argv = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "read_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        out = argv[i + 1]
        del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    ctx = engine.Context(0)
    ta, tw, tc, pac = legs_ac(ctx, rounds, warm=30)
    tr, tws, pb = leg_b(ctx, rounds, warm=30)
    fallbacks = ctx.nif_stats()["fallbacks"]
    ctx.close()
    res = {"rounds": rounds, "elements": N,
           "a_read": stats_us(ta), "a_wait": stats_us(tw),
           "b_read_any_16": stats_us(tr), "b_16_waits": stats_us(tws),
           "c_read_16_lazy": stats_us(tc),
           "d_passes": {"a_read": pac[0], "a_wait": pac[1], "c_read_16_lazy": pac[2],
                        "b_read_any_16": pb[0], "b_16_waits": pb[1]},
           "fallbacks": fallbacks}
    res["wait_over_read"] = round(res["a_wait"]["median_us"] / res["a_read"]["median_us"], 2)
    res["waits_over_read_any"] = round(res["b_16_waits"]["median_us"] /
                                       res["b_read_any_16"]["median_us"], 2)
    line = lambda name, s, p: (f"{name:<52} {s['median_us']:>10} us  "  # noqa: E731
                               f"(p10 {s['p10_us']}, p90 {s['p90_us']})  passes/call {p:g}")
    d = res["d_passes"]
    text = "\n".join([
        f"read_probe: {N}-element OR-Sets, thresholds {{strict, Value}}, {rounds} rounds, medians",
        line("(a) laspj_var_read, blocks", res["a_read"], d["a_read"]),
        line("(a) laspj_var_wait, blocks", res["a_wait"], d["a_wait"]),
        line(f"(b) laspj_var_read_any over {MANY}, none met", res["b_read_any_16"],
             d["b_read_any_16"]),
        line(f"(b) {MANY} laspj_var_wait, each blocks", res["b_16_waits"], d["b_16_waits"]),
        line(f"(c) laspj_var_read beside {LAZY} lazy threads", res["c_read_16_lazy"],
             d["c_read_16_lazy"]),
        f"wait / read = {res['wait_over_read']}    16 waits / read_any = "
        f"{res['waits_over_read_any']}",
        json.dumps(res)])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
