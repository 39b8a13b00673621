"""What the reply path of a list-valued variable costs at the drop-in boundary (read/6 and
write/4's reply_to_all, lasp_core.erl:331-364, 765-825), resident waiters against a
laspj_lvar_etf_threshold call per waiter.  l and r are 10,000-element OR-Sets sharing half
their elements (tools/lvar_probe.py's pair); out is their intersection; every threshold is
{strict, Value} of out's own current value, so it is unmet when registered and all its terms
are known.  Legs, timed in this one process after a warm-up with a host clock around the C
calls:

  (a) laspj_lvar_recheck over 16 waiters (none met: the value has not changed);
  (b) the path it replaces, on a twin: 16 calls of laspj_lvar_etf_threshold with the same
      images;
  (c) laspj_lvar_intersection_recheck after an add on a shared element, 16 waiters
      registered on the value before it: ends WRITTEN, all 16 fire;
  (d) the same step on a twin by laspj_lvar_intersection, then laspj_lvar_recheck;
  (e) laspj_lvar_intersection alone on a third variable over the same l and r (no waiters:
      the bind's tail is null).

(c), (d) and (e) run on the same values, one after the other, every round; the waiters are
registered off the clock, which also brings the namespace's images up to the round's add, so
none of the three pays for that.  (d)'s waiters are registered after (c)'s have fired, so 16
waiter lists are live at a time.  A fired waiter's list goes back to the context's block
cache; when that is full the release is a hipFree instead (some 60 us a list), which shows
in the 90th percentiles of (c) and (d) alike and is the cache's cost, not the check's.
Medians with the 10th and 90th percentiles.  The last line is JSON; the report is also
written to profiles/lvar_waiter_probe.txt (or --out PATH).

    python tools/lvar_waiter_probe.py [rounds] [--out PATH]
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from lasp_amd import engine  # noqa: E402
from lasp_amd._lib import check  # noqa: E402
from lasp_amd.terms import Atom  # noqa: E402
from lvar_probe import HALF, N, pair, stats_us, update  # noqa: E402

W = 16
WRITTEN = 1


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.st, self.vd, self.res = C.c_int32(), C.c_int32(), C.c_int32()
        self.ids = (C.c_uint64 * W)()
        self.nmet, self.left = C.c_uint32(), C.c_uint32()

    def ok(self, what):
        if self.vd.value != 0:
            raise RuntimeError(f"probe: {what} fell back")

    def recheck(self, out):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_recheck(out.h, self.ids, W, C.byref(self.nmet),
                                        C.byref(self.left), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        self.ok("lvar_recheck")
        return t, self.nmet.value

    def thresholds(self, out, img):
        met = 0
        t0 = time.perf_counter()
        for _ in range(W):
            check(self.L.laspj_lvar_etf_threshold(out.h, img, len(img), 1, C.byref(self.res),
                                                  C.byref(self.vd)), self.ctx.h)
            met += self.res.value
        t = time.perf_counter() - t0
        self.ok("lvar_etf_threshold")
        return t, met

    def rerun(self, out, l, r):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_intersection(out.h, l.h, r.h, C.byref(self.st),
                                             C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        self.ok("lvar_intersection")
        return t, self.st.value

    def fused(self, out, l, r):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_intersection_recheck(out.h, l.h, r.h, C.byref(self.st),
                                                     self.ids, W, C.byref(self.nmet),
                                                     C.byref(self.left), C.byref(self.vd)),
              self.ctx.h)
        t = time.perf_counter() - t0
        self.ok("lvar_intersection_recheck")
        return t, self.st.value, self.nmet.value


def register(out, img):
    for k in range(W):
        if out.wait(img, True, k + 1) != (0, False):
            raise RuntimeError("probe: {strict, Value} of the value itself was met")


def main():
    argv = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "lvar_waiter_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    warm = 30
    ctx = engine.Context(0)
    T = Timed(ctx)
    l, r = pair(ctx)
    out_c, out_d, out_e = ctx.list_var(l), ctx.list_var(l), ctx.list_var(l)
    for out in (out_c, out_d, out_e):
        if T.rerun(out, l, r)[1] != WRITTEN:
            raise RuntimeError("probe: the first re-run answered wrongly")
    # (a), (b): nothing changes between the rounds
    img = out_c.read()[1]
    register(out_c, img)
    ta, tb_ = [], []
    for k in range(warm + rounds):
        t1, nmet = T.recheck(out_c)
        t2, met = T.thresholds(out_d, img)
        if nmet or met or T.left.value != W:
            raise RuntimeError("probe: an unmet threshold was answered met")
        if k >= warm:
            ta.append(t1)
            tb_.append(t2)
    s0 = ctx.nif_stats()["device_passes"]
    T.recheck(out_c)
    passes_a = ctx.nif_stats()["device_passes"] - s0
    s0 = ctx.nif_stats()["device_passes"]
    T.thresholds(out_d, img)
    passes_b = ctx.nif_stats()["device_passes"] - s0
    for k in range(W):
        out_c.cancel(k + 1)
    # (c), (d), (e): one add on a shared element per round
    tc, td, tdr, te = [], [], [], []
    passes_c = passes_d = 0
    for k in range(warm + rounds):
        update(l, (Atom("add"), HALF + (7 * k) % HALF))
        img = out_c.read()[1]
        register(out_c, img)
        s0 = ctx.nif_stats()["device_passes"]
        t1, st_c, n_c = T.fused(out_c, l, r)
        passes_c = ctx.nif_stats()["device_passes"] - s0
        register(out_d, img)
        s1 = ctx.nif_stats()["device_passes"]
        t2, st_d = T.rerun(out_d, l, r)
        t3, n_d = T.recheck(out_d)
        s2 = ctx.nif_stats()["device_passes"]
        t4, st_e = T.rerun(out_e, l, r)
        if not (st_c == st_d == st_e == WRITTEN) or (n_c, n_d) != (W, W):
            raise RuntimeError("probe: a re-run after a shared element's add did not fire all")
        passes_d = s2 - s1
        if k >= warm:
            tc.append(t1)
            td.append(t2 + t3)
            tdr.append(t3)
            te.append(t4)
    if not (out_c.read()[1] == out_d.read()[1] == out_e.read()[1]):
        raise RuntimeError("probe: the paths' outputs differ")
    counts = out_c.counts()
    fallbacks = ctx.nif_stats()["fallbacks"]
    ctx.close()
    res = {"rounds": rounds, "elements": N, "waiters": W, "out_entries": counts[0],
           "out_tokens": counts[1], "a_recheck": stats_us(ta), "b_thresholds": stats_us(tb_),
           "c_fused": stats_us(tc), "d_two_calls": stats_us(td), "d_recheck_alone": stats_us(tdr),
           "e_intersection": stats_us(te),
           "passes": {"a": passes_a, "b": passes_b, "c": passes_c, "d": passes_d},
           "fallbacks": fallbacks}
    res["b_p10_over_a"] = round(res["b_thresholds"]["p10_us"] / res["a_recheck"]["median_us"], 2)
    res["d_over_c"] = round(res["d_two_calls"]["median_us"] / res["c_fused"]["median_us"], 2)
    line = lambda name, s: (f"{name:<66} {s['median_us']:>10} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    text = "\n".join([
        f"lvar_waiter_probe: l, r of {N} elements sharing {HALF}, {W} waiters {{strict, Value}}, "
        f"{rounds} rounds, medians; out ends with {counts[0]} entries, {counts[1]} tokens",
        line(f"(a) laspj_lvar_recheck, {W} waiters, none met", res["a_recheck"]),
        line(f"(b) {W} x laspj_lvar_etf_threshold, the same images", res["b_thresholds"]),
        line(f"(c) laspj_lvar_intersection_recheck: WRITTEN, {W} fire", res["c_fused"]),
        line("(d) laspj_lvar_intersection + laspj_lvar_recheck", res["d_two_calls"]),
        line(f"    the recheck alone ({W} fire)", res["d_recheck_alone"]),
        line("(e) laspj_lvar_intersection alone (null tail)", res["e_intersection"]),
        f"device passes: (a) {passes_a}  (b) {passes_b}  (c) {passes_c}  (d) {passes_d}",
        f"b.p10 / a = {res['b_p10_over_a']}    d / c = {res['d_over_c']}",
        json.dumps(res)])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
