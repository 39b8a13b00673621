"""What one re-run of a fold/6 process costs at the drop-in boundary (lasp_process.erl:61-95,
lasp_core.erl:460-486, 291-312), resident against the image path.  `in` is a 10,000-element
OR-Set, one or two tokens per element.  Legs, timed in this one process after a warm-up with
a host clock around the C calls, one after the other every round; every step is one {add, E}
of a known element:

  (a) laspj_fold_run with F = [X + 1,000,000, X + 2,000,000]: ends WRITTEN;
  (b) the parent's only route on the same value: laspj_var_etf_read(in) + laspj_list_etf_args
      + laspj_list_etf_fold + laspj_list_etf_bind against out's image — the C calls only;
      calling the fun and copying the images between the calls are left out, in (b)'s favour;
  (c) (a) with fan-out 1, F = [X + 3,000,000], beside laspj_map_run with X + 4,000,000 over
      the same variable: what the generalisation costs over the map.  Whichever of the two
      runs first after the add also brings the namespace's images and rank rows up to the
      input's new token, so the order alternates and the legs are reported per place;
  (d) skew: one element with 8,192 outputs and the rest with none, beside 8,192 elements of
      one output each — equal output sizes, each in a namespace of its own; the step re-adds
      an element without outputs, so both legs run the whole producer and the bind (NOOP)
      with equal host work and differ only in how the writer's entries lie;
  (e) a step that adds a never-seen element to (a)'s input: run (pending 1), args, results,
      run — the fun off the clock.

Medians with the 10th and 90th percentiles.  At the end (a)'s and (b)'s outputs are compared
byte for byte.  The last line is JSON; the report is also written to profiles/fold_probe.txt
(or --out PATH).

    python tools/fold_probe.py [rounds] [--out PATH]
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

N = 10000
WIDE = 8192
M = 1000000
NOOP, WRITTEN, REFUSED = 0, 1, 2


def tb(t):
    return etf.term_to_binary(t)


def stats_us(xs):
    xs = sorted(xs)
    q = lambda p: xs[min(len(xs) - 1, int(p * len(xs)))]  # noqa: E731
    return {"median_us": round(statistics.median(xs) * 1e6, 2),
            "p10_us": round(q(0.10) * 1e6, 2), "p90_us": round(q(0.90) * 1e6, 2)}


def update(var, op):
    if var.update(tb(op))[:2] != (0, 0):
        raise RuntimeError("probe: update fell back")


def fun_a(x):
    return [x + M, x + 2 * M]


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.st, self.vd, self.pend = C.c_int32(), C.c_int32(), C.c_uint32()
        self.out, self.olen, self.cnt = C.c_void_p(), C.c_uint64(), C.c_uint32()

    def run(self, p, fn=None):
        fn = fn or self.L.laspj_fold_run
        t0 = time.perf_counter()
        check(fn(p.h, C.byref(self.st), C.byref(self.pend), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: a run fell back")
        return t, self.st.value, self.pend.value

    def args(self, p):
        t0 = time.perf_counter()
        check(self.L.laspj_fold_args(p.h, C.byref(self.out), C.byref(self.olen),
                                     C.byref(self.cnt), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: fold_args fell back")
        return t, C.string_at(self.out, self.olen.value)

    def results(self, p, img):
        t0 = time.perf_counter()
        check(self.L.laspj_fold_results(p.h, img, len(img), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: the fold was refused")
        return t

    def image(self, fn, *args):
        """An image-answering call: (seconds, a copy of the answer taken off the clock)."""
        t0 = time.perf_counter()
        check(fn(*args, C.byref(self.out), C.byref(self.olen), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: an image call fell back")
        return t, C.string_at(self.out, self.olen.value)


def filled(ctx):
    v = ctx.var("orset")
    update(v, (Atom("add_all"), list(range(N))))
    update(v, (Atom("add_all"), list(range(0, N, 2))))
    return v


def main():
    argv = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "fold_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    warm = 30
    ctx = engine.Context(0)
    L, T = ctx.L, Timed(ctx)
    inv, inv_c, inv_s, inv_u = filled(ctx), filled(ctx), filled(ctx), filled(ctx)
    out = ctx.list_var(inv)
    out_cf, out_cm = ctx.list_var(inv_c), ctx.list_var(inv_c)
    out_s, out_u = ctx.list_var(inv_s), ctx.list_var(inv_u)
    fa = ctx.fold(inv, out)
    fc, mc = ctx.fold(inv_c, out_cf), ctx.map(inv_c, out_cm)
    fs, fu = ctx.fold(inv_s, out_s), ctx.fold(inv_u, out_u)
    first = [fa.step(fun_a), fc.step(lambda x: [x + 3 * M]), mc.step(lambda x: x + 4 * M),
             fs.step(lambda x: [5 * M + i for i in range(WIDE)] if x == 0 else []),
             fu.step(lambda x: [x + 6 * M] if x < WIDE else [])]
    if any(r[:2] != (0, WRITTEN) for r in first):
        raise RuntimeError("probe: a first re-run answered wrongly")
    if out_s.counts()[0] != WIDE or out_u.counts()[0] != WIDE:
        raise RuntimeError("probe: the skew legs' outputs are not of one size")
    cimg = out.read()[1]
    ta, tb_, ts, tu = [], [], [], []
    tcf, tcm = ([], []), ([], [])                        # [0]: ran first after the add
    for k in range(warm + rounds):
        e = (7 * k + 3) % N
        update(inv, (Atom("add"), e))
        # (a)
        t, st_a, pend = T.run(fa)
        if (st_a, pend) != (WRITTEN, 0):
            raise RuntimeError("probe: a re-run after a known element's add was not WRITTEN")
        # (c) after the same add
        update(inv_c, (Atom("add"), e))
        if k % 2 == 0:
            t5, st, pend = T.run(fc)
            t6, st2, pend2 = T.run(mc, L.laspj_map_run)
        else:
            t6, st2, pend2 = T.run(mc, L.laspj_map_run)
            t5, st, pend = T.run(fc)
        if (st, pend, st2, pend2) != (WRITTEN, 0, WRITTEN, 0):
            raise RuntimeError("probe: (c)'s re-runs were not WRITTEN")
        # (d): an element without outputs in both legs
        e0 = WIDE + (7 * k + 3) % (N - WIDE)
        update(inv_s, (Atom("add"), e0))
        update(inv_u, (Atom("add"), e0))
        t7, st, pend = T.run(fs)
        t8, st2, pend2 = T.run(fu)
        if (st, pend, st2, pend2) != (NOOP, 0, NOOP, 0):
            raise RuntimeError("probe: (d)'s re-runs were not NOOP")
        # (b) on (a)'s value
        t1, vimg = T.image(L.laspj_var_etf_read, inv.h)
        t2, aimg = T.image(L.laspj_list_etf_args, ctx.h, _lib.KIND_ORSET, vimg, len(vimg))
        rimg = tb([fun_a(a) for a in etf.binary_to_term(aimg)])
        t3, acc = T.image(L.laspj_list_etf_fold, ctx.h, _lib.KIND_ORSET, vimg, len(vimg), rimg,
                          len(rimg))
        t0 = time.perf_counter()
        check(L.laspj_list_etf_bind(ctx.h, _lib.KIND_ORSET, cimg, len(cimg), acc, len(acc),
                                    C.byref(T.out), C.byref(T.olen), C.byref(T.st),
                                    C.byref(T.vd)), ctx.h)
        t4 = time.perf_counter() - t0
        if T.vd.value != 0 or T.st.value != st_a:
            raise RuntimeError("probe: the two paths answered differently")
        cimg = C.string_at(T.out, T.olen.value)
        if k >= warm:
            ta.append(t)
            tb_.append(t1 + t2 + t3 + t4)
            tcf[k % 2].append(t5)
            tcm[1 - k % 2].append(t6)
            ts.append(t7)
            tu.append(t8)
    if out.read()[1] != cimg:
        raise RuntimeError("probe: the paths' outputs differ")
    # (e): a never-seen element per step
    te = []
    for k in range(warm + rounds):
        update(inv, (Atom("add"), 2 * N + k))
        t1, st, pend = T.run(fa)
        if pend != 1:
            raise RuntimeError("probe: a never-seen element was not the one pending")
        t2, aimg = T.args(fa)
        rimg = tb([fun_a(a) for a in etf.binary_to_term(aimg)])
        t3 = T.results(fa, rimg)
        t4, st, pend = T.run(fa)
        if (st, pend) != (WRITTEN, 0):
            raise RuntimeError("probe: the re-run after results was not WRITTEN")
        if k >= warm:
            te.append(t1 + t2 + t3 + t4)
    stats = ctx.nif_stats()
    counts = out.counts()
    ctx.close()
    res = {"rounds": rounds, "elements": N, "out_entries": counts[0], "out_tokens": counts[1],
           "a_written": stats_us(ta), "b_image_path": stats_us(tb_),
           "c_fold_first": stats_us(tcf[0]), "c_map_second": stats_us(tcm[1]),
           "c_map_first": stats_us(tcm[0]), "c_fold_second": stats_us(tcf[1]),
           "d_skewed": stats_us(ts), "d_uniform": stats_us(tu),
           "e_new_element": stats_us(te),
           "fallbacks": stats["fallbacks"], "image_rebuilds": stats["image_rebuilds"],
           "image_patches": stats["image_patches"]}
    res["b_p10_over_a"] = round(res["b_image_path"]["p10_us"] / res["a_written"]["median_us"], 2)
    res["c_fold_over_map_first"] = round(res["c_fold_first"]["median_us"] /
                                         res["c_map_first"]["median_us"], 2)
    res["c_fold_over_map_second"] = round(res["c_fold_second"]["median_us"] /
                                          res["c_map_second"]["median_us"], 2)
    res["d_skewed_over_uniform"] = round(res["d_skewed"]["median_us"] /
                                         res["d_uniform"]["median_us"], 2)
    line = lambda name, s: (f"{name:<66} {s['median_us']:>10} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    text = "\n".join([
        f"fold_probe: in of {N} elements, 1-2 tokens each, {rounds} rounds, medians; (a)'s out "
        f"ends with {counts[0]} entries, {counts[1]} tokens",
        line("(a) laspj_fold_run, F = [X+1e6, X+2e6], a known element re-added", res["a_written"]),
        line("(b) etf_read + list_etf_args + list_etf_fold + list_etf_bind", res["b_image_path"]),
        line("(c) laspj_fold_run, fan-out 1, first after the add", res["c_fold_first"]),
        line("    laspj_map_run on the same variable, first after the add", res["c_map_first"]),
        line("    laspj_fold_run, second", res["c_fold_second"]),
        line("    laspj_map_run, second", res["c_map_second"]),
        line(f"(d) one element with {WIDE} outputs (re-run ends NOOP)", res["d_skewed"]),
        line(f"    {WIDE} elements with one output each (NOOP)", res["d_uniform"]),
        line("(e) a never-seen element: run + args + results + run", res["e_new_element"]),
        f"b.p10 / a = {res['b_p10_over_a']}    c fold / map = {res['c_fold_over_map_first']} first, "
        f"{res['c_fold_over_map_second']} second    "
        f"d skewed / uniform = {res['d_skewed_over_uniform']}",
        json.dumps(res)])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
