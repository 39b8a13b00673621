"""What one re-run of a map/6 process costs at the drop-in boundary (lasp_process.erl:61-95,
lasp_core.erl:641-667, 291-312), resident against the image path.  `in` is a 10,000-element
OR-Set, one or two tokens per element; F = X + 1,000,000.  Legs, timed in this one process
after a warm-up with a host clock around the C calls; (a) and (b) run on the same value, (d) on
an equal one in a namespace of its own, one after the other, every round:

  (a) laspj_map_run after an {add, E} of a known element: ends WRITTEN;
  (b) today's path on the same value: laspj_var_etf_read(in) + laspj_list_etf_args +
      laspj_list_etf_map + laspj_list_etf_bind against out's image — the C calls only;
      calling the fun and copying the images between the calls are left out, in (b)'s favour;
  (c) a step that adds a never-seen element: run (pending 1), args, results, run — the fun
      off the clock;
  (d) (a) with F = X div 2 (two inputs per key, keys that are input elements too); its
      statuses are counted, as bind/3 refuses many merges of lists with repeated keys.

Medians with the 10th and 90th percentiles.  At the end (a)'s and (b)'s outputs are compared
byte for byte.  The last line is JSON; the report is also written to profiles/map_probe.txt
(or --out PATH).

    python tools/map_probe.py [rounds] [--out PATH]
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
SHIFT = 1000000
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


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.st, self.vd, self.pend = C.c_int32(), C.c_int32(), C.c_uint32()
        self.out, self.olen, self.cnt = C.c_void_p(), C.c_uint64(), C.c_uint32()

    def run(self, m):
        t0 = time.perf_counter()
        check(self.L.laspj_map_run(m.h, C.byref(self.st), C.byref(self.pend),
                                   C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: map_run fell back")
        return t, self.st.value, self.pend.value

    def args(self, m):
        t0 = time.perf_counter()
        check(self.L.laspj_map_args(m.h, C.byref(self.out), C.byref(self.olen),
                                    C.byref(self.cnt), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: map_args fell back")
        return t, C.string_at(self.out, self.olen.value)

    def results(self, m, img):
        t0 = time.perf_counter()
        check(self.L.laspj_map_results(m.h, img, len(img), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: the map was refused")
        return t

    def image(self, fn, *args):
        """An image-answering call: (seconds, a copy of the answer taken off the clock)."""
        t0 = time.perf_counter()
        check(fn(*args, C.byref(self.out), C.byref(self.olen), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: an image call fell back")
        return t, C.string_at(self.out, self.olen.value)


def main():
    argv = sys.argv[1:]
    path = os.path.join(ROOT, "profiles", "map_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    warm = 30
    ctx = engine.Context(0)
    L, T = ctx.L, Timed(ctx)
    inv = ctx.var("orset")
    update(inv, (Atom("add_all"), list(range(N))))
    update(inv, (Atom("add_all"), list(range(0, N, 2))))
    # (d)'s variables in a namespace of their own: its keys are input elements too, and what
    # it registers under them would be (a)'s map's to name as well
    inv_d = ctx.var("orset")
    update(inv_d, (Atom("add_all"), list(range(N))))
    update(inv_d, (Atom("add_all"), list(range(0, N, 2))))
    out, out_d = ctx.list_var(inv), ctx.list_var(inv_d)
    ma, md = ctx.map(inv, out), ctx.map(inv_d, out_d)
    if ma.step(lambda x: x + SHIFT)[:2] != (0, WRITTEN):
        raise RuntimeError("probe: the first re-run answered wrongly")
    if md.step(lambda x: x // 2)[:2] != (0, WRITTEN):
        raise RuntimeError("probe: the first X div 2 re-run answered wrongly")
    cimg = out.read()[1]
    ta, tb_, td = [], [], []
    d_status = {NOOP: 0, WRITTEN: 0, REFUSED: 0}
    for k in range(warm + rounds):
        update(inv, (Atom("add"), (7 * k + 3) % N))
        # (a)
        t, st_a, pend = T.run(ma)
        if (st_a, pend) != (WRITTEN, 0):
            raise RuntimeError("probe: a re-run after a known element's add was not WRITTEN")
        # (d) after the same add
        update(inv_d, (Atom("add"), (7 * k + 3) % N))
        t5, st_d, pend = T.run(md)
        if pend:
            raise RuntimeError("probe: the X div 2 re-run reported pending elements")
        # (b) on the same value
        t1, vimg = T.image(L.laspj_var_etf_read, inv.h)
        t2, aimg = T.image(L.laspj_list_etf_args, ctx.h, _lib.KIND_ORSET, vimg, len(vimg))
        rimg = tb([a + SHIFT for a in etf.binary_to_term(aimg)])
        t3, acc = T.image(L.laspj_list_etf_map, ctx.h, _lib.KIND_ORSET, vimg, len(vimg), rimg,
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
            td.append(t5)
            d_status[st_d] += 1
    if out.read()[1] != cimg:
        raise RuntimeError("probe: the paths' outputs differ")
    # (c): a never-seen element per step
    tc = []
    for k in range(warm + rounds):
        update(inv, (Atom("add"), 2 * N + k))
        t1, st, pend = T.run(ma)
        if pend != 1:
            raise RuntimeError("probe: a never-seen element was not the one pending")
        t2, aimg = T.args(ma)
        rimg = tb([a + SHIFT for a in etf.binary_to_term(aimg)])
        t3 = T.results(ma, rimg)
        t4, st, pend = T.run(ma)
        if (st, pend) != (WRITTEN, 0):
            raise RuntimeError("probe: the re-run after results was not WRITTEN")
        if k >= warm:
            tc.append(t1 + t2 + t3 + t4)
    stats = ctx.nif_stats()
    counts = out.counts()
    ctx.close()
    res = {"rounds": rounds, "elements": N, "out_entries": counts[0], "out_tokens": counts[1],
           "a_written": stats_us(ta), "b_image_path": stats_us(tb_),
           "c_new_element": stats_us(tc), "d_div2": stats_us(td),
           "d_statuses": {"noop": d_status[NOOP], "written": d_status[WRITTEN],
                          "refused": d_status[REFUSED]},
           "fallbacks": stats["fallbacks"], "image_rebuilds": stats["image_rebuilds"],
           "image_patches": stats["image_patches"]}
    res["b_p10_over_a"] = round(res["b_image_path"]["p10_us"] / res["a_written"]["median_us"], 2)
    res["b_p10_over_d"] = round(res["b_image_path"]["p10_us"] / res["d_div2"]["median_us"], 2)
    line = lambda name, s: (f"{name:<62} {s['median_us']:>10} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    text = "\n".join([
        f"map_probe: in of {N} elements, 1-2 tokens each, F = X + {SHIFT}, {rounds} rounds, "
        f"medians; out ends with {counts[0]} entries, {counts[1]} tokens",
        line("(a) laspj_map_run, a known element re-added: WRITTEN", res["a_written"]),
        line("(b) etf_read + list_etf_args + list_etf_map + list_etf_bind", res["b_image_path"]),
        line("(c) a never-seen element: run + args + results + run", res["c_new_element"]),
        line("(d) (a) with F = X div 2", res["d_div2"]),
        f"    (d) statuses: {res['d_statuses']}",
        f"b.p10 / a = {res['b_p10_over_a']}    b.p10 / d = {res['b_p10_over_d']}",
        json.dumps(res)])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
