"""What one re-run of an OR-Set intersection process costs at the drop-in boundary
(lasp_process.erl:61-95, lasp_core.erl:559-568, 583, 291-312), resident against the image
path.  l and r are 10,000-element OR-Sets sharing half their elements, one or two tokens per
element; every step one {add, E} of a known element on l.  Legs, timed in this one process
after a warm-up with a host clock around the C calls; (a), (c) and (e) run on the same
values, one after the other, every round:

  (a) laspj_lvar_intersection after an add on a shared element: ends WRITTEN;
  (b) the same after an add on an element r does not hold (a second pair of variables whose
      output is exactly AccValue): ends NOOP;
  (c) today's path: laspj_var_etf_read(l) + laspj_var_etf_read(r) +
      laspj_list_etf_intersection + laspj_list_etf_bind against out's image — the C calls
      only; copying the images between the calls is left out, in (c)'s favour;
  (d) a step that adds a never-seen element to l: the update (which rebuilds the namespace's
      images) and the re-run (which derives the order tables again), and the re-run alone;
  (e) (a) with the two-step composition in place of the fused producer
      (LASPJ_TUNE_LVAR_PRODUCER = 1: laspj_list_from_set + laspj_list_intersection_set).

Medians with the 10th and 90th percentiles.  The last line is JSON; the report is also
written to profiles/lvar_probe.txt (or --out PATH).

    python tools/lvar_probe.py [rounds] [--out PATH]
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
HALF = N // 2
NOOP, WRITTEN = 0, 1


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


def pair(ctx):
    """l = 0 .. N-1, r = N/2 .. 3N/2-1, every other element with a second token."""
    l = ctx.var("orset")
    r = l.replica()
    update(l, (Atom("add_all"), list(range(N))))
    update(r, (Atom("add_all"), list(range(HALF, HALF + N))))
    update(l, (Atom("add_all"), list(range(0, N, 2))))
    update(r, (Atom("add_all"), list(range(HALF, HALF + N, 2))))
    return l, r


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.st, self.vd = C.c_int32(), C.c_int32()
        self.out, self.olen = C.c_void_p(), C.c_uint64()

    def rerun(self, out, l, r):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_intersection(out.h, l.h, r.h, C.byref(self.st),
                                             C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: lvar_intersection fell back")
        return t, self.st.value

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
    path = os.path.join(ROOT, "profiles", "lvar_probe.txt")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
    rounds = int(argv[0]) if argv else 300
    warm = 30
    ctx = engine.Context(0)
    L, T = ctx.L, Timed(ctx)
    l, r = pair(ctx)
    out, out_e = ctx.list_var(l), ctx.list_var(l)
    cimg = tb([])
    l2, r2 = pair(ctx)
    out2 = ctx.list_var(l2)
    if T.rerun(out2, l2, r2)[1] != WRITTEN:
        raise RuntimeError("probe: the first re-run answered wrongly")
    ta, tb_, tc, te = [], [], [], []
    for k in range(warm + rounds):
        update(l, (Atom("add"), HALF + (7 * k) % HALF))
        # (a)
        t, st_a = T.rerun(out, l, r)
        # (c) on the same values
        t1, limg = T.image(L.laspj_var_etf_read, l.h)
        t2, rimg = T.image(L.laspj_var_etf_read, r.h)
        t3, acc = T.image(L.laspj_list_etf_intersection, ctx.h, _lib.KIND_ORSET, limg, len(limg),
                          rimg, len(rimg))
        t0 = time.perf_counter()
        check(L.laspj_list_etf_bind(ctx.h, _lib.KIND_ORSET, cimg, len(cimg), acc, len(acc),
                                    C.byref(T.out), C.byref(T.olen), C.byref(T.st),
                                    C.byref(T.vd)), ctx.h)
        t4 = time.perf_counter() - t0
        if T.vd.value != 0 or T.st.value != st_a:
            raise RuntimeError("probe: the two paths answered differently")
        if T.st.value == WRITTEN:
            cimg = C.string_at(T.out, T.olen.value)
        # (e) the composition, on the same values
        ctx.set_tuning(_lib.TUNE_LVAR_PRODUCER, 1)
        t5, st_e = T.rerun(out_e, l, r)
        ctx.set_tuning(_lib.TUNE_LVAR_PRODUCER, 0)
        if st_e != st_a or st_a != WRITTEN:
            raise RuntimeError("probe: a re-run after a shared element's add was not WRITTEN")
        # (b)
        update(l2, (Atom("add"), (7 * k) % HALF))
        t6, st_b = T.rerun(out2, l2, r2)
        if st_b != NOOP:
            raise RuntimeError("probe: a re-run with AccValue unchanged was not NOOP")
        if k >= warm:
            ta.append(t)
            tc.append(t1 + t2 + t3 + t4)
            te.append(t5)
            tb_.append(t6)
    if not (out.read()[1] == out_e.read()[1] == cimg):
        raise RuntimeError("probe: the paths' outputs differ")
    # (d): a never-seen element per step
    td, tdr = [], []
    for k in range(warm + rounds):
        op = tb((Atom("add"), 2 * N + k))
        res, vd = C.c_int32(), C.c_int32()
        t0 = time.perf_counter()
        check(L.laspj_var_etf_update(l.h, op, len(op), C.byref(res), None, None, None, None,
                                     C.byref(vd)), ctx.h)
        t1 = time.perf_counter()
        _t, st = T.rerun(out, l, r)
        t2 = time.perf_counter()
        if (vd.value, res.value) != (0, 0):
            raise RuntimeError("probe: update fell back")
        if k >= warm:
            td.append(t2 - t0)
            tdr.append(t2 - t1)
    stats = ctx.nif_stats()
    counts = out.counts()
    ctx.close()
    res = {"rounds": rounds, "elements": N, "out_entries": counts[0], "out_tokens": counts[1],
           "a_written": stats_us(ta), "b_noop": stats_us(tb_), "c_image_path": stats_us(tc),
           "d_new_element_update_and_rerun": stats_us(td), "d_rerun_alone": stats_us(tdr),
           "e_composition": stats_us(te), "fallbacks": stats["fallbacks"],
           "image_rebuilds": stats["image_rebuilds"], "image_patches": stats["image_patches"]}
    res["c_p10_over_a"] = round(res["c_image_path"]["p10_us"] / res["a_written"]["median_us"], 2)
    res["e_over_a"] = round(res["e_composition"]["median_us"] / res["a_written"]["median_us"], 2)
    line = lambda name, s: (f"{name:<62} {s['median_us']:>10} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    text = "\n".join([
        f"lvar_probe: l, r of {N} elements sharing {HALF}, 1-2 tokens each, {rounds} rounds, "
        f"medians; out ends with {counts[0]} entries, {counts[1]} tokens",
        line("(a) laspj_lvar_intersection, a shared element re-added: WRITTEN", res["a_written"]),
        line("(b) laspj_lvar_intersection, AccValue unchanged: NOOP", res["b_noop"]),
        line("(c) 2 x etf_read + list_etf_intersection + list_etf_bind", res["c_image_path"]),
        line("(d) a never-seen element: update + re-run", res["d_new_element_update_and_rerun"]),
        line("    the re-run alone (tables derived again)", res["d_rerun_alone"]),
        line("(e) (a) by from_set + intersection_set", res["e_composition"]),
        f"c.p10 / a = {res['c_p10_over_a']}    e / a = {res['e_over_a']}",
        json.dumps(res)])
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
