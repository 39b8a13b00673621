"""What one re-run of an OR-Set product process costs at the drop-in boundary
(lasp_process.erl:61-95, lasp_core.erl:499-533, 291-312), resident against the image path.
l and r are OR-Sets of n distinct elements each (300 and 1000), one token per element or two;
every step one {add, E} of a known element on l.  Legs, timed in this one process after a
warm-up with a host clock around the C calls; (a) and (c) run on the same values, one after the
other, every round:

  (a) laspj_lvar_product after the add: ends WRITTEN;
  (b) the same with nothing changed, into a second output that holds exactly AccValue: NOOP;
  (c) today's path: laspj_var_etf_read(l) + laspj_var_etf_read(r) + laspj_list_etf_product +
      laspj_list_etf_bind against out's image — the C calls only; copying the images between
      the calls is left out, in (c)'s favour;
  (d) (a) split by laspj_nif_stats' nanosecond counters: [8] the producer (side pass, the size
      synchronisation, the output's reservation, the write pass enqueued) and [9] the bind
      (which also waits for the write pass);
  (w) the write pass alone: its bytes (12 per entry + 8 per token) over its kernel time, taken
      from a kernel trace of this program (--trace runs leg (a) alone; run it as
      `rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/lvar_product_probe.py
      --trace`, then pass the trace to the full run with --kernel-trace FILE), against the
      store rate of the plain copy stream (laspj_orset_precondition_context, 1R:1W, HIP
      events) writing the same byte count on this box.

Medians with the 10th and 90th percentiles.  The last line is JSON; the report is also written
to profiles/lvar_product_probe.txt (or --out PATH).

    python tools/lvar_product_probe.py [--rounds-small N] [--rounds-large N] [--out PATH]
                                       [--kernel-trace FILE] [--trace]
"""
import csv
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

NOOP, WRITTEN = 0, 1
SHAPES = [(300, 1), (300, 2), (1000, 1), (1000, 2)]


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


def pair(ctx, n, ntok):
    """l = 0 .. n-1 and r = n .. 2n-1, ntok tokens per element."""
    l = ctx.var("orset")
    r = l.replica()
    for _ in range(ntok):
        update(l, (Atom("add_all"), list(range(n))))
        update(r, (Atom("add_all"), list(range(n, 2 * n))))
    return l, r


class Timed:
    def __init__(self, ctx):
        self.ctx, self.L = ctx, ctx.L
        self.st, self.vd = C.c_int32(), C.c_int32()
        self.out, self.olen = C.c_void_p(), C.c_uint64()

    def rerun(self, out, l, r):
        t0 = time.perf_counter()
        check(self.L.laspj_lvar_product(out.h, l.h, r.h, C.byref(self.st), C.byref(self.vd)),
              self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: lvar_product fell back")
        return t, self.st.value

    def image(self, fn, *args):
        """An image-answering call: (seconds, a copy of the answer taken off the clock)."""
        t0 = time.perf_counter()
        check(fn(*args, C.byref(self.out), C.byref(self.olen), C.byref(self.vd)), self.ctx.h)
        t = time.perf_counter() - t0
        if self.vd.value != 0:
            raise RuntimeError("probe: an image call fell back")
        return t, C.string_at(self.out, self.olen.value)


def write_grid(n, ntok, extra_l_tokens):
    """threads of the write pass's grid for this shape (one key / toff word and one token word
    per thread, 256 per block)."""
    tl = n * ntok + extra_l_tokens
    span = max(n * n, tl * n * ntok, 1)
    return (span + 255) // 256 * 256


def trace_only(ctx, rounds):
    """leg (a) alone, for a kernel trace: `rounds` re-runs per shape, each after one add."""
    T = Timed(ctx)
    for n, ntok in SHAPES:
        l, r = pair(ctx, n, ntok)
        out = ctx.pair_list_var(l)
        T.rerun(out, l, r)
        for k in range(rounds):
            update(l, (Atom("add"), (7 * k) % n))
            T.rerun(out, l, r)
        for v in (out, l, r):
            v.close()


def kernel_times(path):
    """{grid threads: [seconds]} of the write pass's dispatches in a rocprofv3 kernel trace."""
    out = {}
    with open(path, newline="") as fh:
        for row in csv.DictReader(fh):
            if "k_lp_write" not in row.get("Kernel_Name", ""):
                continue
            grid = int(row.get("Grid_Size_X") or row.get("Grid_Size") or 0)
            dt = (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) * 1e-9
            out.setdefault(grid, []).append(dt)
    return out


def copy_store_rate(ctx, nbytes):
    """bytes written per second by the plain copy stream (p & ~r of a batch into another)
    writing about nbytes."""
    E = 4096
    R = max(1, nbytes // (16 * E))
    a, c = ctx.orset_batch(R, E), ctx.orset_batch(R, E)
    a.fill_synthetic(2)
    fn = lambda: check(ctx.L.laspj_orset_precondition_context(ctx.h, c.h, a.h), ctx.h)  # noqa: E731
    for _ in range(3):
        fn()
    ctx.synchronize()
    e0, e1 = ctx.event(), ctx.event()
    steps = 20
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    ms = e0.elapsed_ms(e1) / steps
    return 16.0 * R * E / (ms / 1e3), 16 * R * E


def shape(ctx, n, ntok, rounds, warm, ktimes):
    L, T = ctx.L, Timed(ctx)
    l, r = pair(ctx, n, ntok)
    out, out_b = ctx.pair_list_var(l), ctx.pair_list_var(l)
    cimg = tb([])
    ta, tb_, tc, tprod, tbind = [], [], [], [], []
    c_error = None
    for k in range(warm + rounds):
        update(l, (Atom("add"), (7 * k) % n))
        s0 = ctx.nif_stats()
        t, st_a = T.rerun(out, l, r)
        s1 = ctx.nif_stats()
        if st_a != WRITTEN:
            raise RuntimeError("probe: a re-run after an add was not WRITTEN")
        # (c) on the same values
        tcs = None
        if c_error is None:
            try:
                t1, limg = T.image(L.laspj_var_etf_read, l.h)
                t2, rimg = T.image(L.laspj_var_etf_read, r.h)
                t3, acc = T.image(L.laspj_list_etf_product, ctx.h, _lib.KIND_ORSET, limg,
                                  len(limg), rimg, len(rimg))
                t0 = time.perf_counter()
                check(L.laspj_list_etf_bind(ctx.h, _lib.KIND_ORSET, cimg, len(cimg), acc, len(acc),
                                            C.byref(T.out), C.byref(T.olen), C.byref(T.st),
                                            C.byref(T.vd)), ctx.h)
                t4 = time.perf_counter() - t0
                if T.vd.value != 0:
                    raise RuntimeError("list_etf_bind fell back")
                if T.st.value != st_a:
                    raise RuntimeError("probe: the two paths answered differently")
                cimg = C.string_at(T.out, T.olen.value)
                tcs = t1 + t2 + t3 + t4
            except (RuntimeError, _lib.LaspjError) as e:
                if "differently" in str(e):
                    raise
                c_error = str(e)
        # (b): a second output written from [] holds exactly AccValue; the re-run is a no-op
        if out_b.write(tb([])) != 0 or T.rerun(out_b, l, r)[1] != WRITTEN:
            raise RuntimeError("probe: the second output's first re-run answered wrongly")
        t6, st_b = T.rerun(out_b, l, r)
        if st_b != NOOP:
            raise RuntimeError("probe: a re-run with AccValue unchanged was not NOOP")
        if k >= warm:
            ta.append(t)
            tb_.append(t6)
            if tcs is not None:
                tc.append(tcs)
            tprod.append((s1["ns_stage_enqueue"] - s0["ns_stage_enqueue"]) * 1e-9)
            tbind.append((s1["ns_device_wait"] - s0["ns_device_wait"]) * 1e-9)
    if c_error is None and out.read()[1] != cimg:
        raise RuntimeError("probe: the paths' outputs differ")
    counts = out.counts()
    acc_counts = out_b.counts()
    res = {"elements": n, "tokens_per_element": ntok, "rounds": rounds,
           "acc_entries": acc_counts[0], "acc_tokens": acc_counts[1],
           "out_entries": counts[0], "out_tokens": counts[1],
           "a_written": stats_us(ta), "b_noop": stats_us(tb_),
           "c_image_path": stats_us(tc) if tc else None, "c_error": c_error,
           "d_producer": stats_us(tprod), "d_bind": stats_us(tbind)}
    if tc:
        res["c_over_a"] = round(res["c_image_path"]["median_us"] / res["a_written"]["median_us"], 2)
    # (w): the last round's write pass by its grid
    if ktimes is not None:
        grids = [write_grid(n, ntok, k + 1) for k in range(warm + rounds)]
        # (the trace names the grid in threads, or in blocks of 256)
        ts = [t for g in grids for t in ktimes.get(g, []) + ktimes.get(g // 256, [])]
        if ts:
            # (the traced re-runs follow the first adds: l holds about two tokens more)
            nbytes = 12 * n * n + 8 * (n * ntok + 2) * (n * ntok)
            kt = statistics.median(ts)
            rate, copied = copy_store_rate(ctx, nbytes)
            res["w_write_pass"] = {"bytes": nbytes, "kernel_us": round(kt * 1e6, 2),
                                   "GBps": round(nbytes / kt / 1e9, 1),
                                   "copy_stream_store_GBps": round(rate / 1e9, 1),
                                   "copy_stream_bytes_written": copied,
                                   "fraction_of_copy_stream": round(nbytes / kt / rate, 3)}
    for v in (out, out_b, l, r):
        v.close()
    return res


def main():
    argv = sys.argv[1:]

    def opt(name, default):
        if name in argv:
            i = argv.index(name)
            v = argv[i + 1]
            del argv[i:i + 2]
            return v
        return default

    path = opt("--out", os.path.join(ROOT, "profiles", "lvar_product_probe.txt"))
    small, large = int(opt("--rounds-small", 20)), int(opt("--rounds-large", 5))
    trace = opt("--kernel-trace", None)
    ctx = engine.Context(0)
    if "--trace" in argv:
        trace_only(ctx, 3)
        ctx.close()
        return
    ktimes = kernel_times(trace) if trace else None
    results = [shape(ctx, n, ntok, small if n <= 300 else large, 2, ktimes) for n, ntok in SHAPES]
    fallbacks = ctx.nif_stats()["fallbacks"]
    ctx.close()
    res = {"shapes": results, "fallbacks": fallbacks}
    line = lambda name, s: (f"  {name:<60} {s['median_us']:>12} us  "  # noqa: E731
                            f"(p10 {s['p10_us']}, p90 {s['p90_us']})")
    text = ["lvar_product_probe: l x r of n elements each, one {add, E} on l per round, medians"]
    for s in results:
        text.append(f"n = {s['elements']}, {s['tokens_per_element']} token(s) per element, "
                    f"{s['rounds']} rounds; AccValue {s['acc_entries']} entries, "
                    f"{s['acc_tokens']} tokens; out ends with {s['out_entries']} entries, "
                    f"{s['out_tokens']} tokens")
        text.append(line("(a) laspj_lvar_product after an add: WRITTEN", s["a_written"]))
        text.append(line("(b) laspj_lvar_product, nothing changed: NOOP", s["b_noop"]))
        if s["c_image_path"]:
            text.append(line("(c) 2 x etf_read + list_etf_product + list_etf_bind",
                             s["c_image_path"]))
            text.append(f"  c / a = {s['c_over_a']}")
        else:
            text.append(f"  (c) did not run: {s['c_error']}")
        text.append(line("(d) of (a): the producer (nif_stats [8])", s["d_producer"]))
        text.append(line("    of (a): the bind (nif_stats [9])", s["d_bind"]))
        w = s.get("w_write_pass")
        if w:
            text.append(f"  (w) write pass: {w['bytes']} B in {w['kernel_us']} us = {w['GBps']} GB/s; "
                        f"copy stream writing {w['copy_stream_bytes_written']} B: "
                        f"{w['copy_stream_store_GBps']} GB/s stored; fraction "
                        f"{w['fraction_of_copy_stream']}")
    text.append(json.dumps(res))
    text = "\n".join(text)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as fh:
        fh.write(text + "\n")


if __name__ == "__main__":
    main()
