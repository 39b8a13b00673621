"""What the advertisement counter's inner loop and a vnode's queued counter binds cost at
the drop-in boundary (riak_test/lasp_adcounter_test.erl; lasp_core.erl:283-312, 765-825).
Two pairs, each timed in this one process after a warm-up, medians over repeated rounds of a
host clock around calls that end in a device synchronisation:

  (a) laspj_var_etf_increment with the fused re-check on one resident counter of 64 actors
      and 16 waiters, one of which fires per round (one launch, one synchronisation);
  (b) the batch route: laspj_gcounter_apply_increments on a one-replica batch of 64 actor
      slots, then 16 laspj_gcounter_threshold calls, each with its readback (17 launches);

  (c) laspj_var_etf_bind_many over 1024 resident counters of 8 actors, per counter;
  (d) 1024 laspj_var_etf_bind calls over the same counters, per bind.

(a) and (b) alternate round by round, as (c) and (d) do.  The last line is JSON.

    python tools/counter_probe.py [rounds]
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

ACTORS, WAITERS, NVARS = 64, 16, 1024
FAR = 1 << 60


def tb(t):
    return etf.term_to_binary(t)


def med_us(xs):
    return round(statistics.median(xs) * 1e6, 2)


def inner_loop(ctx, rounds, warm):
    L = ctx.L
    var = ctx.var("gcounter")
    if var.bind(tb([(k, 1) for k in range(ACTORS)])) != (0, 1):
        raise RuntimeError("probe: bind fell back")
    for k in range(WAITERS - 1):
        var.wait(tb(FAR + k), False, 100 + k)
    batch = ctx.gcounter_batch(1, ACTORS)
    batch.increment([(0, k, 1) for k in range(ACTORS)])
    flag = ctx.buffer(8)
    op, actor = tb(Atom("increment")), tb(7)
    ids = (C.c_uint64 * WAITERS)()
    nmet, left, vd = C.c_uint32(), C.c_uint32(), C.c_int32()
    inc = (_lib.Incr * 1)()
    inc[0].replica, inc[0].actor, inc[0].amount = 0, 7, 1
    total = ACTORS
    ta, tb_ = [], []
    for r in range(warm + rounds):
        total += 1
        if var.wait(tb(total), False, r) != (0, False):       # the one that fires this round
            raise RuntimeError("probe: the waiter was met early")
        t0 = time.perf_counter()
        check(L.laspj_var_etf_increment(var.h, op, len(op), actor, len(actor), ids, WAITERS,
                                        C.byref(nmet), C.byref(left), C.byref(vd)), ctx.h)
        t1 = time.perf_counter()
        if (vd.value, nmet.value, ids[0], left.value) != (0, 1, r, WAITERS - 1):
            raise RuntimeError("probe: the fused re-check answered wrongly")
        ths = [FAR + k for k in range(WAITERS - 1)] + [total]
        t2 = time.perf_counter()
        check(L.laspj_gcounter_apply_increments(ctx.h, batch.h, inc, 1), ctx.h)
        met = 0
        for t in ths:
            check(L.laspj_gcounter_threshold(ctx.h, batch.h, t, 0, flag.h), ctx.h)
            met += int(flag.download(count=1)[0])
        t3 = time.perf_counter()
        if met != 1:
            raise RuntimeError("probe: the batch route answered wrongly")
        if r >= warm:
            ta.append(t1 - t0)
            tb_.append(t3 - t2)
    return {"a_fused_increment_us": med_us(ta), "b_batch_route_us": med_us(tb_),
            "b_over_a": round(statistics.median(tb_) / statistics.median(ta), 2)}


def many_binds(ctx, rounds, warm):
    L = ctx.L
    vs = [ctx.var("gcounter") for _ in range(NVARS)]
    arr = (C.c_void_p * NVARS)(*[v.h.value for v in vs])
    st, vd = (C.c_int32 * NVARS)(), (C.c_int32 * NVARS)()
    s1, v1 = C.c_int32(), C.c_int32()
    tc, td = [], []
    for r in range(warm + rounds):
        out = {}
        for form in ("many", "single"):
            # every bind raises one count: WRITTEN each time
            base = 2 * r + (form == "single") + 1
            imgs = [tb([(a, base + (a == i % 8)) for a in range(8)]) for i in range(NVARS)]
            pv = (C.c_char_p * NVARS)(*imgs)
            nv = (C.c_uint64 * NVARS)(*[len(x) for x in imgs])
            t0 = time.perf_counter()
            if form == "many":
                check(L.laspj_var_etf_bind_many(ctx.h, NVARS, arr, pv, nv, st, vd), ctx.h)
                ok = all(x == 0 for x in vd) and all(x == 1 for x in st)
            else:
                ok = True
                for i in range(NVARS):
                    check(L.laspj_var_etf_bind(vs[i].h, imgs[i], nv[i], C.byref(s1), C.byref(v1)),
                          ctx.h)
                    ok = ok and (v1.value, s1.value) == (0, 1)
            out[form] = (time.perf_counter() - t0) / NVARS
            if not ok:
                raise RuntimeError("probe: a bind answered wrongly")
        if r >= warm:
            tc.append(out["many"])
            td.append(out["single"])
    return {"c_bind_many_per_counter_us": med_us(tc), "d_single_bind_us": med_us(td),
            "d_over_c": round(statistics.median(td) / statistics.median(tc), 2)}


def main():
    rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 300
    ctx = engine.Context(0)
    res = {"rounds": rounds}
    res.update(inner_loop(ctx, rounds, warm=30))
    s0 = ctx.nif_stats()
    res.update(many_binds(ctx, max(rounds // 10, 10), warm=3))
    s1 = ctx.nif_stats()
    res["fallbacks"] = s1["fallbacks"]
    res["bind_passes"] = s1["device_passes"] - s0["device_passes"]
    ctx.close()
    print(f"(a) fused increment + re-check, {ACTORS} actors, {WAITERS} waiters, 1 fires: "
          f"{res['a_fused_increment_us']} us")
    print(f"(b) apply_increments + {WAITERS} threshold calls with readbacks:        "
          f"{res['b_batch_route_us']} us   (b / a = {res['b_over_a']})")
    print(f"(c) bind_many over {NVARS} counters, per counter: {res['c_bind_many_per_counter_us']} us")
    print(f"(d) {NVARS} single binds, per bind:              {res['d_single_bind_us']} us"
          f"   (d / c = {res['d_over_c']})")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
