"""What a write's re-check of its blocking reads costs (lasp_core.erl:839-844, 765-825), at
the `steady` leg's shape: a 10k-element OR-Set variable and W waiters with distinct
50-element thresholds that stay unmet.  Each step is one {add, E} update followed by either
(a) W sequential laspj_var_etf_threshold calls (one image call per waiter: the parent's
way) or (b) one laspj_var_recheck over the waiters kept on the device; then
laspj_var_recheck_many over 32 variables x 16 waiters after a bind_many.  One JSON line:
medians in microseconds and the host-time split of laspj_nif_stats per device pass ([8]
stage + enqueue, [9] device wait, [10] answers, [13] image patch), for W in {1, 16, 64}.

    python tools/waiters_probe.py [steps]
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

N = 10_000
SPLIT = ("ns_stage_enqueue", "ns_device_wait", "ns_answers", "ns_rebuild")


def tok(tag, e):
    return tag + e.to_bytes(19, "big")


def thresholds(w):
    """W distinct 50-element thresholds, each unmet for good: one token the value never gets"""
    out = []
    for k in range(w):
        es = range(50 * k, 50 * k + 50)
        th = [(e, [(tok(b"A", e), False)]) for e in es]
        th[0] = (es[0], [(tok(b"A", es[0]), False), (tok(b"Z", es[0]), False)])
        out.append(etf.term_to_binary(th))
    return out


def split(ctx, s0, calls):
    s1 = ctx.nif_stats()
    d = {k: (s1[k] - s0[k]) / 1e3 / calls for k in SPLIT}
    d["device_passes"] = (s1["device_passes"] - s0["device_passes"]) / calls
    return {k: round(v, 2) for k, v in d.items()}


def one_variable(ctx, img0, w, steps):
    L = ctx.L
    res, vd, nm = C.c_int32(), C.c_int32(), C.c_uint32()
    ei, el, mi = C.c_void_p(), C.c_uint64(), C.c_void_p()
    ths = thresholds(w)
    ops = [etf.term_to_binary((Atom("add"), (97 * k) % N)) for k in range(steps + 20)]

    def update(var, k):
        check(L.laspj_var_etf_update(var.h, ops[k], len(ops[k]), C.byref(res), C.byref(ei),
                                     C.byref(el), C.byref(mi), C.byref(nm), C.byref(vd)), ctx.h)
        if vd.value != 0:
            raise RuntimeError("probe: update fell back")

    out = {"waiters": w}
    # (a) one image call per waiter
    var = ctx.var("orset")
    if var.write(img0) != 0:
        raise RuntimeError("probe: write fell back")
    each, per_step = [], []
    for k in range(steps + 20):
        if k == 20:
            s0 = ctx.nif_stats()
        update(var, k)
        t_step = 0.0
        for th in ths:
            t0 = time.perf_counter()
            check(L.laspj_var_etf_threshold(var.h, th, len(th), 0, C.byref(res), C.byref(vd)),
                  ctx.h)
            dt = time.perf_counter() - t0
            if vd.value != 0 or res.value != 0:
                raise RuntimeError("probe: threshold answered wrongly")
            t_step += dt
            if k >= 20:
                each.append(dt * 1e6)
        if k >= 20:
            per_step.append(t_step * 1e6)
    out["us_threshold_call_median"] = round(statistics.median(each), 2)
    out["us_threshold_calls_per_step_median"] = round(statistics.median(per_step), 2)
    out["threshold_split_us_per_call"] = split(ctx, s0, steps * w)
    var.close()
    # (b) one re-check of the waiters kept on the device
    var = ctx.var("orset")
    var.write(img0)
    for k, th in enumerate(ths):
        if var.wait(th, False, k) != (0, False):
            raise RuntimeError("probe: wait answered wrongly")
    ids = (C.c_uint64 * w)()
    nmet, left = C.c_uint32(), C.c_uint32()
    ts = []
    for k in range(steps + 20):
        if k == 20:
            s0 = ctx.nif_stats()
        update(var, k)
        t0 = time.perf_counter()
        check(L.laspj_var_recheck(var.h, ids, w, C.byref(nmet), C.byref(left), C.byref(vd)),
              ctx.h)
        dt = time.perf_counter() - t0
        if vd.value != 0 or nmet.value != 0 or left.value != w:
            raise RuntimeError("probe: recheck answered wrongly")
        if k >= 20:
            ts.append(dt * 1e6)
    out["us_recheck_median"] = round(statistics.median(ts), 2)
    out["recheck_split_us"] = split(ctx, s0, steps)
    var.close()
    return out


def many(ctx, img0, imgb, steps):
    L = ctx.L
    nv, w = 32, 16
    vs = [ctx.var("orset") for _ in range(nv)]
    ths = thresholds(w)
    for v in vs:
        v.write(img0)
        for k, th in enumerate(ths):
            if v.wait(th, False, k) != (0, False):
                raise RuntimeError("probe: wait answered wrongly")
    arr_v = (C.c_void_p * nv)(*[v.h.value for v in vs])
    arr_p = (C.c_char_p * nv)(*([imgb] * nv))
    arr_n = (C.c_uint64 * nv)(*([len(imgb)] * nv))
    sts, vds = (C.c_int32 * nv)(), (C.c_int32 * nv)()
    ids, nmet = (C.c_uint64 * (nv * w))(), (C.c_uint32 * nv)()
    tb_, tr = [], []
    for k in range(steps + 3):
        t0 = time.perf_counter()
        check(L.laspj_var_etf_bind_many(ctx.h, nv, arr_v, arr_p, arr_n, sts, vds), ctx.h)
        t1 = time.perf_counter()
        check(L.laspj_var_recheck_many(ctx.h, nv, arr_v, ids, nv * w, nmet, vds), ctx.h)
        t2 = time.perf_counter()
        if any(vds) or any(nmet):
            raise RuntimeError("probe: recheck_many answered wrongly")
        if k >= 3:
            tb_.append((t1 - t0) * 1e6 / nv)
            tr.append((t2 - t1) * 1e6 / nv)
    for v in vs:
        v.close()
    return {"variables": nv, "waiters_each": w,
            "us_bind_many_per_bind_median": round(statistics.median(tb_), 2),
            "us_recheck_many_per_variable_median": round(statistics.median(tr), 2),
            "us_recheck_many_median": round(statistics.median(tr) * nv, 2)}


def main():
    steps = int(sys.argv[1]) if len(sys.argv) > 1 else 200
    ctx = engine.Context(0)
    img0 = etf.term_to_binary([(e, [(tok(b"A", e), False)]) for e in range(N)])
    imgb = etf.term_to_binary([(e, [(tok(b"B", e), e % 10 == 0)]) for e in range(N)])
    out = {"shape": f"{N}-element OR-Set variable, 50-element thresholds, {steps} steps",
           "one_variable": [one_variable(ctx, img0, w, steps) for w in (1, 16, 64)],
           "recheck_many": many(ctx, img0, imgb, 10)}
    r16 = out["one_variable"][1]
    best = r16["us_recheck_median"]
    out["gate_w16"] = {
        "us_recheck": best, "us_one_threshold_call": r16["us_threshold_call_median"],
        "recheck_le_one_threshold_call": best <= r16["us_threshold_call_median"],
        "ratio_to_16_sequential_calls": round(r16["us_threshold_calls_per_step_median"] / best, 2),
        "goal_us_per_write_16_waiters": 15.0, "goal_met": best <= 15.0}
    ctx.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
