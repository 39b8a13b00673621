"""Device-resident batches over the C ABI: the batched lattice-join engine.

`Context` owns one HIP stream on one GPU; `ORSetBatch` / `GSetBatch` hold R replicas of
one CRDT in the columnar layout of include/laspj.h; `Buffer` holds kernel outputs.
Every method is one C-ABI call (and, for the *_host helpers, one download).
"""

from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np

from . import _lib
from ._lib import check, load


class Context:
    def __init__(self, device: int = 0):
        self.L = load()
        h = C.c_void_p()
        check(self.L.laspj_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device
        # free lists of small batches (the bind path allocates one per call): a batch
        # handle goes back here when its Python object dies and is cleared on reuse
        self._pool = {}
        self.pool_hits = 0

    POOL_MAX_BYTES = 4 << 20
    POOL_MAX_PER_SHAPE = 64

    def _pool_take(self, key):
        lst = self._pool.get(key)
        if lst:
            h = lst.pop()
            check(self.L.laspj_batch_clear(self.h, h), self.h)      # new() again
            self.pool_hits += 1
            return h
        return None

    def _pool_give(self, key, h, nbytes) -> bool:
        if nbytes > self.POOL_MAX_BYTES:
            return False
        lst = self._pool.setdefault(key, [])
        if len(lst) >= self.POOL_MAX_PER_SHAPE:
            return False
        lst.append(h)
        return True

    def close(self):
        if getattr(self, "h", None):
            for lst in getattr(self, "_pool", {}).values():
                for h in lst:
                    self.L.laspj_batch_destroy(h)
            self._pool = {}
            self.L.laspj_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def synchronize(self):
        check(self.L.laspj_ctx_synchronize(self.h), self.h)

    def set_tuning(self, knob: int, value: int):
        check(self.L.laspj_ctx_set_tuning(self.h, knob, value), self.h)

    def last_list_walk(self) -> int:
        """laspj_ctx_last_list_walk: 0 = the last list merge / union / bind did not launch
        the chunked walk, 1 = it did and no replica fell back, 2 = a replica fell back."""
        return int(self.L.laspj_ctx_last_list_walk(self.h))

    # -- factories
    def orset_batch(self, replicas: int, elements: int) -> "ORSetBatch":
        return ORSetBatch(self, replicas, elements)

    def orset_wide_batch(self, replicas: int, elements: int,
                         token_words: int) -> "ORSetWideBatch":
        return ORSetWideBatch(self, replicas, elements, token_words)

    def gset_batch(self, replicas: int, elements: int) -> "GSetBatch":
        return GSetBatch(self, replicas, elements)

    def gcounter_batch(self, replicas: int, actors: int) -> "GCounterBatch":
        return GCounterBatch(self, replicas, actors)

    def buffer(self, nbytes: int) -> "Buffer":
        return Buffer(self, nbytes)

    def event(self) -> "Event":
        return Event(self)

    # -- many one-replica batches per launch
    def bind_many(self, dsts, curs, vals) -> np.ndarray:
        """laspj_batch_bind_many_host: status per item (0 = no-op, 1 = merged into
        dst), read back in the call's one synchronisation."""
        n = len(curs)
        if n == 0:
            return np.zeros((0,), dtype=np.uint8)
        arr = lambda xs: (C.c_void_p * n)(*[x.h.value for x in xs])  # noqa: E731
        st = np.zeros((n,), dtype=np.uint8)
        check(self.L.laspj_batch_bind_many_host(self.h, n, arr(dsts), arr(curs), arr(vals),
                                                st.ctypes.data), self.h)
        return st

    # ------------------------------------------------------------ NIF entry points
    # laspj.h "NIF entry points": term_to_binary images in, images / booleans out, over
    # this context's own dictionary.  Each returns (verdict, answer); answer is None on
    # NIF_FALLBACK (the NIF would run the reference's Erlang clause).

    def nif_merge_many(self, pairs, kind: str = "orset"):
        """lasp_orset:merge/2 (kind "gset": lasp_gset:merge/2) over many (A, B) image
        pairs: [(verdict, image)]."""
        fn = self.L.laspj_gset_etf_merge_many if kind == "gset" else \
            self.L.laspj_orset_etf_merge_many
        n = len(pairs)
        if n == 0:
            return []
        keep = [(bytes(a), bytes(b)) for a, b in pairs]
        pa = (C.c_char_p * n)(*[a for a, _ in keep])
        pb = (C.c_char_p * n)(*[b for _, b in keep])
        na = (C.c_uint64 * n)(*[len(a) for a, _ in keep])
        nb = (C.c_uint64 * n)(*[len(b) for _, b in keep])
        out = (C.c_void_p * n)()
        olen = (C.c_uint64 * n)()
        verd = (C.c_int32 * n)()
        check(fn(self.h, n, pa, na, pb, nb, out, olen, verd), self.h)
        return [(int(verd[k]), C.string_at(out[k], olen[k]) if verd[k] == 0 else None)
                for k in range(n)]

    def nif_merge(self, a: bytes, b: bytes, kind: str = "orset"):
        return self.nif_merge_many([(a, b)], kind)[0]

    def nif_value(self, s: bytes, kind: str = "orset"):
        fn = self.L.laspj_gset_etf_value if kind == "gset" else self.L.laspj_orset_etf_value
        out, olen, verd = C.c_void_p(), C.c_uint64(), C.c_int32()
        s = bytes(s)
        check(fn(self.h, s, len(s), C.byref(out), C.byref(olen), C.byref(verd)), self.h)
        return int(verd.value), (C.string_at(out, olen.value) if verd.value == 0 else None)

    def nif_equal(self, a: bytes, b: bytes, kind: str = "orset"):
        fn = self.L.laspj_gset_etf_equal if kind == "gset" else self.L.laspj_orset_etf_equal
        res, verd = C.c_int32(), C.c_int32()
        a, b = bytes(a), bytes(b)
        check(fn(self.h, a, len(a), b, len(b), C.byref(res), C.byref(verd)), self.h)
        return int(verd.value), (bool(res.value) if verd.value == 0 else None)

    def nif_inflation(self, prev: bytes, cur: bytes, strict: bool = False, kind: str = "orset"):
        fn = self.L.laspj_gset_etf_inflation if kind == "gset" else \
            self.L.laspj_orset_etf_inflation
        res, verd = C.c_int32(), C.c_int32()
        prev, cur = bytes(prev), bytes(cur)
        check(fn(self.h, prev, len(prev), cur, len(cur), int(strict), C.byref(res),
                 C.byref(verd)), self.h)
        return int(verd.value), (bool(res.value) if verd.value == 0 else None)

    def list_etf(self, body: str, kind: str, a: bytes, b: bytes = b""):
        """laspj_list_etf_<body> (args, map, filter, fold, union, intersection, product,
        value) on images: (verdict, image or None)."""
        fn = getattr(self.L, "laspj_list_etf_" + body)
        k = _lib.KIND_GSET if kind == "gset" else _lib.KIND_ORSET
        out, olen, verd = C.c_void_p(), C.c_uint64(), C.c_int32()
        a = bytes(a)
        if body in ("args", "value"):
            check(fn(self.h, k, a, len(a), C.byref(out), C.byref(olen), C.byref(verd)), self.h)
        else:
            b = bytes(b)
            check(fn(self.h, k, a, len(a), b, len(b), C.byref(out), C.byref(olen),
                     C.byref(verd)), self.h)
        return int(verd.value), (C.string_at(out, olen.value) if verd.value == 0 else None)

    def list_etf_bind(self, kind: str, value0: bytes, value: bytes):
        """laspj_list_etf_bind: (verdict, status, written image or None)."""
        k = _lib.KIND_GSET if kind == "gset" else _lib.KIND_ORSET
        out, olen, st, verd = C.c_void_p(), C.c_uint64(), C.c_int32(), C.c_int32()
        value0, value = bytes(value0), bytes(value)
        check(self.L.laspj_list_etf_bind(self.h, k, value0, len(value0), value, len(value),
                                         C.byref(out), C.byref(olen), C.byref(st),
                                         C.byref(verd)), self.h)
        img = C.string_at(out, olen.value) if verd.value == 0 and st.value == 1 else None
        return int(verd.value), int(st.value), img

    def var(self, kind: str = "orset") -> "NifVar":
        """A device-resident variable (laspj_var_create): #dv.value kept on the device, in a
        token namespace of its own."""
        return NifVar(self, kind)

    def var_bind_many(self, pairs):
        """laspj_var_etf_bind_many over (NifVar, image) pairs: [(verdict, status)]."""
        n = len(pairs)
        if n == 0:
            return []
        keep = [bytes(img) for _v, img in pairs]
        vs = (C.c_void_p * n)(*[v.h.value for v, _i in pairs])
        pv = (C.c_char_p * n)(*keep)
        nv = (C.c_uint64 * n)(*[len(x) for x in keep])
        st = (C.c_int32 * n)()
        verd = (C.c_int32 * n)()
        check(self.L.laspj_var_etf_bind_many(self.h, n, vs, pv, nv, st, verd), self.h)
        return [(int(verd[k]), int(st[k])) for k in range(n)]

    def var_recheck_many(self, vars, cap: int = 64):
        """laspj_var_recheck_many over NifVars: [(verdict, [ids met])] per variable."""
        n = len(vars)
        if n == 0:
            return []
        vs = (C.c_void_p * n)(*[v.h.value for v in vars])
        while True:
            ids = (C.c_uint64 * max(cap, 1))()
            nmet = (C.c_uint32 * n)()
            verd = (C.c_int32 * n)()
            check(self.L.laspj_var_recheck_many(self.h, n, vs, ids, cap, nmet, verd), self.h)
            total = sum(int(x) for x in nmet)
            if total <= cap:
                break
            cap = total
        out, at = [], 0
        for k in range(n):
            out.append((int(verd[k]), [int(x) for x in ids[at:at + nmet[k]]]))
            at += nmet[k]
        return out

    def filter(self, in_var: "NifVar", out_var: "NifVar") -> "NifFilter":
        """laspj_filter_create: a resident lasp_process running filter/6 from in_var into
        out_var (one namespace), the fun's results kept on the device."""
        return NifFilter(self, in_var, out_var)

    def list_var(self, peer: "NifVar") -> "NifListVar":
        """laspj_lvar_create: a list-valued lasp_orset variable holding [] in peer's
        namespace (what the combinator bodies bind: `{X, Cx ++ Cy}`, repeated keys)."""
        return NifListVar(self, peer)

    def pair_list_var(self, peer: "NifVar") -> "NifListVar":
        """laspj_lvar_create_pairs: a pair-keyed list variable holding [] in peer's namespace
        (what product/7 binds: `{{X, Y}, [{[Tx, Ty], Bool}]}`); its images are walked in pair
        mode for its whole life."""
        return NifListVar(self, peer, pairs=True)

    def map(self, in_var: "NifVar", out_lvar: "NifListVar") -> "NifMap":
        """laspj_map_create: a resident lasp_process running map/6 from the OR-Set in_var
        into the list variable out_lvar (one namespace)."""
        return NifMap(self, in_var, out_lvar)

    def fold(self, in_var: "NifVar", out_lvar: "NifListVar") -> "NifFold":
        """laspj_fold_create: a resident lasp_process running fold/6 from the OR-Set in_var
        into the list variable out_lvar (one namespace)."""
        return NifFold(self, in_var, out_lvar)

    def filter_run_many(self, filters):
        """laspj_filter_run_many: one re-run of each filter in one device pass —
        [(verdict, status, pending)] per filter."""
        n = len(filters)
        if n == 0:
            return []
        fs = (C.c_void_p * n)(*[f.h.value for f in filters])
        st, pend, verd = (C.c_int32 * n)(), (C.c_uint32 * n)(), (C.c_int32 * n)()
        check(self.L.laspj_filter_run_many(self.h, n, fs, st, pend, verd), self.h)
        return [(int(verd[k]), int(st[k]), int(pend[k])) for k in range(n)]

    def nif_stats(self) -> dict:
        out = (C.c_uint64 * _lib.NIF_STATS)()
        check(self.L.laspj_nif_stats(self.h, out, _lib.NIF_STATS), self.h)
        keys = ("calls", "device_passes", "registrations", "dict_resets", "image_rebuilds",
                "host_encoded_passes", "fallbacks", "dict_elements", "ns_stage_enqueue",
                "ns_device_wait", "ns_answers", "ns_stage_copy", "ns_register", "ns_rebuild",
                "image_patches", "chain_redo_passes", "vars_spilled", "vars_hydrated",
                "device_new_tokens", "namespaces_widened")
        return dict(zip(keys, (int(x) for x in out)))

    def nif_reset(self):
        check(self.L.laspj_nif_reset(self.h), self.h)

    def inflation_many(self, prevs, curs, strict: bool) -> np.ndarray:
        """laspj_batch_inflation_many: is_(strict_)inflation(prev[i], cur[i])."""
        n = len(curs)
        if n == 0:
            return np.zeros((0,), dtype=bool)
        arr = lambda xs: (C.c_void_p * n)(*[x.h.value for x in xs])  # noqa: E731
        out = self.buffer(n)
        check(self.L.laspj_batch_inflation_many(self.h, n, arr(prevs), arr(curs), int(strict),
                                                out.h), self.h)
        return out.download(np.uint8).astype(bool)


class NifVar:
    """laspj_var: one OR-Set / G-Set / G-Counter `#dv.value` resident on the device (laspj.h
    "resident variables").  Every call returns (verdict, answer) like the NIF image calls;
    answer is None on NIF_FALLBACK."""

    def __init__(self, ctx: Context, kind: str = "orset", peer: "NifVar" = None):
        self.ctx, self.L, self.kind = ctx, ctx.L, kind
        self.h = C.c_void_p()
        if peer is not None:
            self.kind = peer.kind
            check(self.L.laspj_var_create_replica(peer.h, C.byref(self.h)), ctx.h)
            return
        kinds = {"orset": _lib.KIND_ORSET, "gset": _lib.KIND_GSET,
                 "gcounter": _lib.KIND_GCOUNTER}
        if kind not in kinds:
            raise ValueError(f"NifVar: unknown kind {kind!r} (one of {sorted(kinds)})")
        check(self.L.laspj_var_create(ctx.h, kinds[kind], C.byref(self.h)), ctx.h)

    def replica(self) -> "NifVar":
        """laspj_var_create_replica: another replica in this variable's namespace."""
        return NifVar(self.ctx, peer=self)

    def update(self, op_img: bytes):
        """lasp_core:update/4 (laspj_var_etf_update): (verdict, result, error element image
        or None, [minted tokens]) — result 0 ok, 1 {error, {precondition, {not_present, E}}}."""
        res, verd, n = C.c_int32(), C.c_int32(), C.c_uint32()
        eimg, elen, mint = C.c_void_p(), C.c_uint64(), C.c_void_p()
        op_img = bytes(op_img)
        check(self.L.laspj_var_etf_update(self.h, op_img, len(op_img), C.byref(res),
                                          C.byref(eimg), C.byref(elen), C.byref(mint),
                                          C.byref(n), C.byref(verd)), self.ctx.h)
        if verd.value != 0:
            return int(verd.value), None, None, []
        err = C.string_at(eimg, elen.value) if res.value == 1 else None
        raw = C.string_at(mint, 20 * n.value) if n.value else b""
        return 0, int(res.value), err, [raw[20 * k:20 * k + 20] for k in range(n.value)]

    def increment(self, op_img: bytes, actor_img: bytes, cap=None):
        """lasp_core:update/4 on a G-Counter (laspj_var_etf_increment): op_img / actor_img
        are the images of `increment | {increment, N}` and of the Actor.  cap None: (verdict,)
        once the kernel is enqueued; else the fused re-check, (verdict, [ids met], waiters
        left) as recheck answers (asking laspj_var_recheck again when more than cap fired:
        the increment itself is applied once)."""
        op_img, actor_img = bytes(op_img), bytes(actor_img)
        verd = C.c_int32()
        if cap is None:
            check(self.L.laspj_var_etf_increment(self.h, op_img, len(op_img), actor_img,
                                                 len(actor_img), None, 0, None, None,
                                                 C.byref(verd)), self.ctx.h)
            return (int(verd.value),)
        ids = (C.c_uint64 * max(cap, 1))()
        nmet, left = C.c_uint32(), C.c_uint32()
        check(self.L.laspj_var_etf_increment(self.h, op_img, len(op_img), actor_img,
                                             len(actor_img), ids, cap, C.byref(nmet),
                                             C.byref(left), C.byref(verd)), self.ctx.h)
        if verd.value != 0:
            return int(verd.value), None, int(left.value)
        if nmet.value > cap:
            return self.recheck(nmet.value)
        return 0, [int(x) for x in ids[:nmet.value]], int(left.value)

    def union(self, left: "NifVar", right: "NifVar"):
        """laspj_var_union: lasp_core:union/7's body over resident left / right (one
        namespace) bound into this variable — (verdict, status)."""
        st, verd = C.c_int32(), C.c_int32()
        check(self.L.laspj_var_union(self.h, left.h, right.h, C.byref(st), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value)

    def intersection(self, left: "NifVar", right: "NifVar"):
        """laspj_var_intersection: lasp_core:intersection/7's body over resident G-Sets
        left / right (one namespace) bound into this variable — (verdict, status)."""
        st, verd = C.c_int32(), C.c_int32()
        check(self.L.laspj_var_intersection(self.h, left.h, right.h, C.byref(st),
                                            C.byref(verd)), self.ctx.h)
        return int(verd.value), int(st.value)

    def close(self):
        if self.h:
            self.L.laspj_var_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def bind(self, img: bytes):
        """bind/3: (verdict, status) — status 0 no-op (Value0 =:= Value), 1 written."""
        st, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_var_etf_bind(self.h, img, len(img), C.byref(st), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value)

    def write(self, img: bytes) -> int:
        verd = C.c_int32()
        img = bytes(img)
        check(self.L.laspj_var_etf_write(self.h, img, len(img), C.byref(verd)), self.ctx.h)
        return int(verd.value)

    def _image(self, fn):
        out, olen, verd = C.c_void_p(), C.c_uint64(), C.c_int32()
        check(fn(self.h, C.byref(out), C.byref(olen), C.byref(verd)), self.ctx.h)
        return int(verd.value), (C.string_at(out, olen.value) if verd.value == 0 else None)

    def read(self, threshold: bytes = None, strict: bool = False, id: int = 0, cap: int = 16):
        """Without a threshold: (verdict, the value's image) (laspj_var_etf_read).  With one:
        read/6 with the lazy threads' walk (laspj_var_read): (met, [lazy ids fired, in list
        order]) — an unmet threshold is registered as a waiter {id, strict, threshold} and
        the fired lazy entries leave; met is None on NIF_FALLBACK.  Asks again with more
        room when more than cap fired (nothing was changed by the first call)."""
        if threshold is None:
            return self._image(self.L.laspj_var_etf_read)
        img = bytes(threshold)
        while True:
            ids = (C.c_uint64 * max(cap, 1))()
            met, verd, nl, still = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
            check(self.L.laspj_var_read(self.h, img, len(img), int(strict), id, C.byref(met),
                                        ids, cap, C.byref(nl), C.byref(still), C.byref(verd)),
                  self.ctx.h)
            if verd.value != 0:
                return None, []
            if nl.value <= cap:
                return bool(met.value), [int(x) for x in ids[:nl.value]]
            cap = nl.value

    def value(self):
        return self._image(self.L.laspj_var_etf_value)

    def threshold(self, img: bytes, strict: bool = False):
        res, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_var_etf_threshold(self.h, img, len(img), int(strict), C.byref(res),
                                             C.byref(verd)), self.ctx.h)
        return int(verd.value), (bool(res.value) if verd.value == 0 else None)

    @property
    def resident(self) -> bool:
        r = C.c_int32()
        check(self.L.laspj_var_resident(self.h, C.byref(r)), self.ctx.h)
        return bool(r.value)

    def wait(self, img: bytes, strict: bool = False, id: int = 0):
        """read/6 (laspj_var_wait): (verdict, met) — an unmet threshold is registered as a
        waiter {id, strict, img}; met is None on NIF_FALLBACK."""
        met, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_var_wait(self.h, img, len(img), int(strict), id, C.byref(met),
                                    C.byref(verd)), self.ctx.h)
        return int(verd.value), (bool(met.value) if verd.value == 0 else None)

    def recheck(self, cap: int = 16):
        """write/4's reply_to_all (laspj_var_recheck): (verdict, [ids met, in registration
        order], waiters left); asks again with more room when more than cap are met."""
        while True:
            ids = (C.c_uint64 * max(cap, 1))()
            nmet, left, verd = C.c_uint32(), C.c_uint32(), C.c_int32()
            check(self.L.laspj_var_recheck(self.h, ids, cap, C.byref(nmet), C.byref(left),
                                           C.byref(verd)), self.ctx.h)
            if nmet.value <= cap:
                return int(verd.value), [int(x) for x in ids[:nmet.value]], int(left.value)
            cap = nmet.value

    def cancel(self, id: int) -> bool:
        found = C.c_int32()
        check(self.L.laspj_var_wait_cancel(self.h, id, C.byref(found)), self.ctx.h)
        return bool(found.value)

    def waiters(self):
        """[(id, strict, threshold image)] in list order."""
        n = C.c_uint32()
        check(self.L.laspj_var_waiter_count(self.h, C.byref(n)), self.ctx.h)
        out = []
        for k in range(n.value):
            wid, strict, p, ln = C.c_uint64(), C.c_int32(), C.c_void_p(), C.c_uint64()
            check(self.L.laspj_var_waiter_at(self.h, k, C.byref(wid), C.byref(strict),
                                             C.byref(p), C.byref(ln)), self.ctx.h)
            out.append((int(wid.value), bool(strict.value), C.string_at(p, ln.value)))
        return out

    def wait_needed(self, img: bytes, strict: bool = False, id: int = 0):
        """wait_needed/6 (laspj_var_wait_needed): needed — True: reply at once (the threshold
        is met, or somebody is reading already); False: registered as the lazy thread {id,
        img}; None on NIF_FALLBACK."""
        needed, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_var_wait_needed(self.h, img, len(img), int(strict), id,
                                           C.byref(needed), C.byref(verd)), self.ctx.h)
        return bool(needed.value) if verd.value == 0 else None

    def lazy(self):
        """[(id, threshold image)] of `#dv.lazy_threads`, in list order."""
        n = C.c_uint32()
        check(self.L.laspj_var_lazy_count(self.h, C.byref(n)), self.ctx.h)
        out = []
        for k in range(n.value):
            wid, p, ln = C.c_uint64(), C.c_void_p(), C.c_uint64()
            check(self.L.laspj_var_lazy_at(self.h, k, C.byref(wid), C.byref(p), C.byref(ln)),
                  self.ctx.h)
            out.append((int(wid.value), C.string_at(p, ln.value)))
        return out

    def lazy_cancel(self, id: int) -> bool:
        found = C.c_int32()
        check(self.L.laspj_var_lazy_cancel(self.h, id, C.byref(found)), self.ctx.h)
        return bool(found.value)


def read_any(reads, id: int = 0, cap: int = 16):
    """read_any/3 (laspj_var_read_any) over (NifVar, threshold image, strict) triples of one
    context: (found, [[lazy ids fired] per read]) — found: the first read met, -1 when none
    is (every read then left the waiter {id, strict, img}), None on NIF_FALLBACK.  Asks again
    with more room when more than cap lazy threads fired."""
    n = len(reads)
    if n == 0:
        return -1, []
    ctx = reads[0][0].ctx
    keep = [bytes(img) for _v, img, _s in reads]
    vs = (C.c_void_p * n)(*[v.h.value for v, _i, _s in reads])
    pv = (C.c_char_p * n)(*keep)
    nv = (C.c_uint64 * n)(*[len(x) for x in keep])
    st = (C.c_int32 * n)(*[int(bool(s)) for _v, _i, s in reads])
    while True:
        ids = (C.c_uint64 * max(cap, 1))()
        nl = (C.c_uint32 * n)()
        found, verd = C.c_int32(), C.c_int32()
        check(ctx.L.laspj_var_read_any(ctx.h, n, vs, pv, nv, st, id, C.byref(found), ids, cap,
                                       nl, C.byref(verd)), ctx.h)
        if verd.value != 0:
            return None, []
        total = sum(int(x) for x in nl)
        if total <= cap:
            break
        cap = total
    out, at = [], 0
    for k in range(n):
        out.append([int(x) for x in ids[at:at + nl[k]]])
        at += nl[k]
    return int(found.value), out


class NifFilter:
    """laspj_filter: a resident lasp_process running filter/6 (laspj.h "resident filter
    processes").  run / args answer (verdict, ...) like the variable calls."""

    def __init__(self, ctx: Context, in_var: NifVar, out_var: NifVar):
        self.ctx, self.L = ctx, ctx.L
        self.in_var, self.out_var = in_var, out_var
        self.h = C.c_void_p()
        check(self.L.laspj_filter_create(in_var.h, out_var.h, C.byref(self.h)), ctx.h)

    def run(self):
        """laspj_filter_run: (verdict, status, pending) — pending > 0: out is untouched,
        go through args / results and run again; else status 0 no-op, 1 written."""
        st, pend, verd = C.c_int32(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_filter_run(self.h, C.byref(st), C.byref(pend), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value), int(pend.value)

    def args(self):
        """laspj_filter_args: (verdict, image of the pending arguments' list, count)."""
        out, olen, cnt, verd = C.c_void_p(), C.c_uint64(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_filter_args(self.h, C.byref(out), C.byref(olen), C.byref(cnt),
                                       C.byref(verd)), self.ctx.h)
        if verd.value != 0:
            return int(verd.value), None, 0
        return 0, C.string_at(out, olen.value), int(cnt.value)

    def results(self, image: bytes):
        """laspj_filter_results: the fun's results for the last args list, as a list image."""
        image = bytes(image)
        check(self.L.laspj_filter_results(self.h, image, len(image)), self.ctx.h)

    def step(self, fun, max_rounds: int = 8):
        """The Erlang side's loop for one re-run (the stand-in for the NIF): run; while
        elements are pending, args -> fun on each decoded argument -> results -> run.
        (verdict, status, pending) of the last run."""
        from . import etf
        for _ in range(max_rounds):
            verd, st, pend = self.run()
            if verd != 0 or pend == 0:
                return verd, st, pend
            verd, img, _n = self.args()
            if verd != 0:
                return verd, 0, pend
            res = [fun(a) for a in etf.binary_to_term(img)]
            self.results(etf.term_to_binary(res))
        raise RuntimeError("NifFilter.step: elements still pending")

    def close(self):
        if self.h:
            self.L.laspj_filter_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NifListVar:
    """laspj_lvar: one list-valued lasp_orset `#dv.value` resident on the device over a
    NifVar's namespace (laspj.h "list-valued resident variables").  Calls answer (verdict,
    ...) like the variable calls; bind statuses are 0 no-op, 1 written, 2 refused (the merge
    does not inflate the value: nothing written)."""

    def __init__(self, ctx: Context, peer: NifVar, pairs: bool = False):
        self.ctx, self.L = ctx, ctx.L
        self.h = C.c_void_p()
        self.pairs = pairs
        make = self.L.laspj_lvar_create_pairs if pairs else self.L.laspj_lvar_create
        check(make(peer.h, C.byref(self.h)), ctx.h)

    def product(self, left: NifVar, right: NifVar):
        """laspj_lvar_product: product/7's OR-Set branch over resident left / right bound into
        this pair-keyed variable — (verdict, status)."""
        st, verd = C.c_int32(), C.c_int32()
        check(self.L.laspj_lvar_product(self.h, left.h, right.h, C.byref(st), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value)

    def product_recheck(self, left: NifVar, right: NifVar, cap: int = 16):
        """laspj_lvar_product_recheck: the product's re-run and, when it writes, the waiters'
        re-check inside the bind's synchronisation — (verdict, status, [ids met, in list
        order], waiters left), as intersection_recheck answers."""
        ids = (C.c_uint64 * max(cap, 1))()
        st, nmet, left_n, verd = C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_lvar_product_recheck(self.h, left.h, right.h, C.byref(st), ids, cap,
                                                C.byref(nmet), C.byref(left_n),
                                                C.byref(verd)), self.ctx.h)
        if nmet.value > cap:
            verd2, got, n = self.recheck(nmet.value)
            return verd2, int(st.value), got, n
        return int(verd.value), int(st.value), [int(x) for x in ids[:nmet.value]], \
            int(left_n.value)

    def intersection(self, left: NifVar, right: NifVar):
        """laspj_lvar_intersection: intersection/7's OR-Set branch over resident left / right
        bound into this variable — (verdict, status)."""
        st, verd = C.c_int32(), C.c_int32()
        check(self.L.laspj_lvar_intersection(self.h, left.h, right.h, C.byref(st),
                                             C.byref(verd)), self.ctx.h)
        return int(verd.value), int(st.value)

    def bind(self, img: bytes):
        """bind/3 of any list image: (verdict, status)."""
        st, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_lvar_etf_bind(self.h, img, len(img), C.byref(st), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value)

    def write(self, img: bytes) -> int:
        verd = C.c_int32()
        img = bytes(img)
        check(self.L.laspj_lvar_etf_write(self.h, img, len(img), C.byref(verd)), self.ctx.h)
        return int(verd.value)

    def _image(self, fn):
        out, olen, verd = C.c_void_p(), C.c_uint64(), C.c_int32()
        check(fn(self.h, C.byref(out), C.byref(olen), C.byref(verd)), self.ctx.h)
        return int(verd.value), (C.string_at(out, olen.value) if verd.value == 0 else None)

    def read(self, threshold: bytes = None, strict: bool = False, id: int = 0, cap: int = 16):
        """Without a threshold: (verdict, the value's image) (laspj_lvar_etf_read).  With one:
        read/6 with the lazy threads' walk (laspj_lvar_read): (met, [lazy ids fired, in list
        order]) — an unmet threshold is registered as a waiter {id, strict, threshold} and
        the fired lazy entries leave; met is None on NIF_FALLBACK.  Asks again with more
        room when more than cap fired (nothing was changed by the first call)."""
        if threshold is None:
            return self._image(self.L.laspj_lvar_etf_read)
        img = bytes(threshold)
        while True:
            ids = (C.c_uint64 * max(cap, 1))()
            met, verd, nl, still = C.c_int32(), C.c_int32(), C.c_uint32(), C.c_uint32()
            check(self.L.laspj_lvar_read(self.h, img, len(img), int(strict), id, C.byref(met),
                                         ids, cap, C.byref(nl), C.byref(still), C.byref(verd)),
                  self.ctx.h)
            if verd.value != 0:
                return None, []
            if nl.value <= cap:
                return bool(met.value), [int(x) for x in ids[:nl.value]]
            cap = nl.value

    def value(self):
        """(verdict, the image of lasp_orset:value/1 on the list)."""
        return self._image(self.L.laspj_lvar_etf_value)

    def threshold(self, img: bytes, strict: bool = False):
        res, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_lvar_etf_threshold(self.h, img, len(img), int(strict),
                                              C.byref(res), C.byref(verd)), self.ctx.h)
        return int(verd.value), (bool(res.value) if verd.value == 0 else None)

    def wait(self, img: bytes, strict: bool = False, id: int = 0):
        """read/6 (laspj_lvar_wait): (verdict, met) — an unmet threshold is registered as a
        waiter {id, strict, img}; met is None on NIF_FALLBACK."""
        met, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_lvar_wait(self.h, img, len(img), int(strict), id, C.byref(met),
                                     C.byref(verd)), self.ctx.h)
        return int(verd.value), (bool(met.value) if verd.value == 0 else None)

    def recheck(self, cap: int = 16):
        """write/4's reply_to_all (laspj_lvar_recheck): (verdict, [ids met, in list order],
        waiters left); asks again with more room when more than cap are met."""
        while True:
            ids = (C.c_uint64 * max(cap, 1))()
            nmet, left, verd = C.c_uint32(), C.c_uint32(), C.c_int32()
            check(self.L.laspj_lvar_recheck(self.h, ids, cap, C.byref(nmet), C.byref(left),
                                            C.byref(verd)), self.ctx.h)
            if nmet.value <= cap:
                return int(verd.value), [int(x) for x in ids[:nmet.value]], int(left.value)
            cap = nmet.value

    def intersection_recheck(self, left: NifVar, right: NifVar, cap: int = 16):
        """laspj_lvar_intersection_recheck: the intersection's re-run and, when it writes, the
        waiters' re-check inside the same device pass — (verdict, status, [ids met, in list
        order], waiters left).  More than cap met: the value is written already, so the ids
        are fetched by recheck with the room asked for."""
        ids = (C.c_uint64 * max(cap, 1))()
        st, nmet, left_n, verd = C.c_int32(), C.c_uint32(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_lvar_intersection_recheck(self.h, left.h, right.h, C.byref(st), ids,
                                                     cap, C.byref(nmet), C.byref(left_n),
                                                     C.byref(verd)), self.ctx.h)
        if nmet.value > cap:
            verd2, got, n = self.recheck(nmet.value)
            return verd2, int(st.value), got, n
        return int(verd.value), int(st.value), [int(x) for x in ids[:nmet.value]], \
            int(left_n.value)

    def cancel(self, id: int) -> bool:
        found = C.c_int32()
        check(self.L.laspj_lvar_wait_cancel(self.h, id, C.byref(found)), self.ctx.h)
        return bool(found.value)

    def waiters(self):
        """[(id, strict, threshold image)] in list order."""
        n = C.c_uint32()
        check(self.L.laspj_lvar_waiter_count(self.h, C.byref(n)), self.ctx.h)
        out = []
        for k in range(n.value):
            wid, strict, p, ln = C.c_uint64(), C.c_int32(), C.c_void_p(), C.c_uint64()
            check(self.L.laspj_lvar_waiter_at(self.h, k, C.byref(wid), C.byref(strict),
                                              C.byref(p), C.byref(ln)), self.ctx.h)
            out.append((int(wid.value), bool(strict.value), C.string_at(p, ln.value)))
        return out

    def wait_needed(self, img: bytes, strict: bool = False, id: int = 0):
        """wait_needed/6 (laspj_lvar_wait_needed): needed — True: reply at once (the threshold
        is met, or somebody is reading already); False: registered as the lazy thread {id,
        img}; None on NIF_FALLBACK."""
        needed, verd = C.c_int32(), C.c_int32()
        img = bytes(img)
        check(self.L.laspj_lvar_wait_needed(self.h, img, len(img), int(strict), id,
                                            C.byref(needed), C.byref(verd)), self.ctx.h)
        return bool(needed.value) if verd.value == 0 else None

    def lazy(self):
        """[(id, threshold image)] of `#dv.lazy_threads`, in list order."""
        n = C.c_uint32()
        check(self.L.laspj_lvar_lazy_count(self.h, C.byref(n)), self.ctx.h)
        out = []
        for k in range(n.value):
            wid, p, ln = C.c_uint64(), C.c_void_p(), C.c_uint64()
            check(self.L.laspj_lvar_lazy_at(self.h, k, C.byref(wid), C.byref(p), C.byref(ln)),
                  self.ctx.h)
            out.append((int(wid.value), C.string_at(p, ln.value)))
        return out

    def lazy_cancel(self, id: int) -> bool:
        found = C.c_int32()
        check(self.L.laspj_lvar_lazy_cancel(self.h, id, C.byref(found)), self.ctx.h)
        return bool(found.value)

    def counts(self):
        """(entries, tokens) of the resident list."""
        ne, nt = C.c_uint32(), C.c_uint32()
        check(self.L.laspj_lvar_counts(self.h, C.byref(ne), C.byref(nt)), self.ctx.h)
        return int(ne.value), int(nt.value)

    @property
    def resident(self) -> bool:
        r = C.c_int32()
        check(self.L.laspj_lvar_resident(self.h, C.byref(r)), self.ctx.h)
        return bool(r.value)

    def close(self):
        if self.h:
            self.L.laspj_lvar_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def list_read_any(reads, id: int = 0, cap: int = 16):
    """read_any/3 (laspj_lvar_read_any) over (NifListVar, threshold image, strict) triples of
    one context: (found, [[lazy ids fired] per read]), shaped like read_any."""
    n = len(reads)
    if n == 0:
        return -1, []
    ctx = reads[0][0].ctx
    keep = [bytes(img) for _v, img, _s in reads]
    vs = (C.c_void_p * n)(*[v.h.value for v, _i, _s in reads])
    pv = (C.c_char_p * n)(*keep)
    nv = (C.c_uint64 * n)(*[len(x) for x in keep])
    st = (C.c_int32 * n)(*[int(bool(s)) for _v, _i, s in reads])
    while True:
        ids = (C.c_uint64 * max(cap, 1))()
        nl = (C.c_uint32 * n)()
        found, verd = C.c_int32(), C.c_int32()
        check(ctx.L.laspj_lvar_read_any(ctx.h, n, vs, pv, nv, st, id, C.byref(found), ids, cap,
                                        nl, C.byref(verd)), ctx.h)
        if verd.value != 0:
            return None, []
        total = sum(int(x) for x in nl)
        if total <= cap:
            break
        cap = total
    out, at = [], 0
    for k in range(n):
        out.append([int(x) for x in ids[at:at + nl[k]]])
        at += nl[k]
    return int(found.value), out


class NifMap:
    """laspj_map: a resident lasp_process running map/6 (laspj.h "resident map processes")
    from a NifVar into a NifListVar.  run / args / results answer (verdict, ...) like the
    filter's calls; bind statuses as NifListVar's."""

    def __init__(self, ctx: Context, in_var: NifVar, out_lvar: NifListVar):
        self.ctx, self.L = ctx, ctx.L
        self.in_var, self.out_lvar = in_var, out_lvar
        self.h = C.c_void_p()
        check(self.L.laspj_map_create(in_var.h, out_lvar.h, C.byref(self.h)), ctx.h)

    def run(self):
        """laspj_map_run: (verdict, status, pending) — pending > 0: out is untouched, go
        through args / results and run again; else status 0 no-op, 1 written, 2 refused."""
        st, pend, verd = C.c_int32(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_map_run(self.h, C.byref(st), C.byref(pend), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value), int(pend.value)

    def args(self):
        """laspj_map_args: (verdict, image of the pending arguments' list, count)."""
        out, olen, cnt, verd = C.c_void_p(), C.c_uint64(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_map_args(self.h, C.byref(out), C.byref(olen), C.byref(cnt),
                                    C.byref(verd)), self.ctx.h)
        if verd.value != 0:
            return int(verd.value), None, 0
        return 0, C.string_at(out, olen.value), int(cnt.value)

    def results(self, image: bytes) -> int:
        """laspj_map_results: the list image of F(X) for the last args list — the verdict
        (NIF_FALLBACK: the map is refused, nothing recorded)."""
        image = bytes(image)
        verd = C.c_int32()
        check(self.L.laspj_map_results(self.h, image, len(image), C.byref(verd)), self.ctx.h)
        return int(verd.value)

    def step(self, fun, max_rounds: int = 8):
        """The Erlang side's loop for one re-run (the stand-in for the NIF): run; while
        elements are pending, args -> fun on each decoded argument -> results -> run.
        (verdict, status, pending) of the last run."""
        from . import etf
        for _ in range(max_rounds):
            verd, st, pend = self.run()
            if verd != 0 or pend == 0:
                return verd, st, pend
            verd, img, _n = self.args()
            if verd != 0:
                return verd, 0, pend
            res = [fun(a) for a in etf.binary_to_term(img)]
            verd = self.results(etf.term_to_binary(res))
            if verd != 0:
                return verd, 0, pend
        raise RuntimeError("NifMap.step: elements still pending")

    def close(self):
        if self.h:
            self.L.laspj_map_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class NifFold:
    """laspj_fold: a resident lasp_process running fold/6 (laspj.h "resident fold
    processes") from a NifVar into a NifListVar; the fun answers a list per element.
    Shaped as NifMap."""

    def __init__(self, ctx: Context, in_var: NifVar, out_lvar: NifListVar):
        self.ctx, self.L = ctx, ctx.L
        self.in_var, self.out_lvar = in_var, out_lvar
        self.h = C.c_void_p()
        check(self.L.laspj_fold_create(in_var.h, out_lvar.h, C.byref(self.h)), ctx.h)

    def run(self):
        """laspj_fold_run: (verdict, status, pending) — pending > 0: out is untouched, go
        through args / results and run again; else status 0 no-op, 1 written, 2 refused."""
        st, pend, verd = C.c_int32(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_fold_run(self.h, C.byref(st), C.byref(pend), C.byref(verd)),
              self.ctx.h)
        return int(verd.value), int(st.value), int(pend.value)

    def args(self):
        """laspj_fold_args: (verdict, image of the pending arguments' list, count)."""
        out, olen, cnt, verd = C.c_void_p(), C.c_uint64(), C.c_uint32(), C.c_int32()
        check(self.L.laspj_fold_args(self.h, C.byref(out), C.byref(olen), C.byref(cnt),
                                     C.byref(verd)), self.ctx.h)
        if verd.value != 0:
            return int(verd.value), None, 0
        return 0, C.string_at(out, olen.value), int(cnt.value)

    def results(self, image: bytes) -> int:
        """laspj_fold_results: the image of the list of F(X), each a list, for the last args
        list — the verdict (NIF_FALLBACK: the fold is refused, nothing recorded)."""
        image = bytes(image)
        verd = C.c_int32()
        check(self.L.laspj_fold_results(self.h, image, len(image), C.byref(verd)), self.ctx.h)
        return int(verd.value)

    def step(self, fun, max_rounds: int = 8):
        """NifMap.step with a list-valued fun: (verdict, status, pending) of the last run."""
        from . import etf
        for _ in range(max_rounds):
            verd, st, pend = self.run()
            if verd != 0 or pend == 0:
                return verd, st, pend
            verd, img, _n = self.args()
            if verd != 0:
                return verd, 0, pend
            res = [fun(a) for a in etf.binary_to_term(img)]
            verd = self.results(etf.term_to_binary(res))
            if verd != 0:
                return verd, 0, pend
        raise RuntimeError("NifFold.step: elements still pending")

    def close(self):
        if self.h:
            self.L.laspj_fold_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def device_count() -> int:
    L = load()
    n = C.c_int()
    check(L.laspj_device_count(C.byref(n)))
    return n.value


class Buffer:
    def __init__(self, ctx: Context, nbytes: int):
        self.ctx = ctx
        h = C.c_void_p()
        check(ctx.L.laspj_buf_create(ctx.h, nbytes, C.byref(h)), ctx.h)
        self.h = h
        self.nbytes = nbytes

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.L.laspj_buf_destroy(self.h)
            self.h = None

    def download(self, dtype=np.uint8, count: Optional[int] = None, offset: int = 0) -> np.ndarray:
        itemsize = np.dtype(dtype).itemsize
        if count is None:
            count = (self.nbytes - offset) // itemsize
        out = np.empty((count,), dtype=dtype)
        check(self.ctx.L.laspj_buf_download(self.ctx.h, self.h, offset, out.ctypes.data,
                                            count * itemsize), self.ctx.h)
        return out

    def upload(self, arr: np.ndarray, offset: int = 0):
        arr = np.ascontiguousarray(arr)
        check(self.ctx.L.laspj_buf_upload(self.ctx.h, self.h, offset, arr.ctypes.data,
                                          arr.nbytes), self.ctx.h)


class Event:
    def __init__(self, ctx: Context):
        self.ctx = ctx
        h = C.c_void_p()
        check(ctx.L.laspj_event_create(ctx.h, C.byref(h)), ctx.h)
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.L.laspj_event_destroy(self.h)
            self.h = None

    def record(self):
        check(self.ctx.L.laspj_event_record(self.ctx.h, self.h), self.ctx.h)

    def elapsed_ms(self, stop: "Event") -> float:
        ms = C.c_float()
        check(self.ctx.L.laspj_event_elapsed_ms(self.h, stop.h, C.byref(ms)), self.ctx.h)
        return ms.value


class ETFDict:
    """Device copy of a dictionary's external term images (laspj_etf_dict_create):
    element slot images in term order and, for OR-Sets, per-element token images."""

    def __init__(self, ctx: Context, elements: int, elem_blob: bytes, elem_off: np.ndarray,
                 elem_order: np.ndarray, tok_blob: Optional[bytes] = None,
                 tok_off: Optional[np.ndarray] = None, tok_order: Optional[np.ndarray] = None):
        self.ctx = ctx
        eb = np.frombuffer(elem_blob or b"\0", dtype=np.uint8)
        eo = np.ascontiguousarray(elem_off, dtype=np.uint32)
        eord = np.ascontiguousarray(elem_order, dtype=np.uint32)
        if tok_off is not None:
            tb = np.frombuffer(tok_blob or b"\0", dtype=np.uint8)
            to = np.ascontiguousarray(tok_off, dtype=np.uint32)
            tord = np.ascontiguousarray(tok_order, dtype=np.uint8)
            tptrs = (tb.ctypes.data, to.ctypes.data, tord.ctypes.data)
        else:
            tptrs = (None, None, None)
        h = C.c_void_p()
        check(ctx.L.laspj_etf_dict_create(ctx.h, elements, eb.ctypes.data, eo.ctypes.data,
                                          eord.ctypes.data, *tptrs, C.byref(h)), ctx.h)
        self.h = h
        self.elements = elements

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.L.laspj_etf_dict_destroy(self.h)
            self.h = None


class _Batch:
    kind = 0
    _create = ""

    def __init__(self, ctx: Context, replicas: int, elements: int):
        self.ctx = ctx
        key = (self._create, replicas, elements)
        h = ctx._pool_take(key)
        if h is None:
            h = C.c_void_p()
            check(getattr(ctx.L, self._create)(ctx.h, replicas, elements, C.byref(h)), ctx.h)
        self.h = h
        self._pool_key = key
        self.replicas = replicas
        self.elements = elements
        info = _lib.BatchInfo()
        check(ctx.L.laspj_batch_info_get(self.h, C.byref(info)))
        self.bytes_per_replica = info.bytes_per_replica
        self.nbytes = info.bytes

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            key = getattr(self, "_pool_key", None)
            if key is None or not self.ctx._pool_give(key, self.h, self.nbytes):
                self.ctx.L.laspj_batch_destroy(self.h)
            self.h = None

    @property
    def words_per_replica(self) -> int:
        return self.bytes_per_replica // 8

    def upload(self, host: np.ndarray, first: int = 0):
        host = np.ascontiguousarray(host, dtype=np.uint64)
        count = host.nbytes // self.bytes_per_replica
        if count * self.bytes_per_replica != host.nbytes:
            raise ValueError("host array is not a whole number of replicas")
        check(self.ctx.L.laspj_batch_upload(self.ctx.h, self.h, first, count, host.ctypes.data),
              self.ctx.h)

    def download_words(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        if count is None:
            count = self.replicas - first
        out = np.empty((count, self.words_per_replica), dtype=np.uint64)
        check(self.ctx.L.laspj_batch_download(self.ctx.h, self.h, first, count,
                                              out.ctypes.data), self.ctx.h)
        return out

    def clear(self):
        check(self.ctx.L.laspj_batch_clear(self.ctx.h, self.h), self.ctx.h)

    def download_range(self, offset: int, nbytes: int) -> np.ndarray:
        """Bytes [offset, offset + nbytes) of the batch's device image."""
        out = np.zeros((nbytes,), dtype=np.uint8)
        check(self.ctx.L.laspj_batch_download_range(self.ctx.h, self.h, offset, nbytes,
                                                    out.ctypes.data), self.ctx.h)
        return out

    def view(self, first: int, count: int) -> "_Batch":
        """A non-owning batch of the same kind over replicas [first, first + count)
        (laspj_batch_device_ptr + laspj_batch_wrap); keeps this batch alive."""
        if first < 0 or count < 1 or first + count > self.replicas:
            raise ValueError("replica range out of bounds")
        p = C.c_void_p()
        check(self.ctx.L.laspj_batch_device_ptr(self.h, C.byref(p)))
        out = type(self).__new__(type(self))
        out.ctx, out._keep = self.ctx, self
        h = C.c_void_p()
        check(self.ctx.L.laspj_batch_wrap(self.ctx.h, self.kind,
                                          C.c_void_p(p.value + first * self.bytes_per_replica),
                                          count * self.bytes_per_replica, count, self.elements,
                                          C.byref(h)), self.ctx.h)
        out.h = h
        out.replicas, out.elements = count, self.elements
        out.bytes_per_replica = self.bytes_per_replica
        out.nbytes = count * self.bytes_per_replica
        return out

    def fill_synthetic(self, seed: int, replica_base: int = 0, token_slots: int = 0):
        if token_slots:
            check(self.ctx.L.laspj_batch_fill_synthetic_tokens(self.ctx.h, self.h, seed,
                                                               replica_base, token_slots),
                  self.ctx.h)
            return
        check(self.ctx.L.laspj_batch_fill_synthetic(self.ctx.h, self.h, seed, replica_base),
              self.ctx.h)

    def join_n(self, srcs):
        """self = srcs[0] ⊔ ... ⊔ srcs[n-1] (laspj_batch_join_n; self may be one of them)."""
        arr = (C.c_void_p * len(srcs))(*[b.h for b in srcs])
        check(self.ctx.L.laspj_batch_join_n(self.ctx.h, self.h, arr, len(srcs)), self.ctx.h)
        return self

    def reduce_chunks(self, src: "_Batch", nchunks: int):
        """self[i] = join over j of src[j*R + i] (laspj_batch_reduce_chunks)."""
        check(self.ctx.L.laspj_batch_reduce_chunks(self.ctx.h, self.h, src.h, nchunks),
              self.ctx.h)
        return self

    def etf_encode(self, d: ETFDict, tag: int = -1, vers: int = 1):
        """to_binary/1 payloads of every replica, on the device: (offsets Buffer of
        R + 1 uint64, payload Buffer, total bytes).  tag < 0: bare term_to_binary/1."""
        size_fn, write_fn = self._etf
        offs = Buffer(self.ctx, 8 * (self.replicas + 1))
        total = C.c_uint64()
        check(getattr(self.ctx.L, size_fn)(self.ctx.h, self.h, d.h, tag, offs.h,
                                           C.byref(total)), self.ctx.h)
        out = Buffer(self.ctx, max(1, total.value))
        check(getattr(self.ctx.L, write_fn)(self.ctx.h, self.h, d.h, tag, vers, offs.h, out.h),
              self.ctx.h)
        return offs, out, total.value

    def etf_decode(self, d: ETFDict, payload: "Buffer", offsets: "Buffer", tag: int = -1,
                   vers: int = 1) -> np.ndarray:
        """from_binary/1 of every replica on the device (laspj_orset_etf_read /
        laspj_gset_etf_read): payload
        bytes [offsets[i], offsets[i+1]) into replica i; returns the LASPJ_DEC_* status
        per replica (replicas with a non-zero status are undefined)."""
        st = self.ctx.buffer(4 * max(1, self.replicas))
        fn = self.ctx.L.laspj_gset_etf_read if self.kind == _lib.KIND_GSET else \
            self.ctx.L.laspj_orset_etf_read
        check(fn(self.ctx.h, self.h, d.h, tag, vers, payload.h, offsets.h, st.h), self.ctx.h)
        return st.download(np.int32, count=self.replicas)

    def to_binaries(self, d: ETFDict, tag: int = -1, vers: int = 1) -> list:
        """etf_encode + download, split per replica."""
        offs, out, total = self.etf_encode(d, tag, vers)
        o = offs.download(np.uint64)
        blob = out.download(np.uint8, count=total).tobytes() if total else b""
        return [blob[int(o[i]):int(o[i + 1])] for i in range(self.replicas)]

    def _bool_out(self, fn, *args) -> np.ndarray:
        buf = self.ctx.buffer(self.replicas)
        check(fn(self.ctx.h, *args, buf.h), self.ctx.h)
        return buf.download(np.uint8).astype(bool)

    def _apply_ops(self, fn, ops: Sequence[tuple], statuses: bool = True):
        """statuses=False (every op an ADD, whose precondition cannot fail): no status
        readback, the call does not wait for the device; returns None."""
        n = len(ops)
        arr = (_lib.Op * max(n, 1))()
        for k, (rep, elem, kind, slot, flags) in enumerate(ops):
            arr[k].replica, arr[k].element, arr[k].kind = rep, elem, kind
            arr[k].slot, arr[k].flags, arr[k].pad = slot, flags, 0
        if not statuses:
            check(fn(self.ctx.h, self.h, arr, n, None), self.ctx.h)
            return None
        status = np.zeros((max(n, 1),), dtype=np.int32)
        check(fn(self.ctx.h, self.h, arr, n, status.ctypes.data_as(C.POINTER(C.c_int32))),
              self.ctx.h)
        return status[:n]


class ORSetBatch(_Batch):
    """R replicas of an OR-Set over E element slots (16-byte {p, r} cells)."""

    kind = _lib.KIND_ORSET
    _create = "laspj_orset_batch_create"
    _etf = ("laspj_orset_etf_size", "laspj_orset_etf_write")

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """(count, E, 2) uint64 array of {p, r} cells."""
        w = self.download_words(first, count)
        return w.reshape(w.shape[0], self.elements, 2)

    # lasp_orset:merge/2
    def join(self, a: "ORSetBatch", b: "ORSetBatch"):
        check(self.ctx.L.laspj_orset_join(self.ctx.h, self.h, a.h, b.h), self.ctx.h)
        return self

    def reduce_from(self, src: "ORSetBatch", group: int):
        check(self.ctx.L.laspj_orset_reduce(self.ctx.h, self.h, src.h, group), self.ctx.h)
        return self

    def value_bits(self, removed: bool = False) -> np.ndarray:
        W = (self.elements + 63) // 64
        buf = self.ctx.buffer(self.replicas * W * 8)
        fn = self.ctx.L.laspj_orset_removed if removed else self.ctx.L.laspj_orset_value
        check(fn(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, W)

    def fragment(self, element: int) -> np.ndarray:
        """(R, 2) cells of one element slot (value({tokens, E}) / {fragment, E})."""
        buf = self.ctx.buffer(self.replicas * 16)
        check(self.ctx.L.laspj_orset_fragment(self.ctx.h, self.h, element, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, 2)

    def precondition_context(self, src: "ORSetBatch"):
        """self := precondition_context(src) per replica."""
        check(self.ctx.L.laspj_orset_precondition_context(self.ctx.h, self.h, src.h),
              self.ctx.h)
        return self

    def stats(self) -> np.ndarray:
        buf = self.ctx.buffer(self.replicas * 24)
        check(self.ctx.L.laspj_orset_stats(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, 3)

    def equal(self, other: "ORSetBatch") -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_orset_equal, self.h, other.h)

    def is_inflation_of(self, prev: "ORSetBatch", strict: bool = False) -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_orset_inflation, prev.h, self.h, int(strict))

    def apply_ops(self, ops: Sequence[tuple], statuses: bool = True):
        """ops: (replica, element_slot, OP_ADD|OP_REMOVE, token_slot, flags)."""
        return self._apply_ops(self.ctx.L.laspj_orset_apply_ops, ops, statuses)

    def union(self, l: "ORSetBatch", r: "ORSetBatch"):
        check(self.ctx.L.laspj_orset_union(self.ctx.h, self.h, l.h, r.h), self.ctx.h)
        return self

    def filter(self, src: "ORSetBatch", keep_bits: np.ndarray):
        keep = self.ctx.buffer(((self.elements + 63) // 64) * 8)
        keep.upload(np.ascontiguousarray(keep_bits, dtype=np.uint64))
        check(self.ctx.L.laspj_orset_filter(self.ctx.h, self.h, src.h, keep.h), self.ctx.h)
        self.ctx.synchronize()
        return self

    # intersection body (lasp_core.erl:546-589): returns a CONCAT batch
    def intersection(self, r: "ORSetBatch") -> "ConcatBatch":
        out = ConcatBatch(self.ctx, self.replicas, self.elements)
        check(self.ctx.L.laspj_orset_intersection(self.ctx.h, out.h, self.h, r.h), self.ctx.h)
        return out

    # product body (lasp_core.erl:499-533): returns a PRODUCT batch (EL x ER cells):
    # 4-byte cells when every token slot is < 8 (detected on the device), else 32-byte
    def product(self, r: "ORSetBatch", out=None, wide: Optional[bool] = None):
        if out is None and not wide:
            out = ORSetProductBatch(self.ctx, self.replicas, self.elements, r.elements)
        if out is not None:
            st = self.ctx.L.laspj_orset_product(self.ctx.h, out.h, self.h, r.h)
            if st == _lib.OK:
                return out
            if st != _lib.E_RANGE or wide is False or not isinstance(out, ORSetProductBatch):
                check(st, self.ctx.h)
        out = ORSetProductWideBatch(self.ctx, self.replicas, self.elements, r.elements)
        check(self.ctx.L.laspj_orset_product(self.ctx.h, out.h, self.h, r.h), self.ctx.h)
        return out

    def product_diag(self, r: "ORSetBatch", out=None) -> "ORSetProductBatch":
        """product then filter({X, Y} -> X =:= Y), fused (laspj_orset_product_diag): an
        EL = E, ER = 1 PRODUCT batch whose cell (e, 0) pairs slot e of both sides (one
        element dictionary shared by self and r)."""
        if out is None:
            out = ORSetProductBatch(self.ctx, self.replicas, self.elements, 1)
        check(self.ctx.L.laspj_orset_product_diag(self.ctx.h, out.h, self.h, r.h), self.ctx.h)
        return out

    # a gather whose output is threshold-checked in the same pass (config 4 fused)
    def gather_inflation(self, src: "ORSetBatch", index, prev: "ORSetBatch",
                         strict: bool = True, chains=None) -> np.ndarray:
        """self <- src through index; returns is_(strict_)inflation(prev, self) per
        replica (laspj_orset_gather_inflation).  `index` is a uint32 array or Buffer.
        `chains` = (head, next) from key_chains(): the keyed form, for outputs whose keys
        repeat across src slots (laspj_orset_gather_inflation_keyed)."""
        def dev(a):
            if isinstance(a, Buffer):
                return a
            b = self.ctx.buffer(4 * self.elements)
            b.upload(np.ascontiguousarray(a, dtype=np.uint32))
            return b
        idx = dev(index)
        out = self.ctx.buffer(self.replicas)
        if chains is None:
            check(self.ctx.L.laspj_orset_gather_inflation(self.ctx.h, self.h, src.h, idx.h,
                                                          prev.h, int(strict), out.h),
                  self.ctx.h)
        else:
            hd, nx = (dev(c) for c in chains)
            check(self.ctx.L.laspj_orset_gather_inflation_keyed(
                self.ctx.h, self.h, src.h, idx.h, hd.h, nx.h, prev.h, int(strict), out.h),
                self.ctx.h)
        return out.download(np.uint8).astype(bool)

    # map / fold bodies: self <- src gathered through index (one u32 per slot of self)
    def gather(self, src: "ORSetBatch", index: np.ndarray):
        idx = self.ctx.buffer(4 * self.elements)
        idx.upload(np.ascontiguousarray(index, dtype=np.uint32))
        check(self.ctx.L.laspj_orset_gather(self.ctx.h, self.h, src.h, idx.h), self.ctx.h)
        self.ctx.synchronize()
        return self


def _wrap(self, ctx: Context, tensor, replicas: int, elements: int, bytes_per_replica: int):
    self.ctx = ctx
    self._keep = tensor
    nbytes = tensor.numel() * tensor.element_size()
    h = C.c_void_p()
    check(ctx.L.laspj_batch_wrap(ctx.h, self.kind, C.c_void_p(tensor.data_ptr()),
                                 nbytes, replicas, elements, C.byref(h)), ctx.h)
    self.h = h
    self.replicas, self.elements = replicas, elements
    self.bytes_per_replica = bytes_per_replica
    self.nbytes = nbytes


class ORSetWideBatch(ORSetBatch):
    """R replicas of an OR-Set with T = 64 k token slots per element
    (LASPJ_KIND_ORSET_WIDE): k {p, r} pairs per cell, token slot t in pair t // 64.  Join,
    reduce, equal, value/removed, stats, inflation and update/3 take it; the combinator
    bodies and the codec take narrow batches only."""

    kind = _lib.KIND_ORSET_WIDE

    def __init__(self, ctx: Context, replicas: int, elements: int, token_words: int):
        self.ctx = ctx
        self.token_words = token_words
        h = C.c_void_p()
        check(ctx.L.laspj_orset_wide_batch_create(ctx.h, replicas, elements, token_words,
                                                  C.byref(h)), ctx.h)
        self.h = h
        self._pool_key = None
        self.replicas, self.elements = replicas, elements
        info = _lib.BatchInfo()
        check(ctx.L.laspj_batch_info_get(self.h, C.byref(info)))
        self.bytes_per_replica, self.nbytes = info.bytes_per_replica, info.bytes

    def fragment(self, element: int) -> np.ndarray:
        """(R, k, 2) pairs of one element slot."""
        k = self.token_words
        buf = self.ctx.buffer(self.replicas * 16 * k)
        check(self.ctx.L.laspj_orset_fragment(self.ctx.h, self.h, element, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, k, 2)

    def widen_from(self, src: "ORSetBatch") -> "ORSetWideBatch":
        """laspj_orset_widen: self := src (narrow, or wide with fewer token words)."""
        check(self.ctx.L.laspj_orset_widen(self.ctx.h, self.h, src.h), self.ctx.h)
        return self

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        """(count, E, k, 2) uint64 array of {p, r} pairs."""
        w = self.download_words(first, count)
        return w.reshape(w.shape[0], self.elements, self.token_words, 2)

    def apply_ops(self, ops: Sequence[tuple], statuses: bool = True):
        """ops: (replica, element_slot, OP_*, token_slot 0 .. 64 k - 1, flags)."""
        n = len(ops)
        arr = (_lib.Op * max(n, 1))()
        for i, (rep, elem, kind, slot, flags) in enumerate(ops):
            arr[i].replica, arr[i].element, arr[i].kind = rep, elem, kind
            arr[i].slot, arr[i].flags, arr[i].pad = slot & 255, flags, slot >> 8
        fn = self.ctx.L.laspj_orset_apply_ops
        if not statuses:
            check(fn(self.ctx.h, self.h, arr, n, None), self.ctx.h)
            return None
        status = np.zeros((max(n, 1),), dtype=np.int32)
        check(fn(self.ctx.h, self.h, arr, n, status.ctypes.data_as(C.POINTER(C.c_int32))),
              self.ctx.h)
        return status[:n]


class WrappedORSetBatch(ORSetBatch):
    """An OR-Set batch over device memory owned by someone else (e.g. a torch tensor
    that RCCL collectives write into); laspj_batch_wrap, non-owning."""

    def __init__(self, ctx: Context, tensor, replicas: int, elements: int):
        _wrap(self, ctx, tensor, replicas, elements, 16 * elements)


class ConcatBatch(_Batch):
    """Intersection output: per slot {pL, rL, pR, rR} (tokens decode as Cx ++ Cy)."""

    kind = _lib.KIND_ORSET_CONCAT
    _create = "laspj_orset_concat_batch_create"

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        w = self.download_words(first, count)
        return w.reshape(w.shape[0], self.elements, 4)

    def value_bits(self) -> np.ndarray:
        W = (self.elements + 63) // 64
        buf = self.ctx.buffer(self.replicas * W * 8)
        check(self.ctx.L.laspj_orset_value(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, W)


class _ProductBatch(_Batch):
    def __init__(self, ctx: Context, replicas: int, el: int, er: int):
        self.ctx = ctx
        h = C.c_void_p()
        check(getattr(ctx.L, self._create)(ctx.h, replicas, el, er, C.byref(h)), ctx.h)
        self.h = h
        self.replicas, self.elements, self.elements_r = replicas, el, er
        info = _lib.BatchInfo()
        check(ctx.L.laspj_batch_info_get(self.h, C.byref(info)))
        self.bytes_per_replica = info.bytes_per_replica
        self.nbytes = info.bytes
        self.cells = info.cells_per_replica


class ORSetProductBatch(_ProductBatch):
    """Product output: EL x ER uint32 cells {pX:8, rX:8, pY:8, rY:8}."""

    kind = _lib.KIND_ORSET_PRODUCT
    _create = "laspj_orset_product_batch_create"

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        w = self.download_words(first, count)
        return w.view(np.uint32)[:, : self.cells].reshape(w.shape[0], self.elements,
                                                           self.elements_r)

    def value_bits(self) -> np.ndarray:
        W = (self.cells + 63) // 64
        buf = self.ctx.buffer(self.replicas * W * 8)
        check(self.ctx.L.laspj_orset_value(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, W)


class ORSetProductWideBatch(_ProductBatch):
    """Product output for any token slots: EL x ER cells of {pX, rX, pY, rY} u64."""

    kind = _lib.KIND_ORSET_PRODUCT_WIDE
    _create = "laspj_orset_product_wide_batch_create"

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        w = self.download_words(first, count)
        return w.reshape(w.shape[0], self.elements, self.elements_r, 4)

    def value_bits(self) -> np.ndarray:
        W = (self.cells + 63) // 64
        buf = self.ctx.buffer(self.replicas * W * 8)
        check(self.ctx.L.laspj_orset_value(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64).reshape(self.replicas, W)


class GSetProductBatch(_ProductBatch):
    """G-Set product output: EL rows x ceil(ER/64) words."""

    kind = _lib.KIND_GSET_PRODUCT
    _create = "laspj_gset_product_batch_create"

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        w = self.download_words(first, count)
        return w.reshape(w.shape[0], self.elements, (self.elements_r + 63) // 64)


class GSetBatch(_Batch):
    """R replicas of a G-Set over E element slots (ceil(E/64) u64 words)."""

    kind = _lib.KIND_GSET
    _create = "laspj_gset_batch_create"
    _etf = ("laspj_gset_etf_size", "laspj_gset_etf_write")

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        return self.download_words(first, count)

    def join(self, a: "GSetBatch", b: "GSetBatch"):
        check(self.ctx.L.laspj_gset_join(self.ctx.h, self.h, a.h, b.h), self.ctx.h)
        return self

    def reduce_from(self, src: "GSetBatch", group: int):
        check(self.ctx.L.laspj_gset_reduce(self.ctx.h, self.h, src.h, group), self.ctx.h)
        return self

    def stats(self) -> np.ndarray:
        buf = self.ctx.buffer(self.replicas * 8)
        check(self.ctx.L.laspj_gset_stats(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64)

    def equal(self, other: "GSetBatch") -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_gset_equal, self.h, other.h)

    def is_inflation_of(self, prev: "GSetBatch", strict: bool = False) -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_gset_inflation, prev.h, self.h, int(strict))

    def apply_ops(self, ops: Sequence[tuple], statuses: bool = True):
        return self._apply_ops(self.ctx.L.laspj_gset_apply_ops, ops, statuses)

    def union(self, l: "GSetBatch", r: "GSetBatch"):
        check(self.ctx.L.laspj_gset_union(self.ctx.h, self.h, l.h, r.h), self.ctx.h)
        return self

    def intersection(self, l: "GSetBatch", r: "GSetBatch"):
        check(self.ctx.L.laspj_gset_intersection(self.ctx.h, self.h, l.h, r.h), self.ctx.h)
        return self

    def filter(self, src: "GSetBatch", keep_bits: np.ndarray):
        keep = self.ctx.buffer(self.words_per_replica * 8)
        keep.upload(np.ascontiguousarray(keep_bits, dtype=np.uint64))
        check(self.ctx.L.laspj_gset_filter(self.ctx.h, self.h, src.h, keep.h), self.ctx.h)
        self.ctx.synchronize()
        return self

    def product(self, r: "GSetBatch") -> "GSetProductBatch":
        out = GSetProductBatch(self.ctx, self.replicas, self.elements, r.elements)
        check(self.ctx.L.laspj_gset_product(self.ctx.h, out.h, self.h, r.h), self.ctx.h)
        return out

    def gather(self, src: "GSetBatch", index: np.ndarray):
        idx = self.ctx.buffer(4 * self.elements)
        idx.upload(np.ascontiguousarray(index, dtype=np.uint32))
        check(self.ctx.L.laspj_gset_gather(self.ctx.h, self.h, src.h, idx.h), self.ctx.h)
        self.ctx.synchronize()
        return self


class GCounterBatch(_Batch):
    """R replicas of a riak_dt_gcounter over E actor slots (uint64 count per slot)."""

    kind = _lib.KIND_GCOUNTER
    _create = "laspj_gcounter_batch_create"

    def download(self, first: int = 0, count: Optional[int] = None) -> np.ndarray:
        return self.download_words(first, count)

    def join(self, a: "GCounterBatch", b: "GCounterBatch"):
        check(self.ctx.L.laspj_gcounter_join(self.ctx.h, self.h, a.h, b.h), self.ctx.h)
        return self

    def reduce_from(self, src: "GCounterBatch", group: int):
        check(self.ctx.L.laspj_gcounter_reduce(self.ctx.h, self.h, src.h, group), self.ctx.h)
        return self

    def values(self) -> np.ndarray:
        buf = self.ctx.buffer(self.replicas * 8)
        check(self.ctx.L.laspj_gcounter_value(self.ctx.h, self.h, buf.h), self.ctx.h)
        return buf.download(np.uint64)

    def threshold_met(self, threshold: int, strict: bool = False) -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_gcounter_threshold, self.h, int(threshold),
                              int(strict))

    def is_inflation_of(self, prev: "GCounterBatch", strict: bool = False) -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_gcounter_inflation, prev.h, self.h, int(strict))

    def equal(self, other: "GCounterBatch") -> np.ndarray:
        return self._bool_out(self.ctx.L.laspj_gcounter_equal, self.h, other.h)

    def increment(self, incs: Sequence[tuple]):
        """incs: (replica, actor_slot, amount)."""
        n = len(incs)
        arr = (_lib.Incr * max(n, 1))()
        for k, (rep, actor, amount) in enumerate(incs):
            if not 0 < amount < (1 << 64):
                raise ValueError(f"increment amount {amount} is not in 1 .. 2^64-1")
            arr[k].replica, arr[k].actor, arr[k].amount = rep, actor, amount
        check(self.ctx.L.laspj_gcounter_apply_increments(self.ctx.h, self.h, arr, n), self.ctx.h)
        return self


class WrappedGCounterBatch(GCounterBatch):
    """A G-Counter batch over someone else's device memory (the int64 tensor an RCCL
    all_reduce(MAX) writes into); laspj_batch_wrap, non-owning."""

    def __init__(self, ctx: Context, tensor, replicas: int, actors: int):
        _wrap(self, ctx, tensor, replicas, actors, 8 * actors)


class ListBatch:
    """R list-faithful values (LASPJ_KIND_ORSET_LIST / GSET_LIST, include/laspj.h "list
    values"): entries in list order, key items and token runs.  Every method is one
    C-ABI call; the list entry points size their outputs themselves."""

    def __init__(self, ctx: Context, kind: int, replicas: int = 1, cap_entries: int = 1,
                 cap_tokens: int = 1):
        self.ctx, self.kind, self.replicas = ctx, kind, replicas
        h = C.c_void_p()
        check(ctx.L.laspj_list_batch_create(ctx.h, kind, replicas, cap_entries, cap_tokens,
                                            C.byref(h)), ctx.h)
        self.h = h

    def __del__(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.L.laspj_batch_destroy(self.h)
            self.h = None

    @property
    def gset(self) -> bool:
        return self.kind == _lib.KIND_GSET_LIST

    def _like(self, kind: Optional[int] = None) -> "ListBatch":
        return ListBatch(self.ctx, self.kind if kind is None else kind, self.replicas)

    def counts(self) -> np.ndarray:
        out = np.zeros((self.replicas, 2), dtype=np.uint32)
        check(self.ctx.L.laspj_list_counts(self.ctx.h, self.h, out.ctypes.data), self.ctx.h)
        return out

    def upload(self, keys, toff=None, toks=None, replica: int = 0):
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        n = len(keys)
        if toff is None:
            toff = np.zeros((n + 1,), dtype=np.uint32)
        toff = np.ascontiguousarray(toff, dtype=np.uint32)
        toks = np.ascontiguousarray(np.zeros((0,), np.uint64) if toks is None else toks,
                                    dtype=np.uint64)
        check(self.ctx.L.laspj_list_upload(self.ctx.h, self.h, replica, n,
                                           keys.ctypes.data if n else None,
                                           toff.ctypes.data,
                                           toks.ctypes.data if len(toks) else None), self.ctx.h)
        return self

    def download(self, replica: int = 0):
        """(keys u64[n], toff u32[n+1], toks u64[nt]) of one replica."""
        n, nt = (int(x) for x in self.counts()[replica])
        keys = np.zeros((max(n, 1),), dtype=np.uint64)
        toff = np.zeros((n + 1,), dtype=np.uint32)
        toks = np.zeros((max(nt, 1),), dtype=np.uint64)
        check(self.ctx.L.laspj_list_download(self.ctx.h, self.h, replica, keys.ctypes.data,
                                             toff.ctypes.data, toks.ctypes.data), self.ctx.h)
        return keys[:n], toff, toks[:nt]

    @classmethod
    def from_set(cls, batch, elem_order: "Buffer", nslots: int,
                 tok_order: Optional["Buffer"]) -> "ListBatch":
        kind = _lib.KIND_GSET_LIST if batch.kind == _lib.KIND_GSET else _lib.KIND_ORSET_LIST
        out = cls(batch.ctx, kind, batch.replicas)
        check(batch.ctx.L.laspj_list_from_set(batch.ctx.h, out.h, batch.h, elem_order.h, nslots,
                                              tok_order.h if tok_order is not None else None),
              batch.ctx.h)
        return out

    def _binary(self, fn, other: "ListBatch", order) -> "ListBatch":
        out = self._like()
        args = (C.byref(order),) if order is not None else ()
        check(fn(self.ctx.h, out.h, self.h, other.h, *args), self.ctx.h)
        return out

    # lasp_orset:merge/2, lasp_gset:merge/2 on lists
    def merge(self, other: "ListBatch", order) -> "ListBatch":
        return self._binary(self.ctx.L.laspj_list_merge, other, order)

    def union(self, other: "ListBatch", order) -> "ListBatch":
        return self._binary(self.ctx.L.laspj_list_union, other, order)

    def intersection(self, other: "ListBatch", order) -> "ListBatch":
        return self._binary(self.ctx.L.laspj_list_intersection, other, order)

    def intersection_set(self, other, tok_order: Optional["Buffer"]) -> "ListBatch":
        """laspj_list_intersection_set: the body with a canonical right side (an OR-Set /
        G-Set batch; tok_order: laspj_list_from_set's token-order rows)."""
        out = self._like()
        check(self.ctx.L.laspj_list_intersection_set(
            self.ctx.h, out.h, self.h, other.h, tok_order.h if tok_order is not None else None),
            self.ctx.h)
        return out

    def product(self, other: "ListBatch") -> "ListBatch":
        return self._binary(self.ctx.L.laspj_list_product, other, None)

    def equal(self, other: "ListBatch", order) -> np.ndarray:
        buf = self.ctx.buffer(self.replicas)
        check(self.ctx.L.laspj_list_equal(self.ctx.h, self.h, other.h, C.byref(order), buf.h),
              self.ctx.h)
        return buf.download(np.uint8).astype(bool)

    def is_inflation_of(self, prev: "ListBatch", order, strict: bool = False) -> np.ndarray:
        buf = self.ctx.buffer(self.replicas)
        check(self.ctx.L.laspj_list_inflation(self.ctx.h, prev.h, self.h, int(strict),
                                              C.byref(order), buf.h), self.ctx.h)
        return buf.download(np.uint8).astype(bool)

    # lasp_core:bind/3 (lasp_core.erl:291-312) on list values, one call
    def bind(self, val: "ListBatch", order):
        """(merged, status) for Value0 = self, Value = val: status[i] = 0 when
        self[i] =:= val[i] (no-op), 1 when merged[i] = Type:merge(self[i], val[i])
        inflates self[i] (the bind writes it), 2 when it does not (no write)."""
        out = self._like()
        st = np.zeros((self.replicas,), dtype=np.uint8)
        check(self.ctx.L.laspj_list_bind(self.ctx.h, out.h, self.h, val.h, C.byref(order),
                                         st.ctypes.data), self.ctx.h)
        return out, st

    def value(self) -> "ListBatch":
        out = self._like(_lib.KIND_GSET_LIST)
        check(self.ctx.L.laspj_list_value(self.ctx.h, out.h, self.h), self.ctx.h)
        return out

    def map(self, keys: np.ndarray, per_entry: bool) -> "ListBatch":
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        tab = self.ctx.buffer(max(8, keys.nbytes))
        if len(keys):
            tab.upload(keys)
        out = self._like()
        check(self.ctx.L.laspj_list_map(self.ctx.h, out.h, self.h, tab.h, len(keys),
                                        int(per_entry)), self.ctx.h)
        return out

    def filter(self, keep: np.ndarray, per_entry: bool) -> "ListBatch":
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        tab = self.ctx.buffer(max(1, keep.nbytes))
        if len(keep):
            tab.upload(keep)
        out = self._like()
        check(self.ctx.L.laspj_list_filter(self.ctx.h, out.h, self.h, tab.h, len(keep),
                                           int(per_entry)), self.ctx.h)
        return out

    def fold(self, off: np.ndarray, keys: np.ndarray, per_entry: bool) -> "ListBatch":
        off = np.ascontiguousarray(off, dtype=np.uint32)
        keys = np.ascontiguousarray(keys, dtype=np.uint64)
        ob = self.ctx.buffer(off.nbytes)
        ob.upload(off)
        kb = self.ctx.buffer(max(8, keys.nbytes))
        if len(keys):
            kb.upload(keys)
        out = self._like()
        check(self.ctx.L.laspj_list_fold(self.ctx.h, out.h, self.h, ob.h, kb.h, len(off) - 1,
                                         int(per_entry)), self.ctx.h)
        return out


def key_chains(keys: np.ndarray):
    """The key chains of laspj_orset_gather_inflation_keyed for output slots whose key
    ids (any integers; equal ids = equal key terms) are `keys`, in list order:
    head[o] = first slot with o's key, next[o] = the next one (0xFFFFFFFF after the last)."""
    keys = np.asarray(keys)
    n = len(keys)
    order = np.argsort(keys, kind="stable")          # slots grouped by key, list order kept
    ks = keys[order]
    start = np.ones(n, dtype=bool)
    start[1:] = ks[1:] != ks[:-1]
    first = order[np.maximum.accumulate(np.where(start, np.arange(n), 0))]
    head = np.empty(n, dtype=np.uint32)
    head[order] = first
    nxt = np.full(n, 0xFFFFFFFF, dtype=np.uint32)
    cont = ~start[1:]
    nxt[order[:-1][cont]] = order[1:][cont]
    return head, nxt


def antientropy_plan(kind: int, rank: int, nranks: int, state_words: int,
                     piece_words: int = 0) -> list:
    """The steps one rank's anti-entropy round runs (laspj_antientropy_plan; host only, no
    GPU): a list of dicts with the laspj_ae_step fields, in order."""
    from ._lib import AEStep
    L = load()
    n = C.c_uint64()
    check(L.laspj_antientropy_plan(kind, rank, nranks, state_words, piece_words, None, 0,
                                   C.byref(n)))
    arr = (AEStep * max(1, n.value))()
    check(L.laspj_antientropy_plan(kind, rank, nranks, state_words, piece_words, arr,
                                   n.value, C.byref(n)))
    return [{f: getattr(arr[k], f) for f, _ in AEStep._fields_} for k in range(n.value)]


class Comm:
    """A communicator of the anti-entropy collective (laspj_comm_*, RCCL over xGMI)."""

    ID_BYTES = 128

    def __init__(self, ctx: Context, nranks: int, uid: bytes, rank: int, _h=None):
        self.ctx = ctx
        if _h is not None:
            self.h = _h
        else:
            buf = (C.c_uint8 * self.ID_BYTES).from_buffer_copy(uid)
            h = C.c_void_p()
            check(ctx.L.laspj_comm_init_rank(ctx.h, nranks, buf, rank, C.byref(h)), ctx.h)
            self.h = h
        r, n = C.c_int(), C.c_int()
        check(ctx.L.laspj_comm_info(self.h, C.byref(r), C.byref(n)))
        self.rank, self.nranks = r.value, n.value

    @staticmethod
    def unique_id() -> bytes:
        L = load()
        buf = (C.c_uint8 * Comm.ID_BYTES)()
        check(L.laspj_comm_unique_id(buf))
        return bytes(buf)

    @classmethod
    def init_all(cls, ctxs: Sequence[Context]) -> list:
        """One communicator per context, one process driving every GPU."""
        n = len(ctxs)
        L = ctxs[0].L
        harr = (C.c_void_p * n)(*[c.h.value for c in ctxs])
        out = (C.c_void_p * n)()
        check(L.laspj_comm_init_all(harr, n, out), ctxs[0].h)
        return [cls(ctxs[i], n, b"", i, _h=C.c_void_p(out[i])) for i in range(n)]

    def close(self):
        if getattr(self, "h", None) and getattr(self.ctx, "h", None):
            self.ctx.L.laspj_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def antientropy(self, state, recv=None, chunk=None):
        """One round (laspj_antientropy): state becomes the join over all ranks."""
        check(self.ctx.L.laspj_antientropy(self.h, state.h, recv.h if recv else None,
                                           chunk.h if chunk else None), self.ctx.h)

    @staticmethod
    def antientropy_group(comms: Sequence["Comm"], states, recvs=None, chunks=None):
        n = len(comms)
        L = comms[0].ctx.L
        arr = lambda xs: (C.c_void_p * n)(*[x.h.value if x is not None else None  # noqa: E731
                                             for x in xs])
        check(L.laspj_antientropy_group(arr(comms), arr(states),
                                        arr(recvs) if recvs else None,
                                        arr(chunks) if chunks else None, n), comms[0].ctx.h)
