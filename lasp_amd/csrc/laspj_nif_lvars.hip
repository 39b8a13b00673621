// List-valued variables (laspj_lvar_*).
// include/laspj.h "list-valued resident variables": a `#dv.value` that is any list of
// {Key, [{Token, Bool}]}, kept as a LIST batch over the slots of a laspj_var namespace.  The
// list kernels are laspj_lists.hip's; the order tables and the producer of intersection/7's
// OR-Set branch (lasp_core.erl:559-568, 583) are laspj_lvars.hip's.  The variable's waiting
// threads (read/6 and write/4's reply_to_all, lasp_core.erl:331-364, 765-825) are kept here as
// device lists and checked by laspj_lists.hip's waiter pass, alone or behind a bind; its lazy
// threads (wait_needed/6, :730-758) likewise, and read/6 / read_any/3 over them (:331-364,
// 371-420, 795-813) answered by laspj_lists.hip's read pass.

#include "laspj_nif_internal.h"

using laspj::fail;
using laspj::var_state;

namespace laspj {

void lwaiter_release(LWaiter& w) {
    if (w.list) laspj_batch_destroy(w.list);
    w.list = nullptr;
}

void llazy_clear(laspj_lvar* lv) {
    for (LWaiter& z : lv->lazy) lwaiter_release(z);
    lv->lazy.clear();
}

// an image of the variable walked in its mode: pair-keyed variables take
// [{{X, Y}, [{[Tx, Ty], Bool}]}] (list_walk_pairs), the others list_walk's OR-Set lists
int lvar_walk_image(laspj_dict* dict, bool pairs, const uint8_t* p, size_t n, ListItems* it) {
    return pairs ? list_walk_pairs(dict, p, n, it)
                 : list_walk(dict, LASPJ_KIND_ORSET, p, n, it, nullptr);
}

namespace {

// the list of a one-replica batch as items (list order)
int lvar_download(laspj_ctx* ctx, const laspj_batch* b, ListItems* it) {
    uint32_t cnt[2] = {0, 0};
    if (int s = laspj_list_counts(ctx, b, cnt)) return s;
    it->keys.assign(std::max(cnt[0], 1u), 0);
    it->toff.assign(cnt[0] + 1ull, 0);
    it->toks.assign(std::max(cnt[1], 1u), 0);
    if (int s = laspj_list_download(ctx, b, 0, it->keys.data(), it->toff.data(), it->toks.data()))
        return s;
    it->keys.resize(cnt[0]);
    it->toks.resize(cnt[1]);
    return LASPJ_OK;
}

int lvar_upload(laspj_ctx* ctx, laspj_batch* b, const ListItems& it) {
    return laspj_list_upload(ctx, b, 0, (uint32_t)it.keys.size(), it.keys.data(), it.toff.data(),
                             it.toks.empty() ? nullptr : it.toks.data());
}

// A resident list written out to its image while the dictionary its items refer to is still
// there (a reset or a widening follows); S->mu held, ctx->mu not
int lvar_spill(NifState* S, laspj_lvar* lv) {
    KindState& K = *lv->ns;
    if (!lv->ctx || !lv->resident || lv->epoch != K.epoch || !K.dict) return LASPJ_OK;
    ListItems it;
    if (int s = lvar_download(lv->ctx, lv->list, &it)) return s;
    std::string img;
    if (int s = list_write(K.dict, LASPJ_KIND_ORSET, it, &img))
        return fail(lv->ctx, s, "lvar: image of a list variable");
    lv->image.assign(img.begin(), img.end());
    lv->resident = false;
    lv->held = false;
    ++S->stats[ST_SPILLED];
    return LASPJ_OK;
}

}  // namespace

// (reg_mark to lvar_ready, and lvar_scratch: shared with the map processes, laspj_nif_maps.hip)
// what a walk registered in the namespace: the device images are stale from here on
RegMark reg_mark(const KindState& K) {
    RegMark m;
    uint64_t eb = 0;
    if (K.dict) laspj_dict_info(K.dict, &m.n, &eb, &m.tb);
    return m;
}
void reg_note(NifState* S, KindState& K, const RegMark& before) {
    const RegMark now = reg_mark(K);
    if (now.n == before.n && now.tb == before.tb) return;
    K.stale = true;
    ++S->stats[ST_REGISTRATIONS];
}

// the namespace's device images brought up to its dictionary (patched when only tokens of
// known elements arrived); call without ctx->mu held, with at least one element registered
int lvar_images(laspj_ctx* ctx, NifState* S, KindState& K) {
    if (!K.stale && K.etf) return LASPJ_OK;
    if (patch_etf(ctx, S, K)) return LASPJ_OK;
    return rebuild_etf(ctx, S, K);
}

// The order tables sized to the images' element slots and derived on the device: fully when
// the images were rebuilt (or the tables are new), for the patched slots otherwise — the
// steady state uploads the few dirty slot numbers and nothing else.  ctx->mu held.
int lvar_ranks(laspj_ctx* ctx, NifState* S, KindState& K) {
    const uint32_t E = K.etf && !K.wide ? K.E : 0, cap = std::max(E, 1u);
    if (K.rank_E != cap || !K.krank || !K.grank) {
        if (int s = grow_dev(ctx, &K.krank, &K.krank_bytes, 4ull * cap)) return s;
        if (int s = grow_dev(ctx, &K.grank, &K.grank_bytes, 256ull * cap)) return s;
        K.rank_E = cap;
        K.rank_full = true;
    }
    if (!E) return LASPJ_OK;
    const uint32_t* eo = etf_dict_elem_order(K.etf);
    const uint8_t* to = etf_dict_tok_order(K.etf);
    if (!eo || !to) return fail(ctx, LASPJ_E_DEVICE, "lvar: the images hold no order arrays");
    auto* kr = static_cast<uint32_t*>(K.krank);
    auto* gr = static_cast<uint32_t*>(K.grank);
    if (K.rank_full) {
        LJ_HIP(ctx, hipMemsetAsync(gr, 0, 256ull * E, ctx->stream));
        LJ_HIP(ctx, launch_lv_ranks(ctx, eo, to, E, kr, gr, nullptr, 0));
        K.rank_full = false;
        K.rank_dirty.clear();
        return LASPJ_OK;
    }
    if (K.rank_dirty.empty()) return LASPJ_OK;
    std::sort(K.rank_dirty.begin(), K.rank_dirty.end());
    K.rank_dirty.erase(std::unique(K.rank_dirty.begin(), K.rank_dirty.end()), K.rank_dirty.end());
    const uint32_t nd = (uint32_t)K.rank_dirty.size();
    const uint64_t bytes = std::max<uint64_t>(4ull * nd, 256);
    void* blk = nullptr;
    if (dev_alloc(ctx, bytes, &blk) != hipSuccess) {
        hipGetLastError();
        return fail(ctx, LASPJ_E_NOMEM, "lvar: dirty slots");
    }
    const void* staged = stage_small(ctx, K.rank_dirty.data(), 4ull * nd);
    hipError_t e = hipMemcpyAsync(blk, staged ? staged : K.rank_dirty.data(), 4ull * nd,
                                  hipMemcpyHostToDevice, ctx->stream);
    // (an unstaged copy reads the host vector: it must land before the vector is cleared)
    if (e == hipSuccess && !staged) e = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess)
        e = launch_lv_ranks(ctx, eo, to, E, kr, gr, static_cast<const uint32_t*>(blk), nd);
    dev_release(ctx, blk, bytes);
    LJ_HIP(ctx, e);
    K.rank_dirty.clear();
    return LASPJ_OK;
}

// *ok: the variable's list is on the device over the current dictionary.  A list written
// out by a dictionary reset is walked back in here (its terms registered afresh); in a wide
// namespace, or when the walk refuses the image, it stays host-held.  S->mu held.
int lvar_ready(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, bool* ok) {
    KindState& K = *lv->ns;
    *ok = lv->resident && lv->epoch == K.epoch && !K.wide;
    if (*ok || lv->held || K.wide || lv->image.empty()) return LASPJ_OK;
    if (!K.dict)
        if (int s = reset_dict(ctx, S, K)) return s;
    const RegMark m = reg_mark(K);
    ListItems it;
    const int st = lvar_walk_image(K.dict, lv->pairs, lv->image.data(), lv->image.size(), &it);
    if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "lvar: host allocation");
    if (st != LASPJ_DEC_OK) {
        lv->held = true;
        return LASPJ_OK;
    }
    reg_note(S, K, m);
    if (int s = lvar_upload(ctx, lv->list, it)) return s;
    lv->resident = true;
    lv->epoch = K.epoch;
    lv->image.clear();
    lv->image.shrink_to_fit();
    ++S->stats[ST_HYDRATED];
    *ok = true;
    return LASPJ_OK;
}

namespace {

// images and tables ready for a list kernel over the namespace (S->mu held, ctx->mu not)
int lvar_prepare(laspj_ctx* ctx, NifState* S, KindState& K) {
    if (K.dict && dict_elements(K.dict) > 0)
        if (int s = lvar_images(ctx, S, K)) return s;
    Guard g(ctx);
    return lvar_ranks(ctx, S, K);
}

// bind/3 (lasp_core.erl:291-312) of lv->val into the variable: laspj_list_bind's status; the
// merge becomes the variable's list by a swap of the two batches when it is written
// tail (or null): the variable's waiters checked against the merge inside the bind's one
// synchronisation (list_bind_tail); met: a byte per waiter, written when the status is 1
int lvar_bind(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, int32_t* status,
              const std::vector<ListWaiter>* tail = nullptr, uint8_t* met = nullptr) {
    const LvOrder ord(ctx, *lv->ns);
    uint8_t st = 0;
    const uint64_t t0 = now_ns();
    // (pair keys have no rank universe: straight to the general bind, no rank-indexed try)
    if (lv->pairs) lv->list->not_asc = lv->val->not_asc = true;
    if (int s = list_bind_tail(ctx, lv->dst, lv->list, lv->val, &ord.o, &st,
                               tail ? tail->data() : nullptr, tail ? (uint32_t)tail->size() : 0,
                               met))
        return s;
    ++S->stats[ST_PASSES];
    S->stats[ST_NS_WAIT] += now_ns() - t0;
    if (st == 1) std::swap(lv->list, lv->dst);
    *status = st;
    return LASPJ_OK;
}

}  // namespace

// the producer's scratch: tile sums on the device, its totals in pinned memory (ctx->mu held)
int lvar_scratch(laspj_ctx* ctx, NifState* S, uint32_t ntile) {
    if (int s = grow_dev(ctx, &S->lv_tiles, &S->lv_tiles_bytes, 16ull * ntile)) return s;
    if (S->lv_ans) return LASPJ_OK;
    void* h = nullptr;
    if (hipHostMalloc(&h, 64, hipHostMallocCoherent) != hipSuccess) {
        hipGetLastError();
        return fail(ctx, LASPJ_E_NOMEM, "lvar: pinned totals");
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        hipGetLastError();
        hipHostFree(h);
        return fail(ctx, LASPJ_E_DEVICE, "lvar: pinned totals' device address");
    }
    S->lv_ans = static_cast<uint32_t*>(h);
    S->lv_ans_d = static_cast<uint32_t*>(d);
    return LASPJ_OK;
}

namespace {

// laspj_lvar_intersection with S->mu held and the handles checked
int lvar_intersection_locked(laspj_ctx* ctx, NifState* S, laspj_lvar* out, laspj_var* l,
                             laspj_var* r, int32_t* status, int32_t* verdict,
                             const std::vector<ListWaiter>* tail = nullptr,
                             uint8_t* met = nullptr) {
    ++S->stats[ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    // OR-Sets of the list's namespace only: cells of another namespace name other terms
    // (a pair-keyed variable takes product/7's output only)
    if (out->pairs || l->kind != LASPJ_KIND_ORSET || r->kind != LASPJ_KIND_ORSET ||
        l->ns != out->ns || r->ns != out->ns)
        return fallback(S);
    KindState& K = *out->ns;
    if (K.wide) return fallback(S);
    for (laspj_var* v : {l, r}) {
        bool ok = false;
        if (int s = hydrate(ctx, S, v, &ok)) return s;
        if (!ok) return fallback(S);
    }
    bool ok = false;
    if (int s = lvar_ready(ctx, S, out, &ok)) return s;
    // (a decode above may have widened the namespace or started its dictionary afresh)
    if (!ok || K.wide || !var_current(l) || !var_current(r) || out->epoch != K.epoch)
        return fallback(S);
    *verdict = LASPJ_NIF_OK;
    if (!K.dict || dict_elements(K.dict) == 0) return LASPJ_OK;      // three empty values
    if (int s = lvar_images(ctx, S, K)) return s;
    const uint32_t n = K.built_K;
    const uint64_t ub_t = std::max<uint64_t>(2ull * K.built_toks, 1);
    if (ub_t > 0xFFFFFFF0ull) return fail(ctx, LASPJ_E_RANGE, "lvar_intersection: too many tokens");
    const uint64_t t0 = now_ns();
    if (ctx->tune_lvar == 1) {
        // the two-step composition (A/B): l's list form, then the intersection with r's cells
        {
            Guard g(ctx);
            if (int s = lvar_ranks(ctx, S, K)) return s;
            if (int s = fit_var(ctx, l, K.E, 1)) return s;
            if (int s = fit_var(ctx, r, K.E, 1)) return s;
        }
        if (!out->tmp)
            if (int s = laspj_list_batch_create(ctx, LASPJ_KIND_ORSET_LIST, 1, 1, 1, &out->tmp))
                return s;
        laspj_buf eo, to;
        eo.ctx = to.ctx = ctx;
        eo.dev = const_cast<uint32_t*>(etf_dict_elem_order(K.etf));
        eo.bytes = 4ull * K.E;
        to.dev = const_cast<uint8_t*>(etf_dict_tok_order(K.etf));
        to.bytes = 64ull * K.E;
        const laspj_batch lb = view(ctx, LASPJ_KIND_ORSET, 1, K.E, l->cells);
        const laspj_batch rb = view(ctx, LASPJ_KIND_ORSET, 1, K.E, r->cells);
        if (int s = laspj_list_from_set(ctx, out->tmp, &lb, &eo, n, &to)) return s;
        if (int s = laspj_list_intersection_set(ctx, out->val, out->tmp, &rb, &to)) return s;
    } else {
        Guard g(ctx);
        if (int s = lvar_ranks(ctx, S, K)) return s;
        const uint32_t ntile = lv_isect_tiles(n);
        if (int s = lvar_scratch(ctx, S, ntile)) return s;
        if (int s = list_reserve(ctx, out->val, std::max(n, 1u), (uint32_t)ub_t)) return s;
        LvIsect a;
        a.l = l->cells;
        a.r = r->cells;
        a.El = l->cells ? l->E : 0;
        a.Er = r->cells ? r->E : 0;
        a.elem_order = etf_dict_elem_order(K.etf);
        a.n = n;
        a.grank = static_cast<const uint32_t*>(K.grank);
        S->lv_ans[2] = 2;                                   // (not written yet)
        LJ_HIP(ctx, launch_lv_isect(ctx, a, list_dev(out->val),
                                    static_cast<uint64_t*>(S->lv_tiles), S->lv_ans_d));
        // upper bounds until the bind's synchronisation brings the totals
        out->val->known_e = std::min(out->val->cap_e, std::max(n, 1u));
        out->val->known_t = (uint32_t)std::min<uint64_t>(out->val->cap_t, ub_t);
        out->val->not_asc = false;                          // term-order positions: keys ascend
        out->val->no_spec = false;
    }
    S->stats[ST_NS_ENQUEUE] += now_ns() - t0;
    int32_t st = 0;
    if (int s = lvar_bind(ctx, S, out, &st, tail, met)) return s;
    if (ctx->tune_lvar != 1) {
        if (S->lv_ans[2] != 0)
            return fail(ctx, LASPJ_E_RANGE, "lvar_intersection: the producer's output bound did "
                        "not hold (%u entries, %u tokens)", S->lv_ans[0], S->lv_ans[1]);
        out->val->known_e = S->lv_ans[0];
        out->val->known_t = S->lv_ans[1];
    }
    if (st == LASPJ_BIND_WRITTEN) llazy_clear(out);      // write/4: a fresh #dv (:842-843)
    *status = st;
    return LASPJ_OK;
}

// laspj_lvar_product with S->mu held and the handles checked
int lvar_product_locked(laspj_ctx* ctx, NifState* S, laspj_lvar* out, laspj_var* l, laspj_var* r,
                        int32_t* status, int32_t* verdict,
                        const std::vector<ListWaiter>* tail = nullptr, uint8_t* met = nullptr) {
    ++S->stats[ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    if (!out->pairs || l->kind != LASPJ_KIND_ORSET || r->kind != LASPJ_KIND_ORSET ||
        l->ns != out->ns || r->ns != out->ns)
        return fallback(S);
    KindState& K = *out->ns;
    if (K.wide) return fallback(S);
    for (laspj_var* v : {l, r}) {
        bool ok = false;
        if (int s = hydrate(ctx, S, v, &ok)) return s;
        if (!ok) return fallback(S);
    }
    bool ok = false;
    if (int s = lvar_ready(ctx, S, out, &ok)) return s;
    // (a decode above may have widened the namespace or started its dictionary afresh)
    if (!ok || K.wide || !var_current(l) || !var_current(r) || out->epoch != K.epoch)
        return fallback(S);
    *verdict = LASPJ_NIF_OK;
    if (!K.dict || dict_elements(K.dict) == 0) return LASPJ_OK;      // three empty values
    if (int s = lvar_images(ctx, S, K)) return s;
    const uint32_t n = K.built_K;
    const uint64_t cap_t = std::max<uint64_t>(K.built_toks, 1);
    if (cap_t > 0xFFFFFFF0ull) return fail(ctx, LASPJ_E_RANGE, "lvar_product: too many tokens");
    const uint64_t t0 = now_ns();
    {
        Guard g(ctx);
        if (int s = lvar_ranks(ctx, S, K)) return s;
        const uint32_t ntile = lv_isect_tiles(n);
        if (int s = lvar_scratch(ctx, S, 2 * ntile)) return s;
        // per side: [slot n | tpre n + 1 | own cap_t] words (to 8 bytes), then run cap_t u64
        const uint64_t words = ((uint64_t)n + (n + 1ull) + cap_t + 1) & ~1ull;
        const uint64_t side = 4 * words + 8 * cap_t;
        if (int s = grow_dev(ctx, &S->lp_side, &S->lp_side_bytes, 2 * side)) return s;
        LvProd a;
        for (int k = 0; k < 2; ++k) {
            const laspj_var* v = k ? r : l;
            char* base = static_cast<char*>(S->lp_side) + k * side;
            a.s[k].cells = v->cells;
            a.s[k].E = v->cells ? v->E : 0;
            a.s[k].slot = reinterpret_cast<uint32_t*>(base);
            a.s[k].tpre = a.s[k].slot + n;
            a.s[k].own = a.s[k].tpre + n + 1;
            a.s[k].run = reinterpret_cast<uint64_t*>(base + 4 * words);
        }
        a.elem_order = etf_dict_elem_order(K.etf);
        a.n = n;
        a.cap_t = (uint32_t)cap_t;
        a.grank = static_cast<const uint32_t*>(K.grank);
        S->lv_ans[4] = S->lv_ans[5] = 2;                    // (not written yet)
        LJ_HIP(ctx, launch_lp_sides(ctx, a, static_cast<uint64_t*>(S->lv_tiles), S->lv_ans_d));
        // the one small synchronisation the sizes cost: |L| x |R| has no useful a-priori bound
        LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (S->lv_ans[4] != 0 || S->lv_ans[5] != 0)
            return fail(ctx, LASPJ_E_RANGE, "lvar_product: a side's token bound did not hold "
                        "(%u and %u tokens)", S->lv_ans[1], S->lv_ans[3]);
        const uint32_t nl = S->lv_ans[0], TL = S->lv_ans[1], nr = S->lv_ans[2], TR = S->lv_ans[3];
        const uint64_t NE = (uint64_t)nl * nr, NT = (uint64_t)TL * TR;
        if (NE > 0xFFFFFFF0ull || NT > 0xFFFFFFF0ull)
            return fail(ctx, LASPJ_E_RANGE, "lvar_product: %llu entries, %llu tokens",
                        (unsigned long long)NE, (unsigned long long)NT);
        if (int s = list_reserve(ctx, out->val, (uint32_t)std::max<uint64_t>(NE, 1),
                                 (uint32_t)std::max<uint64_t>(NT, 1)))
            return s;
        S->lv_ans[6] = 2;
        LJ_HIP(ctx, launch_lp_write(ctx, a, nl, nr, TL, TR, list_dev(out->val), S->lv_ans_d));
        out->val->known_e = (uint32_t)NE;
        out->val->known_t = (uint32_t)NT;
        out->val->not_asc = true;           // (pairs: the general bind, see lvar_bind)
        out->val->no_spec = false;
    }
    S->stats[ST_NS_ENQUEUE] += now_ns() - t0;
    int32_t st = 0;
    if (int s = lvar_bind(ctx, S, out, &st, tail, met)) return s;
    if (S->lv_ans[6] != 0)
        return fail(ctx, LASPJ_E_RANGE, "lvar_product: the output's capacity did not hold");
    if (st == LASPJ_BIND_WRITTEN) llazy_clear(out);      // write/4: a fresh #dv (:842-843)
    *status = st;
    return LASPJ_OK;
}

// an image walked into lv->val over the namespace (its unseen terms registered, the images
// and tables brought up to them); *ok false: the walk refused it (its registrations undone)
// into (or null: lv->val): the list that takes the items
int lvar_walk_val(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, const uint8_t* p, uint64_t n,
                  bool* ok, laspj_batch* into = nullptr) {
    KindState& K = *lv->ns;
    *ok = false;
    if (!K.dict)
        if (int s = reset_dict(ctx, S, K)) return s;
    const RegMark m = reg_mark(K);
    ListItems it;
    const uint64_t t0 = now_ns();
    const int st = lvar_walk_image(K.dict, lv->pairs, p, n, &it);
    S->stats[ST_NS_REGISTER] += now_ns() - t0;
    if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "lvar: host allocation");
    if (st != LASPJ_DEC_OK) return LASPJ_OK;
    reg_note(S, K, m);
    if (int s = lvar_prepare(ctx, S, K)) return s;
    if (int s = lvar_upload(ctx, into ? into : lv->val, it)) return s;
    *ok = true;
    return LASPJ_OK;
}

// threshold_met(lasp_orset, #dv.value, T) (lasp_lattice.erl:62-75) for the threshold walked
// into lv->val: is_inflation / is_strict_inflation of it -> the value, one device pass
int lvar_val_met(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, int strict, uint8_t* met) {
    const LvOrder ord(ctx, *lv->ns);
    laspj_buf* res = nullptr;
    if (int s = laspj_buf_create(ctx, 8, &res)) return s;
    uint8_t b = 0;
    int s = laspj_list_inflation(ctx, lv->val, lv->list, strict ? 1 : 0, &ord.o, res);
    if (s == LASPJ_OK) s = laspj_buf_download(ctx, res, 0, &b, 1);
    laspj_buf_destroy(res);
    if (s) return s;
    ++S->stats[ST_PASSES];
    *met = b;
    return LASPJ_OK;
}

// The threshold walked into *list (lv->val, or a read_any's list of its own) becomes the
// device list of a new entry {id, strict, image} at the tail of `es` — the variable's waiters
// (lasp_core.erl:355-364) or its lazy threads (:747-755) — and a fresh block takes its place
// (fresh false: *list is the caller's to give away, and comes back null).
int lvar_keep(laspj_ctx* ctx, laspj_lvar* lv, std::vector<LWaiter>& es, laspj_batch** list,
              bool fresh, uint64_t id, int strict, const uint8_t* image, uint64_t n) {
    LWaiter w;
    w.id = id;
    w.strict = strict ? 1 : 0;
    w.image.assign(image, image + n);
    w.n = (*list)->known_e;
    w.epoch = lv->ns->epoch;
    es.reserve(es.size() + 1);
    laspj_batch* next = nullptr;
    if (fresh)
        if (int c = laspj_list_batch_create(ctx, LASPJ_KIND_ORSET_LIST, 1, 1, 1, &next)) return c;
    w.list = *list;
    *list = next;
    es.push_back(std::move(w));
    return LASPJ_OK;
}

// *ok: every threshold of `es` (the variable's waiters, or its lazy threads) is on the device
// over the current dictionary.  One whose list a dictionary reset made stale is walked back
// in from its image here (its terms registered afresh: the caller brings the images and
// tables up to them); in a wide namespace, or when the walk refuses an image, the lists stay
// as they are.  S->mu held.
int lentries_ready(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, std::vector<LWaiter>& es,
                   bool* ok) {
    KindState& K = *lv->ns;
    *ok = !K.wide;
    if (K.wide) return LASPJ_OK;
    for (LWaiter& w : es) {
        if (w.list && w.epoch == K.epoch) continue;
        if (!K.dict)
            if (int s = reset_dict(ctx, S, K)) return s;
        const RegMark m = reg_mark(K);
        ListItems it;
        const int st = lvar_walk_image(K.dict, lv->pairs, w.image.data(), w.image.size(), &it);
        if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "lvar: host allocation");
        if (st != LASPJ_DEC_OK) {
            *ok = false;
            return LASPJ_OK;
        }
        reg_note(S, K, m);
        if (!w.list)
            if (int s = laspj_list_batch_create(ctx, LASPJ_KIND_ORSET_LIST, 1, 1, 1, &w.list))
                return s;
        if (int s = lvar_upload(ctx, w.list, it)) return s;
        w.n = (uint32_t)it.keys.size();
        w.epoch = K.epoch;
        ++S->stats[ST_HYDRATED];
    }
    return LASPJ_OK;
}
int lwaiters_ready(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, bool* ok) {
    return lentries_ready(ctx, S, lv, lv->waiters, ok);
}
int llazy_ready(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, bool* ok) {
    return lentries_ready(ctx, S, lv, lv->lazy, ok);
}

// the waiters as the check pass takes them, in list order
std::vector<ListWaiter> lwaiter_descs(const laspj_lvar* lv) {
    std::vector<ListWaiter> d;
    d.reserve(lv->waiters.size());
    for (const LWaiter& w : lv->waiters) d.push_back(ListWaiter{w.list, w.n, (uint32_t)w.strict});
    return d;
}

// reply_to_all's outcome (lasp_core.erl:795-825): the met waiters' ids in list order,
// removed — the others keep their order — unless more than cap are met
void lwaiters_take(laspj_lvar* lv, const uint8_t* met, uint64_t* ids, uint32_t cap,
                   uint32_t* nmet) {
    std::vector<LWaiter>& ws = lv->waiters;
    uint32_t total = 0;
    for (size_t k = 0; k < ws.size(); ++k) total += met[k] ? 1u : 0u;
    *nmet = total;
    if (!total || total > cap || !ids) return;
    size_t keep = 0, at = 0;
    for (size_t k = 0; k < ws.size(); ++k) {
        if (met[k]) {
            ids[at++] = ws[k].id;
            lwaiter_release(ws[k]);
        } else {
            if (keep != k) ws[keep] = std::move(ws[k]);
            ++keep;
        }
    }
    ws.resize(keep);
}

}  // namespace

int spill_lvars(NifState* S, KindState& K) {
    for (laspj_lvar* lv : K.lvars) {
        if (int s = lvar_spill(S, lv)) return s;
        // the waiters' lists name the same slots: released, their images kept
        for (LWaiter& w : lv->waiters) lwaiter_release(w);
        for (LWaiter& z : lv->lazy) lwaiter_release(z);
    }
    return LASPJ_OK;
}

}  // namespace laspj

namespace {

// the variable's context state; null: the context is gone
laspj::NifState* lvar_state(laspj_lvar* lv) {
    if (!lv || !lv->ctx) return nullptr;
    return laspj::state(lv->ctx);
}

// (S->mu held) the handle is a live list variable of this context
bool lvar_alive(const laspj::NifState* S, laspj_lvar* lv) { return lv && S->lvars.count(lv); }

// a list variable call's opening (laspj::enter, then the handle checked under the call lock)
laspj::Entry enter_lvar(laspj_lvar* lv, const char* name, bool args_ok) {
    laspj::Entry e = laspj::enter(lvar_state(lv), lv ? lv->ctx : nullptr, name, args_ok);
    if (e.rc == LASPJ_OK && !lvar_alive(e.S, lv)) e.rc = laspj::unknown_variable(e.ctx, name);
    return e;
}

void lvar_free_batches(laspj_lvar* lv) {
    for (laspj_batch** b : {&lv->list, &lv->val, &lv->dst, &lv->tmp}) {
        if (*b) laspj_batch_destroy(*b);
        *b = nullptr;
    }
    for (laspj::LWaiter& w : lv->waiters) laspj::lwaiter_release(w);
    for (laspj::LWaiter& z : lv->lazy) laspj::lwaiter_release(z);
}

// laspj_lvar_create / laspj_lvar_create_pairs
int lvar_create(laspj_var* peer, laspj_lvar** out, bool pairs) {
    if (!peer || !out) return LASPJ_E_INVAL;
    *out = nullptr;
    if (peer->gc) {
        laspj_ctx* c = laspj::gc_var_ctx(peer->gc);
        return c ? fail(c, LASPJ_E_KIND, "lvar_create: an OR-Set variable's namespace") : LASPJ_E_KIND;
    }
    const laspj::Entry e = laspj::enter_var(peer, "lvar_create", true);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    if (peer->kind != LASPJ_KIND_ORSET)
        return fail(ctx, LASPJ_E_KIND, "lvar_create: an OR-Set variable's namespace");
    auto* lv = new (std::nothrow) laspj_lvar;
    if (!lv) return fail(ctx, LASPJ_E_NOMEM, "lvar_create: host allocation");
    lv->ctx = ctx;
    lv->ns = peer->ns;
    lv->epoch = peer->ns->epoch;
    lv->pairs = pairs;
    for (laspj_batch** b : {&lv->list, &lv->val, &lv->dst})
        if (int s = laspj_list_batch_create(ctx, LASPJ_KIND_ORSET_LIST, 1, 1, 1, b)) {
            lvar_free_batches(lv);
            delete lv;
            return s;
        }
    const int s = laspj::nomem_guard(ctx, "lvar_create", [&] {
        S->lvars.insert(lv);
        try {
            lv->ns->lvars.insert(lv);
        } catch (const std::bad_alloc&) {
            S->lvars.erase(lv);
            throw;
        }
        return LASPJ_OK;
    }, "registry");
    if (s) {
        lvar_free_batches(lv);
        delete lv;
        return s;
    }
    // (patches before this variable were not recorded for the tables)
    lv->ns->rank_full = true;
    *out = lv;
    return LASPJ_OK;
}

}  // namespace

extern "C" {

int laspj_lvar_create(laspj_var* peer, laspj_lvar** out) { return lvar_create(peer, out, false); }

int laspj_lvar_create_pairs(laspj_var* peer, laspj_lvar** out) {
    return lvar_create(peer, out, true);
}

int laspj_lvar_destroy(laspj_lvar* lv) {
    if (!lv) return LASPJ_E_INVAL;
    if (laspj::NifState* S = lvar_state(lv)) {
        std::lock_guard<std::mutex> lk(S->mu);
        if (lv->ctx) {
            S->lvars.erase(lv);
            lv->ns->lvars.erase(lv);
            laspj::maps_lvar_gone(S, lv);        // a map writing into it is dead from here on
            laspj::folds_lvar_gone(S, lv);       // a fold, likewise
            lvar_free_batches(lv);
            // the namespace's last holder: its dictionary, device images and tables go too
            if (lv->ns.use_count() == 1) laspj::free_ns(*lv->ns);
        }
    }
    if (!lv->ctx && lv->ns && lv->ns.use_count() == 1 && lv->ns->dict) {
        laspj_dict_destroy(lv->ns->dict);        // (its device side went with the context)
        lv->ns->dict = nullptr;
    }
    delete lv;
    return LASPJ_OK;
}

int laspj_lvar_intersection(laspj_lvar* out, laspj_var* l, laspj_var* r, int32_t* status,
                            int32_t* verdict) {
    if (!l || !r) return LASPJ_E_INVAL;
    const laspj::Entry e = enter_lvar(out, "lvar_intersection", status && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    if (l->gc || r->gc || l->ctx != ctx || r->ctx != ctx || !S->vars.count(l) || !S->vars.count(r)) {
        // a counter, a variable of another context: nothing this body runs over
        ++S->stats[laspj::ST_CALLS];
        return laspj::fallback(S);
    }
    return laspj::nomem_guard(ctx, "lvar_intersection", [&] {
        return laspj::lvar_intersection_locked(ctx, S, out, l, r, status, verdict);
    });
}

int laspj_lvar_etf_bind(laspj_lvar* lv, const uint8_t* value, uint64_t n, int32_t* status,
                        int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_bind", value && n && status && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_bind", [&]() -> int {
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (ok)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, value, n, &ok)) return s;
        if (!ok) return laspj::fallback(S);
        int32_t st = 0;
        if (int s = laspj::lvar_bind(ctx, S, lv, &st)) return s;
        if (st == LASPJ_BIND_WRITTEN) laspj::llazy_clear(lv);    // write/4: a fresh #dv
        *status = st;
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    });
}

int laspj_lvar_etf_write(laspj_lvar* lv, const uint8_t* value, uint64_t n, int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_write", value && n && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_write", [&]() -> int {
        laspj::KindState& K = *lv->ns;
        bool ok = false;
        if (!K.wide)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, value, n, &ok)) return s;
        laspj::llazy_clear(lv);                          // write/4: a fresh #dv (:842-843)
        if (!ok) {
            // held as its image: read answers it, the other calls FALLBACK until a write
            lv->image.assign(value, value + n);
            lv->resident = false;
            lv->held = true;
            return laspj::fallback(S);
        }
        std::swap(lv->list, lv->val);
        lv->resident = true;
        lv->held = false;
        lv->epoch = K.epoch;
        lv->image.clear();
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    });
}

int laspj_lvar_etf_read(laspj_lvar* lv, const uint8_t** out, uint64_t* out_len,
                        int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_read", out && out_len && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *verdict = LASPJ_NIF_OK;
    return laspj::nomem_guard(ctx, "lvar_read", [&]() -> int {
        laspj::KindState& K = *lv->ns;
        if (!(lv->resident && lv->epoch == K.epoch)) {
            // host-held: the image as it was written out (or written)
            if (lv->image.empty()) S->lv_out.assign({(char)131, (char)106});
            else S->lv_out.assign(lv->image.begin(), lv->image.end());
        } else {
            laspj::ListItems it;
            if (int s = laspj::lvar_download(ctx, lv->list, &it)) return s;
            if (it.keys.empty()) {
                S->lv_out.assign({(char)131, (char)106});
            } else if (int s = laspj::list_write(K.dict, LASPJ_KIND_ORSET, it, &S->lv_out)) {
                return fail(ctx, s, "lvar_read: image");
            }
        }
        *out = reinterpret_cast<const uint8_t*>(S->lv_out.data());
        *out_len = S->lv_out.size();
        return LASPJ_OK;
    });
}

int laspj_lvar_etf_value(laspj_lvar* lv, const uint8_t** out, uint64_t* out_len,
                         int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_value", out && out_len && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_value", [&]() -> int {
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (!ok) return laspj::fallback(S);
        laspj::KindState& K = *lv->ns;
        laspj_batch* gv = nullptr;                       // value/1 is a list of keys
        if (int s = laspj_list_batch_create(ctx, LASPJ_KIND_GSET_LIST, 1, 1, 1, &gv)) return s;
        laspj::ListItems it;
        int s = laspj_list_value(ctx, gv, lv->list);
        if (s == LASPJ_OK) s = laspj::lvar_download(ctx, gv, &it);
        laspj_batch_destroy(gv);
        if (s) return s;
        if (it.keys.empty()) {
            S->lv_out.assign({(char)131, (char)106});
        } else if (int w = laspj::list_write(K.dict, LASPJ_KIND_GSET, it, &S->lv_out)) {
            return fail(ctx, w, "lvar_value: image");
        }
        *out = reinterpret_cast<const uint8_t*>(S->lv_out.data());
        *out_len = S->lv_out.size();
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    });
}

int laspj_lvar_etf_threshold(laspj_lvar* lv, const uint8_t* threshold, uint64_t n, int strict,
                             int32_t* result, int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_threshold", threshold && n && result && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *result = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_threshold", [&]() -> int {
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (ok)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, threshold, n, &ok)) return s;
        if (!ok) return laspj::fallback(S);
        uint8_t b = 0;
        if (int s = laspj::lvar_val_met(ctx, S, lv, strict, &b)) return s;
        *result = b ? 1 : 0;
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    });
}

int laspj_lvar_wait(laspj_lvar* lv, const uint8_t* threshold, uint64_t n, int strict, uint64_t id,
                    int32_t* met, int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_wait", threshold && n && met && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *met = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_wait", [&]() -> int {
        bool ok = false, wok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        // (stale waiters come back ahead of the threshold's walk, which brings the images up
        // to every term registered; one the walk refuses waits for recheck's FALLBACK)
        if (ok)
            if (int s = laspj::lwaiters_ready(ctx, S, lv, &wok)) return s;
        if (ok)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, threshold, n, &ok)) return s;
        if (!ok) return laspj::fallback(S);
        // threshold_met (lasp_lattice.erl:62-75) as laspj_lvar_etf_threshold answers it
        uint8_t b = 0;
        if (int s = laspj::lvar_val_met(ctx, S, lv, strict, &b)) return s;
        if (b) {
            *met = 1;
            *verdict = LASPJ_NIF_OK;
            return LASPJ_OK;
        }
        // unmet (lasp_core.erl:355-364): appended to waiting_threads; the walked threshold
        // (lv->val) becomes the waiter's list, a fresh block takes its place
        if (int c = laspj::lvar_keep(ctx, lv, lv->waiters, &lv->val, true, id, strict, threshold, n))
            return c;
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    });
}

int laspj_lvar_recheck(laspj_lvar* lv, uint64_t* ids, uint32_t cap, uint32_t* nmet,
                       uint32_t* nwaiting, int32_t* verdict) {
    const laspj::Entry e =
        enter_lvar(lv, "lvar_recheck", (ids || !cap) && nmet && nwaiting && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *nmet = 0;
    *nwaiting = (uint32_t)lv->waiters.size();
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_recheck", [&]() -> int {
        laspj::KindState& K = *lv->ns;
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (ok)
            if (int s = laspj::lwaiters_ready(ctx, S, lv, &ok)) return s;
        if (!ok || K.wide || lv->epoch != K.epoch) return laspj::fallback(S);
        *verdict = LASPJ_NIF_OK;
        if (lv->waiters.empty()) return LASPJ_OK;
        if (int s = laspj::lvar_prepare(ctx, S, K)) return s;
        const std::vector<laspj::ListWaiter> ws = laspj::lwaiter_descs(lv);
        std::vector<uint8_t> met(ws.size(), 0);
        const laspj::LvOrder ord(ctx, K);
        const uint64_t t0 = laspj::now_ns();
        if (int s = laspj::list_waiters_check(ctx, lv->list, &ord.o, ws.data(),
                                              (uint32_t)ws.size(), met.data()))
            return s;
        ++S->stats[laspj::ST_PASSES];
        S->stats[laspj::ST_NS_WAIT] += laspj::now_ns() - t0;
        laspj::lwaiters_take(lv, met.data(), ids, cap, nmet);
        *nwaiting = (uint32_t)lv->waiters.size();
        return LASPJ_OK;
    });
}

int laspj_lvar_intersection_recheck(laspj_lvar* out, laspj_var* l, laspj_var* r, int32_t* status,
                                    uint64_t* ids, uint32_t cap, uint32_t* nmet,
                                    uint32_t* nwaiting, int32_t* verdict) {
    if (!l || !r) return LASPJ_E_INVAL;
    const laspj::Entry e = enter_lvar(out, "lvar_intersection_recheck",
                                      status && (ids || !cap) && nmet && nwaiting && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    *nmet = 0;
    *nwaiting = (uint32_t)out->waiters.size();
    if (l->gc || r->gc || l->ctx != ctx || r->ctx != ctx || !S->vars.count(l) || !S->vars.count(r)) {
        ++S->stats[laspj::ST_CALLS];
        return laspj::fallback(S);
    }
    return laspj::nomem_guard(ctx, "lvar_intersection_recheck", [&]() -> int {
        // the waiters' thresholds on the device first: what their walk registers joins the
        // dictionary ahead of the images the producer and the bind run over
        bool ok = false, wok = false;
        if (int s = laspj::lvar_ready(ctx, S, out, &ok)) return s;
        if (ok)
            if (int s = laspj::lwaiters_ready(ctx, S, out, &wok)) return s;
        const bool tail = wok && !out->waiters.empty();
        const std::vector<laspj::ListWaiter> ws =
            tail ? laspj::lwaiter_descs(out) : std::vector<laspj::ListWaiter>();
        std::vector<uint8_t> met(ws.size(), 0);
        if (int s = laspj::lvar_intersection_locked(ctx, S, out, l, r, status, verdict,
                                                    tail ? &ws : nullptr, met.data()))
            return s;
        // NOOP, REFUSED, FALLBACK: the value is as it was, so no registered waiter became met
        if (*verdict != LASPJ_NIF_OK || *status != LASPJ_BIND_WRITTEN || out->waiters.empty())
            return LASPJ_OK;
        if (!tail) {
            // written, the waiters not checked (an image the walk refuses): the NIF's walk
            *verdict = LASPJ_NIF_FALLBACK;
            return laspj::fallback(S);
        }
        laspj::lwaiters_take(out, met.data(), ids, cap, nmet);
        *nwaiting = (uint32_t)out->waiters.size();
        return LASPJ_OK;
    });
}

int laspj_lvar_product(laspj_lvar* out, laspj_var* l, laspj_var* r, int32_t* status,
                       int32_t* verdict) {
    if (!l || !r) return LASPJ_E_INVAL;
    const laspj::Entry e = enter_lvar(out, "lvar_product", status && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    if (l->gc || r->gc || l->ctx != ctx || r->ctx != ctx || !S->vars.count(l) || !S->vars.count(r)) {
        // a counter, a variable of another context: nothing this body runs over
        ++S->stats[laspj::ST_CALLS];
        return laspj::fallback(S);
    }
    return laspj::nomem_guard(ctx, "lvar_product", [&] {
        return laspj::lvar_product_locked(ctx, S, out, l, r, status, verdict);
    });
}

int laspj_lvar_product_recheck(laspj_lvar* out, laspj_var* l, laspj_var* r, int32_t* status,
                               uint64_t* ids, uint32_t cap, uint32_t* nmet, uint32_t* nwaiting,
                               int32_t* verdict) {
    if (!l || !r) return LASPJ_E_INVAL;
    const laspj::Entry e = enter_lvar(out, "lvar_product_recheck",
                                      status && (ids || !cap) && nmet && nwaiting && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    *nmet = 0;
    *nwaiting = (uint32_t)out->waiters.size();
    if (l->gc || r->gc || l->ctx != ctx || r->ctx != ctx || !S->vars.count(l) || !S->vars.count(r)) {
        ++S->stats[laspj::ST_CALLS];
        return laspj::fallback(S);
    }
    return laspj::nomem_guard(ctx, "lvar_product_recheck", [&]() -> int {
        // the waiters' thresholds on the device first, as laspj_lvar_intersection_recheck
        bool ok = false, wok = false;
        if (int s = laspj::lvar_ready(ctx, S, out, &ok)) return s;
        if (ok)
            if (int s = laspj::lwaiters_ready(ctx, S, out, &wok)) return s;
        const bool tail = wok && !out->waiters.empty();
        const std::vector<laspj::ListWaiter> ws =
            tail ? laspj::lwaiter_descs(out) : std::vector<laspj::ListWaiter>();
        std::vector<uint8_t> met(ws.size(), 0);
        if (int s = laspj::lvar_product_locked(ctx, S, out, l, r, status, verdict,
                                               tail ? &ws : nullptr, met.data()))
            return s;
        // NOOP, REFUSED, FALLBACK: the value is as it was, so no registered waiter became met
        if (*verdict != LASPJ_NIF_OK || *status != LASPJ_BIND_WRITTEN || out->waiters.empty())
            return LASPJ_OK;
        if (!tail) {
            // written, the waiters not checked (an image the walk refuses): the NIF's walk
            *verdict = LASPJ_NIF_FALLBACK;
            return laspj::fallback(S);
        }
        laspj::lwaiters_take(out, met.data(), ids, cap, nmet);
        *nwaiting = (uint32_t)out->waiters.size();
        return LASPJ_OK;
    });
}

int laspj_lvar_wait_cancel(laspj_lvar* lv, uint64_t id, int32_t* found) {
    const laspj::Entry e = enter_lvar(lv, "lvar_wait_cancel", found != nullptr);
    if (e.rc) return e.rc;
    *found = 0;
    std::vector<laspj::LWaiter>& ws = lv->waiters;
    for (size_t k = 0; k < ws.size(); ++k)
        if (ws[k].id == id) {
            laspj::lwaiter_release(ws[k]);
            ws.erase(ws.begin() + (ptrdiff_t)k);
            *found = 1;
            break;
        }
    return LASPJ_OK;
}

int laspj_lvar_waiter_count(const laspj_lvar* lv, uint32_t* n) {
    laspj::NifState* S = lvar_state(const_cast<laspj_lvar*>(lv));
    if (!S || !n) return LASPJ_E_INVAL;
    std::lock_guard<std::mutex> lk(S->mu);
    *n = (uint32_t)lv->waiters.size();
    return LASPJ_OK;
}

int laspj_lvar_waiter_at(laspj_lvar* lv, uint32_t k, uint64_t* id, int32_t* strict,
                         const uint8_t** threshold, uint64_t* n) {
    const laspj::Entry e = laspj::enter(lvar_state(lv), lv ? lv->ctx : nullptr, "lvar_waiter_at",
                                        id && strict && threshold && n);
    if (e.rc) return e.rc;
    if (k >= lv->waiters.size())
        return fail(e.ctx, LASPJ_E_RANGE, "lvar_waiter_at: no waiter %u", k);
    *id = lv->waiters[k].id;
    *strict = lv->waiters[k].strict;
    *threshold = lv->waiters[k].image.data();
    *n = lv->waiters[k].image.size();
    return LASPJ_OK;
}

int laspj_lvar_wait_needed(laspj_lvar* lv, const uint8_t* threshold, uint64_t n, int strict,
                           uint64_t id, int32_t* needed, int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_wait_needed", threshold && n && needed && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *needed = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_wait_needed", [&]() -> int {
        bool ok = false, wok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        // (stale waiters and lazy threads come back ahead of the threshold's walk, as in
        // laspj_lvar_wait; one the walk refuses waits for the call that checks it)
        if (ok)
            if (int s = laspj::lwaiters_ready(ctx, S, lv, &wok)) return s;
        if (ok)
            if (int s = laspj::llazy_ready(ctx, S, lv, &wok)) return s;
        if (ok)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, threshold, n, &ok)) return s;
        if (!ok) return laspj::fallback(S);
        uint8_t b = 0;
        if (int s = laspj::lvar_val_met(ctx, S, lv, strict, &b)) return s;
        // met (lasp_core.erl:735-737), or somebody is reading already (:739-741)
        if (b || !lv->waiters.empty()) {
            *needed = 1;
            *verdict = LASPJ_NIF_OK;
            return LASPJ_OK;
        }
        // the stored {strict, T} would later be handed to keyfind as a value (:798)
        if (strict) return laspj::fallback(S);
        // :747-755: appended to lazy_threads; lv->val becomes the entry's list
        if (int c = laspj::lvar_keep(ctx, lv, lv->lazy, &lv->val, true, id, 0, threshold, n))
            return c;
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    });
}

namespace {

// a read_any's own threshold lists, destroyed unless a waiter took them
struct OwnLists {
    std::vector<laspj_batch*> v;
    ~OwnLists() {
        for (laspj_batch* b : v)
            if (b) laspj_batch_destroy(b);
    }
};

// laspj_lvar_read (n = 1, the threshold walked into lvs[0]->val) and laspj_lvar_read_any (a
// list of its own per read) with S->mu held and the handles checked
int lreads_locked(laspj_ctx* ctx, laspj::NifState* S, uint32_t n, laspj_lvar* const* lvs,
                  const uint8_t* const* thresholds, const uint64_t* lens, const int32_t* strict,
                  bool own, uint64_t id, int32_t* found, uint64_t* lazy_ids, uint32_t cap,
                  uint32_t* nlazy, int32_t* verdict) {
    using namespace laspj;
    // the distinct variables, in the order named
    std::vector<laspj_lvar*> vars;
    std::vector<uint32_t> var_of(n);
    for (uint32_t i = 0; i < n; ++i) {
        const auto at = std::find(vars.begin(), vars.end(), lvs[i]);
        var_of[i] = (uint32_t)(at - vars.begin());
        if (at == vars.end()) vars.push_back(lvs[i]);
    }
    // values, waiters and lazy threads on the device first, then the thresholds' walks, which
    // bring the images and tables up to every term registered
    for (laspj_lvar* lv : vars) {
        bool ok = false, wok = false;
        if (int s = lvar_ready(ctx, S, lv, &ok)) return s;
        if (!ok) return fallback(S);
        if (int s = lwaiters_ready(ctx, S, lv, &wok)) return s;
        if (int s = llazy_ready(ctx, S, lv, &ok)) return s;
        if (!ok) return fallback(S);       // a stale lazy entry whose image the walk refuses
    }
    OwnLists mine;
    std::vector<ListWaiter> reads(n);
    for (uint32_t i = 0; i < n; ++i) {
        laspj_lvar* lv = lvs[i];
        laspj_batch* into = nullptr;
        if (own) {
            mine.v.push_back(nullptr);
            if (int s = laspj_list_batch_create(ctx, LASPJ_KIND_ORSET_LIST, 1, 1, 1, &mine.v.back()))
                return s;
            into = mine.v.back();
        }
        bool ok = false;
        if (int s = lvar_walk_val(ctx, S, lv, thresholds[i], lens[i], &ok, into)) return s;
        if (!ok) return fallback(S);
        const laspj_batch* t = into ? into : lv->val;
        reads[i] = ListWaiter{t, t->known_e, strict[i] ? 1u : 0u};
    }
    for (laspj_lvar* lv : vars) {
        const KindState& K = *lv->ns;
        if (K.wide || !lv->resident || lv->epoch != K.epoch) return fallback(S);
        for (const LWaiter& z : lv->lazy)
            if (!z.list || z.epoch != K.epoch) return fallback(S);
    }
    // read i's pairs: its variable's value, then that variable's lazy thresholds in list
    // order; one pass per namespace named (its order tables are the pass's)
    std::vector<uint32_t> nl(vars.size()), pair0(n + 1, 0);
    for (size_t v = 0; v < vars.size(); ++v) nl[v] = (uint32_t)vars[v]->lazy.size();
    for (uint32_t i = 0; i < n; ++i) pair0[i + 1] = pair0[i] + 1 + nl[var_of[i]];
    std::vector<uint8_t> met(pair0[n], 0);
    std::vector<uint8_t> done(n, 0);
    for (uint32_t first = 0; first < n; ++first) {
        if (done[first]) continue;
        KindState& K = *lvs[first]->ns;
        std::vector<ListWaiter> rd;
        std::vector<ListReadCur> curs;
        std::vector<ListReadPair> pairs;
        std::vector<uint32_t> cur0(vars.size(), ~0u), where;
        for (uint32_t i = first; i < n; ++i) {
            if (done[i] || lvs[i]->ns.get() != &K) continue;
            done[i] = 1;
            const uint32_t v = var_of[i];
            if (cur0[v] == ~0u) {
                cur0[v] = (uint32_t)curs.size();
                curs.push_back(ListReadCur{vars[v]->list, vars[v]->list->known_e});
                for (const LWaiter& z : vars[v]->lazy) curs.push_back(ListReadCur{z.list, z.n});
            }
            for (uint32_t c = 0; c <= nl[v]; ++c) {
                pairs.push_back(ListReadPair{(uint32_t)rd.size(), cur0[v] + c});
                where.push_back(pair0[i] + c);
            }
            rd.push_back(reads[i]);
        }
        std::vector<uint8_t> got(pairs.size(), 0);
        const LvOrder ord(ctx, K);
        const uint64_t t0 = now_ns();
        if (int s = list_reads_check(ctx, &ord.o, rd.data(), (uint32_t)rd.size(), curs.data(),
                                     (uint32_t)curs.size(), pairs.data(), (uint32_t)pairs.size(),
                                     got.data()))
            return s;
        ++S->stats[ST_PASSES];
        S->stats[ST_NS_WAIT] += now_ns() - t0;
        for (size_t k = 0; k < got.size(); ++k) met[where[k]] = got[k];
    }
    // the fold of :372-414 over the met bytes (laspj_reads_host.cpp)
    std::vector<const uint8_t*> ans(n);
    for (uint32_t i = 0; i < n; ++i) ans[i] = met.data() + pair0[i];
    ReadFold F;
    read_fold(n, var_of.data(), (uint32_t)vars.size(), nl.data(), ans.data(), &F);
    *verdict = LASPJ_NIF_OK;
    *found = F.found;
    for (uint32_t i = 0; i < n; ++i) nlazy[i] = (uint32_t)F.fired[i].size();
    if (F.total > cap) return LASPJ_OK;                  // nothing is changed
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t j : F.fired[i]) lazy_ids[at++] = lvs[i]->lazy[j].id;
    for (uint32_t i = 0; i < n; ++i) {
        if (!F.blocked[i]) continue;
        // unmet (:355-364): the waiter laspj_lvar_wait makes, its list the walked threshold
        laspj_lvar* lv = lvs[i];
        laspj_batch** list = own ? &mine.v[i] : &lv->val;
        if (int c = lvar_keep(ctx, lv, lv->waiters, list, !own, id, strict[i], thresholds[i],
                              lens[i]))
            return c;
    }
    for (size_t v = 0; v < vars.size(); ++v) {
        std::vector<LWaiter>& lz = vars[v]->lazy;
        if (F.still[v].size() == lz.size()) continue;
        std::vector<LWaiter> keep;
        keep.reserve(F.still[v].size());
        std::vector<uint8_t> stays(lz.size(), 0);
        for (uint32_t j : F.still[v]) stays[j] = 1;
        for (size_t j = 0; j < lz.size(); ++j) {
            if (stays[j]) keep.push_back(std::move(lz[j]));
            else lwaiter_release(lz[j]);
        }
        lz.swap(keep);
    }
    return LASPJ_OK;
}

}  // namespace

int laspj_lvar_read(laspj_lvar* lv, const uint8_t* threshold, uint64_t n, int strict, uint64_t id,
                    int32_t* met, uint64_t* lazy_ids, uint32_t cap, uint32_t* nlazy,
                    uint32_t* nstill_lazy, int32_t* verdict) {
    const laspj::Entry e = enter_lvar(lv, "lvar_read", threshold && n && met && (lazy_ids || !cap) &&
                                                           nlazy && nstill_lazy && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    ++S->stats[laspj::ST_CALLS];
    *met = 0;
    *nlazy = 0;
    *nstill_lazy = (uint32_t)lv->lazy.size();
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_read", [&]() -> int {
        int32_t found = -1;
        const int32_t st = strict ? 1 : 0;
        const int s = lreads_locked(ctx, S, 1, &lv, &threshold, &n, &st, false, id, &found,
                                    lazy_ids, cap, nlazy, verdict);
        *met = found == 0 ? 1 : 0;
        *nstill_lazy = (uint32_t)lv->lazy.size();
        return s;
    });
}

int laspj_lvar_read_any(laspj_ctx* ctx, uint32_t n, laspj_lvar* const* lvs,
                        const uint8_t* const* thresholds, const uint64_t* lens,
                        const int32_t* strict, uint64_t id, int32_t* found, uint64_t* lazy_ids,
                        uint32_t cap, uint32_t* nlazy, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!found || !verdict) return fail(ctx, LASPJ_E_INVAL, "lvar_read_any: null argument");
    *found = -1;
    *verdict = LASPJ_NIF_OK;
    if (!n) return LASPJ_OK;                      // lists:foldl over []: not_available_yet
    if (!lvs || !thresholds || !lens || !strict || (!lazy_ids && cap) || !nlazy)
        return fail(ctx, LASPJ_E_INVAL, "lvar_read_any: null array");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    for (uint32_t i = 0; i < n; ++i) {
        nlazy[i] = 0;
        if (!lvs[i] || lvs[i]->ctx != ctx || !lvar_alive(S, lvs[i]))
            return fail(ctx, LASPJ_E_INVAL, "lvar_read_any: variable %u is not this context's", i);
        if (!thresholds[i] || !lens[i])
            return fail(ctx, LASPJ_E_INVAL, "lvar_read_any: null threshold");
    }
    ++S->stats[laspj::ST_CALLS];
    *verdict = LASPJ_NIF_FALLBACK;
    return laspj::nomem_guard(ctx, "lvar_read_any", [&]() -> int {
        return lreads_locked(ctx, S, n, lvs, thresholds, lens, strict, true, id, found, lazy_ids,
                             cap, nlazy, verdict);
    });
}

int laspj_lvar_lazy_count(const laspj_lvar* lv, uint32_t* n) {
    laspj::NifState* S = lvar_state(const_cast<laspj_lvar*>(lv));
    if (!S || !n) return LASPJ_E_INVAL;
    std::lock_guard<std::mutex> lk(S->mu);
    *n = (uint32_t)lv->lazy.size();
    return LASPJ_OK;
}

int laspj_lvar_lazy_at(laspj_lvar* lv, uint32_t k, uint64_t* id, const uint8_t** threshold,
                       uint64_t* n) {
    const laspj::Entry e = laspj::enter(lvar_state(lv), lv ? lv->ctx : nullptr, "lvar_lazy_at",
                                        id && threshold && n);
    if (e.rc) return e.rc;
    if (k >= lv->lazy.size())
        return fail(e.ctx, LASPJ_E_RANGE, "lvar_lazy_at: no lazy thread %u", k);
    *id = lv->lazy[k].id;
    *threshold = lv->lazy[k].image.data();
    *n = lv->lazy[k].image.size();
    return LASPJ_OK;
}

int laspj_lvar_lazy_cancel(laspj_lvar* lv, uint64_t id, int32_t* found) {
    const laspj::Entry e = enter_lvar(lv, "lvar_lazy_cancel", found != nullptr);
    if (e.rc) return e.rc;
    *found = 0;
    std::vector<laspj::LWaiter>& zs = lv->lazy;
    for (size_t k = 0; k < zs.size(); ++k)
        if (zs[k].id == id) {
            laspj::lwaiter_release(zs[k]);
            zs.erase(zs.begin() + (ptrdiff_t)k);
            *found = 1;
            break;
        }
    return LASPJ_OK;
}

int laspj_lvar_counts(laspj_lvar* lv, uint32_t* entries, uint32_t* tokens) {
    const laspj::Entry e = enter_lvar(lv, "lvar_counts", entries && tokens);
    if (e.rc) return e.rc;
    if (!(lv->resident && lv->epoch == lv->ns->epoch))
        return fail(e.ctx, LASPJ_E_UNSUPPORTED, "lvar_counts: the value is held as its image");
    uint32_t cnt[2] = {0, 0};
    if (int s = laspj_list_counts(e.ctx, lv->list, cnt)) return s;
    *entries = cnt[0];
    *tokens = cnt[1];
    return LASPJ_OK;
}

int laspj_lvar_resident(const laspj_lvar* lv, int32_t* resident) {
    if (!lv || !lv->ctx || !resident) return LASPJ_E_INVAL;
    laspj::NifState* S = laspj::state(lv->ctx);
    if (!S) return LASPJ_E_INVAL;
    std::lock_guard<std::mutex> lk(S->mu);
    *resident = lv->resident && lv->epoch == lv->ns->epoch ? 1 : 0;
    return LASPJ_OK;
}

}  // extern "C"
