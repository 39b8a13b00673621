// List-valued variables (laspj_lvar_*).
// include/laspj.h "list-valued resident variables": a `#dv.value` that is any list of
// {Key, [{Token, Bool}]}, kept as a LIST batch over the slots of a laspj_var namespace.  The
// list kernels are laspj_lists.hip's; the order tables and the producer of intersection/7's
// OR-Set branch (lasp_core.erl:559-568, 583) are laspj_lvars.hip's.  The variable's waiting
// threads (read/6 and write/4's reply_to_all, lasp_core.erl:331-364, 765-825) are kept here as
// device lists and checked by laspj_lists.hip's waiter pass, alone or behind a bind.

#include "laspj_nif_internal.h"

using laspj::fail;
using laspj::var_state;

namespace laspj {

void lwaiter_release(LWaiter& w) {
    if (w.list) laspj_batch_destroy(w.list);
    w.list = nullptr;
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
    const int st = list_walk(K.dict, LASPJ_KIND_ORSET, lv->image.data(), lv->image.size(), &it,
                             nullptr);
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
    if (l->kind != LASPJ_KIND_ORSET || r->kind != LASPJ_KIND_ORSET || l->ns != out->ns ||
        r->ns != out->ns)
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
    *status = st;
    return LASPJ_OK;
}

// an image walked into lv->val over the namespace (its unseen terms registered, the images
// and tables brought up to them); *ok false: the walk refused it (its registrations undone)
int lvar_walk_val(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, const uint8_t* p, uint64_t n,
                  bool* ok) {
    KindState& K = *lv->ns;
    *ok = false;
    if (!K.dict)
        if (int s = reset_dict(ctx, S, K)) return s;
    const RegMark m = reg_mark(K);
    ListItems it;
    const uint64_t t0 = now_ns();
    const int st = list_walk(K.dict, LASPJ_KIND_ORSET, p, n, &it, nullptr);
    S->stats[ST_NS_REGISTER] += now_ns() - t0;
    if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "lvar: host allocation");
    if (st != LASPJ_DEC_OK) return LASPJ_OK;
    reg_note(S, K, m);
    if (int s = lvar_prepare(ctx, S, K)) return s;
    if (int s = lvar_upload(ctx, lv->val, it)) return s;
    *ok = true;
    return LASPJ_OK;
}

// *ok: every waiter's threshold is on the device over the current dictionary.  One whose
// list a dictionary reset made stale is walked back in from its image here (its terms
// registered afresh: the caller brings the images and tables up to them); in a wide
// namespace, or when the walk refuses an image, the lists stay as they are.  S->mu held.
int lwaiters_ready(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, bool* ok) {
    KindState& K = *lv->ns;
    *ok = !K.wide;
    if (K.wide) return LASPJ_OK;
    for (LWaiter& w : lv->waiters) {
        if (w.list && w.epoch == K.epoch) continue;
        if (!K.dict)
            if (int s = reset_dict(ctx, S, K)) return s;
        const RegMark m = reg_mark(K);
        ListItems it;
        const int st = list_walk(K.dict, LASPJ_KIND_ORSET, w.image.data(), w.image.size(), &it,
                                 nullptr);
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
}

}  // namespace

extern "C" {

int laspj_lvar_create(laspj_var* peer, laspj_lvar** out) {
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
        // threshold_met (lasp_lattice.erl:62-75): is_inflation / is_strict_inflation of the
        // threshold -> the value
        const laspj::LvOrder ord(ctx, *lv->ns);
        laspj_buf* res = nullptr;
        if (int s = laspj_buf_create(ctx, 8, &res)) return s;
        uint8_t b = 0;
        int s = laspj_list_inflation(ctx, lv->val, lv->list, strict ? 1 : 0, &ord.o, res);
        if (s == LASPJ_OK) s = laspj_buf_download(ctx, res, 0, &b, 1);
        laspj_buf_destroy(res);
        if (s) return s;
        ++S->stats[laspj::ST_PASSES];
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
        const laspj::LvOrder ord(ctx, *lv->ns);
        laspj_buf* res = nullptr;
        if (int s = laspj_buf_create(ctx, 8, &res)) return s;
        uint8_t b = 0;
        int s = laspj_list_inflation(ctx, lv->val, lv->list, strict ? 1 : 0, &ord.o, res);
        if (s == LASPJ_OK) s = laspj_buf_download(ctx, res, 0, &b, 1);
        laspj_buf_destroy(res);
        if (s) return s;
        ++S->stats[laspj::ST_PASSES];
        *verdict = LASPJ_NIF_OK;
        if (b) {
            *met = 1;
            return LASPJ_OK;
        }
        // unmet (lasp_core.erl:355-364): appended to waiting_threads; the walked threshold
        // (lv->val) becomes the waiter's list, a fresh block takes its place
        laspj::LWaiter w;
        w.id = id;
        w.strict = strict ? 1 : 0;
        w.image.assign(threshold, threshold + n);
        w.n = lv->val->known_e;
        w.epoch = lv->ns->epoch;
        lv->waiters.reserve(lv->waiters.size() + 1);
        laspj_batch* fresh = nullptr;
        if (int c = laspj_list_batch_create(ctx, LASPJ_KIND_ORSET_LIST, 1, 1, 1, &fresh)) {
            *verdict = LASPJ_NIF_FALLBACK;
            return c;
        }
        w.list = lv->val;
        lv->val = fresh;
        lv->waiters.push_back(std::move(w));
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
