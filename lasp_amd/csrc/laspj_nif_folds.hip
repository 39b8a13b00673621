// Resident fold processes (include/laspj.h "resident fold processes": laspj_fold_*).
// lasp_process:process/3 re-runs (lasp_process.erl:61-95) of fold/6's body (lasp_core.erl:
// 460-486): AccValue = foldl(fun({X, C}, Acc) -> Acc ++ [{V, C} || V <- F(X)] end, [], Value),
// bound with bind/3 (:291-312) into a list-valued variable of the input's namespace.  It is
// the map process (laspj_nif_maps.hip) with a run of outputs per element: a slot owns rows of
// a pool — ykey (the element slot V took) and tmap (per input token, the slot its image holds
// under that key) — and frow / fmapped say per slot where its run lies and which of its
// tokens every row maps.  Every id the producer emits is one the walker of a peer's image
// would give the same term (laspj_lvar_etf_bind).  The kernels are laspj_lvars.hip's
// (k_lf_count, k_lf_write); the argument list is the filter's.  The helpers here are copies
// of the map's, not shared: the map's tables are per slot, these per row.

#include <deque>

#include "laspj_nif_internal.h"

using laspj::fail;

namespace {

using laspj::KindState;
using laspj::NifState;

constexpr uint64_t kFoldHead = 256;         // rec {pending, unmapped}, padded
constexpr uint32_t kFoldRows0 = 64;         // the row pool's first capacity

// the fold's context state; null: the context is gone
NifState* fold_state(laspj_fold* f) {
    if (!f || !f->ctx) return nullptr;
    return laspj::state(f->ctx);
}

// (S->mu held) the handle is this context's and both its variables are alive
bool fold_alive(const NifState* S, laspj_fold* f) {
    return f && S->folds.count(f) && f->in && f->out;
}

laspj::Entry enter_fold(laspj_fold* f, const char* name, bool args_ok) {
    laspj::Entry e = laspj::enter(fold_state(f), f ? f->ctx : nullptr, name, args_ok);
    if (e.rc == LASPJ_OK && !fold_alive(e.S, f))
        e.rc = fail(e.ctx, LASPJ_E_INVAL, "%s: a variable of the fold was destroyed", name);
    return e;
}

// the device tables given back and the fold taken off its variables (ctx->mu held)
void fold_kill(laspj_ctx* ctx, laspj_fold* f) {
    if (f->dev) laspj::dev_release(ctx, f->dev, f->dev_bytes);
    f->dev = nullptr;
    f->dev_bytes = 0;
    if (f->ns) f->ns->folds.erase(f);
    f->in = nullptr;
    f->out = nullptr;
    f->ns.reset();
}

// The tables follow the namespace's generation, as the map's (map_sync): released, the
// mirrors and the row pool cleared, an outstanding list dropped, a refusal forgotten.  Call
// without ctx->mu held.
void fold_sync(laspj_ctx* ctx, laspj_fold* f) {
    if (f->epoch == f->ns->epoch) return;
    if (f->dev) {
        laspj::Guard g(ctx);
        laspj::dev_release(ctx, f->dev, f->dev_bytes);
    }
    f->dev = nullptr;
    f->dev_bytes = 0;
    f->E = f->words = f->row_cap = f->rows_up = 0;
    f->h_eval.clear();
    f->h_frow.clear();
    f->h_fmapped.clear();
    f->h_ykey.clear();
    f->h_tmap.clear();
    f->h_mine.clear();
    f->h_seen.clear();
    f->sum_rt = 0;
    f->up_lo = ~0u;
    f->up_hi = 0;
    f->up_slots.clear();
    f->up_rows.clear();
    f->pmask_valid = false;
    f->rec_dirty = true;
    f->refused = false;
    f->val_not_asc = false;
    f->tok_dirty.clear();
    f->tok_all = true;
    f->listed.clear();
    if (f->outstanding) f->dropped = true;
    f->outstanding = false;
    f->epoch = f->ns->epoch;
}

// the per-slot mirrors sized to n element slots (zero-extended)
void fold_host_fit(laspj_fold* f, uint32_t n) {
    if (f->h_frow.size() >= n) return;
    const size_t cap = std::max<size_t>(n, f->h_frow.size() + f->h_frow.size() / 2);
    f->h_eval.resize((cap + 63) / 64, 0);
    f->h_frow.resize(cap, 0);
    f->h_fmapped.resize(cap, 0);
    f->h_mine.resize(cap, 0);
    f->h_seen.resize(cap, 0);
}

uint32_t fold_rows(const laspj_fold* f) { return (uint32_t)f->h_ykey.size(); }

uint64_t* fold_eval_d(const laspj_fold* f) { return reinterpret_cast<uint64_t*>(f->dev + kFoldHead); }
uint64_t* fold_pmask_d(const laspj_fold* f) { return fold_eval_d(f) + f->words; }
uint64_t* fold_frow_d(const laspj_fold* f) { return fold_pmask_d(f) + f->words; }
uint64_t* fold_fmapped_d(const laspj_fold* f) { return fold_frow_d(f) + f->E; }
uint32_t* fold_ykey_d(const laspj_fold* f) {
    return reinterpret_cast<uint32_t*>(fold_fmapped_d(f) + f->E);
}
uint8_t* fold_tmap_d(const laspj_fold* f) {
    return reinterpret_cast<uint8_t*>(fold_ykey_d(f) + f->row_cap);
}

// The indices listed (below `limit`), sorted and made unique, copied as runs of neighbours:
// many scattered ones as their span.  copy(lo, count) enqueues one range.
template <class Copy>
hipError_t fold_upload_runs(std::vector<uint32_t>& r, uint32_t limit, Copy copy) {
    std::sort(r.begin(), r.end());
    r.erase(std::unique(r.begin(), r.end()), r.end());
    while (!r.empty() && r.back() >= limit) r.pop_back();
    size_t runs = 0;
    for (size_t i = 0; i < r.size(); ++i) runs += i == 0 || r[i] != r[i - 1] + 1;
    hipError_t e = hipSuccess;
    if (runs > 8) {
        e = copy(r.front(), r.back() - r.front() + 1);
    } else {
        for (size_t i = 0; i < r.size() && e == hipSuccess;) {
            size_t j = i + 1;
            while (j < r.size() && r[j] == r[j - 1] + 1) ++j;
            e = copy(r[i], (uint32_t)(j - i));
            i = j;
        }
    }
    r.clear();
    return e;
}

// The device tables sized to the namespace's E element slots and the pool's rows, and brought
// up to the mirrors: a new block (E changed, or the pool outgrew its room: half as much
// again) takes the whole mirrors, else only what changed since the last pass.  ctx->mu held.
int fold_fit(laspj_ctx* ctx, laspj_fold* f, uint32_t E) {
    fold_host_fit(f, E);
    const uint32_t rows = fold_rows(f);
    if (!f->dev || f->E != E || rows > f->row_cap) {
        const uint32_t words = (E + 63u) / 64u;
        const uint64_t cap64 = std::max<uint64_t>(kFoldRows0, rows > f->row_cap ? rows + rows / 2ull
                                                                                 : f->row_cap);
        const uint32_t cap = (uint32_t)std::min<uint64_t>(cap64, 0xFFFFFFF0ull);
        const uint64_t bytes = kFoldHead + 16ull * words + 16ull * E + 4ull * cap + 64ull * cap;
        void* p = nullptr;
        if (laspj::dev_alloc(ctx, bytes, &p) != hipSuccess) {
            hipGetLastError();
            return fail(ctx, LASPJ_E_NOMEM, "fold: device tables (%llu bytes)",
                        (unsigned long long)bytes);
        }
        if (f->dev) laspj::dev_release(ctx, f->dev, f->dev_bytes);
        f->dev = static_cast<uint8_t*>(p);
        f->dev_bytes = bytes;
        f->E = E;
        f->words = words;
        f->row_cap = cap;
        // rec and both bitmaps zero, then the mirrors
        hipError_t e = hipMemsetAsync(f->dev, 0, kFoldHead + 16ull * words, ctx->stream);
        if (e == hipSuccess)
            e = laspj::proc_upload(ctx, fold_eval_d(f), f->h_eval.data(), 8ull * words);
        if (e == hipSuccess) e = laspj::proc_upload(ctx, fold_frow_d(f), f->h_frow.data(), 8ull * E);
        if (e == hipSuccess)
            e = laspj::proc_upload(ctx, fold_fmapped_d(f), f->h_fmapped.data(), 8ull * E);
        if (e == hipSuccess) e = laspj::proc_upload(ctx, fold_ykey_d(f), f->h_ykey.data(), 4ull * rows);
        if (e == hipSuccess) e = laspj::proc_upload(ctx, fold_tmap_d(f), f->h_tmap.data(), 64ull * rows);
        if (e != hipSuccess) {
            laspj::dev_release(ctx, f->dev, f->dev_bytes);
            f->dev = nullptr;
            return fail(ctx, LASPJ_E_DEVICE, "fold: table upload: %s", hipGetErrorString(e));
        }
        f->rows_up = rows;
        f->rec_dirty = false;
        f->pmask_valid = false;
        f->up_lo = ~0u;
        f->up_hi = 0;
        f->up_slots.clear();
        f->up_rows.clear();
        return LASPJ_OK;
    }
    if (f->up_lo <= f->up_hi) {
        // results: the evaluated words and frow entries of the slots answered, as one range
        const uint32_t lo = f->up_lo, hi = std::min(f->up_hi, E - 1);
        if (lo <= hi) {
            const uint32_t w0 = lo >> 6, w1 = hi >> 6;
            LJ_HIP(ctx, laspj::proc_upload(ctx, fold_eval_d(f) + w0, f->h_eval.data() + w0,
                                           8ull * (w1 - w0 + 1)));
            LJ_HIP(ctx, laspj::proc_upload(ctx, fold_frow_d(f) + lo, f->h_frow.data() + lo,
                                           8ull * (hi - lo + 1)));
        }
        f->up_lo = ~0u;
        f->up_hi = 0;
        f->pmask_valid = false;
    }
    // the old rows whose tmap changed (ahead of rows_up moving), then the rows appended
    LJ_HIP(ctx, fold_upload_runs(f->up_rows, f->rows_up, [&](uint32_t lo, uint32_t n) {
        return laspj::proc_upload(ctx, fold_tmap_d(f) + 64ull * lo, f->h_tmap.data() + 64ull * lo,
                                  64ull * n);
    }));
    if (f->rows_up < rows) {
        const uint32_t lo = f->rows_up, n = rows - lo;
        LJ_HIP(ctx, laspj::proc_upload(ctx, fold_ykey_d(f) + lo, f->h_ykey.data() + lo, 4ull * n));
        LJ_HIP(ctx, laspj::proc_upload(ctx, fold_tmap_d(f) + 64ull * lo,
                                       f->h_tmap.data() + 64ull * lo, 64ull * n));
        f->rows_up = rows;
    }
    LJ_HIP(ctx, fold_upload_runs(f->up_slots, E, [&](uint32_t lo, uint32_t n) {
        return laspj::proc_upload(ctx, fold_fmapped_d(f) + lo, f->h_fmapped.data() + lo, 8ull * n);
    }));
    return LASPJ_OK;
}

// the mirrors' edits of one call, undone when the call refuses the fold
struct FoldUndo {
    struct Ed {
        uint8_t what;               // 0 evaluated word, 1 frow, 2 tmap byte, 3 mine, 4 seen, 5 fmapped
        uint64_t at, old;
    };
    std::vector<Ed> eds;
    size_t rows0, up_rows0, up_slots0;
    uint32_t lo0, hi0;
    uint64_t sum0;
    explicit FoldUndo(const laspj_fold* f)
        : rows0(f->h_ykey.size()), up_rows0(f->up_rows.size()), up_slots0(f->up_slots.size()),
          lo0(f->up_lo), hi0(f->up_hi), sum0(f->sum_rt) {}
    void back(laspj_fold* f) {
        for (size_t i = eds.size(); i-- > 0;) {
            const Ed& d = eds[i];
            switch (d.what) {
                case 0: f->h_eval[d.at] = d.old; break;
                case 1: f->h_frow[d.at] = d.old; break;
                case 2: if (d.at < 64ull * rows0) f->h_tmap[d.at] = (uint8_t)d.old; break;
                case 3: f->h_mine[d.at] = d.old; break;
                case 4: f->h_seen[d.at] = (uint8_t)d.old; break;
                default: f->h_fmapped[d.at] = d.old; break;
            }
        }
        eds.clear();
        f->h_ykey.resize(rows0);
        f->h_tmap.resize(64ull * rows0);
        f->up_rows.resize(up_rows0);
        f->up_slots.resize(up_slots0);
        f->up_lo = lo0;
        f->up_hi = hi0;
        f->sum_rt = sum0;
    }
};

// Slot e's tokens the fold has not named yet, each registered under the key of every row of
// e's run as the walker of a peer's image would (dict_reg_tok: an image already there keeps
// its slot — so the rows of a V repeated inside one result agree) and entered in tmap; the
// token's bit of fmapped[e] then says every row has it.  Tokens this fold itself put under e
// stand for another input's and are passed over unless `all` (the map's rule, map_slot_tokens).
// LASPJ_DEC_OK, another DEC status (the fold is refused) or LASPJ_E_NOMEM.
int fold_slot_tokens(laspj_fold* f, KindState& K, uint32_t e, bool all, FoldUndo* u) {
    const uint32_t cnt = std::min(laspj::dict_token_count(K.dict, e), 64u);
    const uint32_t first = (uint32_t)f->h_frow[e], nrow = (uint32_t)(f->h_frow[e] >> 32);
    bool word = false;
    for (uint32_t k = all ? 0 : f->h_seen[e]; k < cnt; ++k) {
        if ((f->h_fmapped[e] >> k) & 1ull) continue;
        if (!all && ((f->h_mine[e] >> k) & 1ull)) continue;
        for (uint32_t r = first; r < first + nrow; ++r) {
            const uint32_t y = f->h_ykey[r];
            uint32_t k2 = k;
            if (y != e) {
                // (the image looked up per row: a registration may move the dictionary's bytes)
                const std::string_view img = laspj::list_tok_image(K.dict, 64ull * e + k);
                const uint32_t before = laspj::dict_token_count(K.dict, y);
                const int st = laspj::dict_reg_tok(K.dict, y, reinterpret_cast<const uint8_t*>(img.data()),
                                                   img.size(), &k2);
                if (st != LASPJ_DEC_OK) return st;
                if (k2 >= 64u) return LASPJ_DEC_UNREPRESENTABLE;
                if (laspj::dict_token_count(K.dict, y) != before) {
                    u->eds.push_back({3, y, f->h_mine[y]});
                    f->h_mine[y] |= 1ull << k2;
                }
            }
            const uint64_t at = 64ull * r + k;
            u->eds.push_back({2, at, f->h_tmap[at]});
            f->h_tmap[at] = (uint8_t)k2;
            if (r < f->rows_up) f->up_rows.push_back(r);
        }
        u->eds.push_back({5, e, f->h_fmapped[e]});
        f->h_fmapped[e] |= 1ull << k;
        word = true;
    }
    if (f->h_seen[e] != cnt) {
        u->eds.push_back({4, e, f->h_seen[e]});
        f->sum_rt += (uint64_t)nrow * (cnt - f->h_seen[e]);
        f->h_seen[e] = (uint8_t)cnt;
    }
    if (word) f->up_slots.push_back(e);
    return LASPJ_DEC_OK;
}

// The tokens minted since the last look mapped under one journal, as map_new_tokens.
// *refused: the fold is refused from here on (everything of this call undone).  S->mu held,
// ctx->mu not.
int fold_new_tokens(laspj_ctx* ctx, NifState* S, laspj_fold* f, bool all, bool* refused) {
    KindState& K = *f->ns;
    *refused = false;
    const uint32_t known = laspj::dict_elements(K.dict);
    fold_host_fit(f, known);
    std::vector<uint32_t> slots;
    if (all || f->tok_all) {
        for (uint32_t e = 0; e < known; ++e)
            if ((f->h_eval[e >> 6] >> (e & 63u)) & 1ull) slots.push_back(e);
    } else {
        std::sort(f->tok_dirty.begin(), f->tok_dirty.end());
        f->tok_dirty.erase(std::unique(f->tok_dirty.begin(), f->tok_dirty.end()), f->tok_dirty.end());
        for (uint32_t e : f->tok_dirty)
            if (e < known && ((f->h_eval[e >> 6] >> (e & 63u)) & 1ull)) slots.push_back(e);
    }
    f->tok_dirty.clear();
    f->tok_all = false;
    if (slots.empty()) return LASPJ_OK;
    const laspj::RegMark mark = laspj::reg_mark(K);
    const uint64_t t0 = laspj::now_ns();
    FoldUndo u(f);
    laspj::dict_begin(K.dict);
    int st = LASPJ_DEC_OK;
    for (size_t i = 0; i < slots.size() && st == LASPJ_DEC_OK; ++i)
        st = fold_slot_tokens(f, K, slots[i], all, &u);
    S->stats[laspj::ST_NS_REGISTER] += laspj::now_ns() - t0;
    if (st != LASPJ_DEC_OK) {
        laspj::dict_rollback(K.dict);
        u.back(f);
        if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "fold: host allocation");
        f->refused = *refused = true;
        return LASPJ_OK;
    }
    laspj::dict_begin(K.dict);
    laspj::reg_note(S, K, mark);
    return LASPJ_OK;
}

// in and out on the device over the current dictionary and the fold's tables of its
// generation; *verdict FALLBACK (counted) otherwise, or when the fold is refused.  S->mu held.
int fold_ready(laspj_ctx* ctx, NifState* S, laspj_fold* f, int32_t* verdict) {
    *verdict = LASPJ_NIF_FALLBACK;
    KindState& K = *f->ns;
    bool a = false, b = false;
    if (int s = laspj::hydrate(ctx, S, f->in, &a)) return s;
    if (a && !K.wide)
        if (int s = laspj::lvar_ready(ctx, S, f->out, &b)) return s;
    // (a decode above may have widened the namespace or started its dictionary afresh)
    if (!a || !b || K.wide || !laspj::var_current(f->in) || f->out->epoch != K.epoch)
        return laspj::fallback(S);
    fold_sync(ctx, f);
    if (f->refused) return laspj::fallback(S);
    *verdict = LASPJ_NIF_OK;
    return LASPJ_OK;
}

laspj::LfFold fold_args_dev(const laspj_fold* f, const KindState& K) {
    laspj::LfFold a;
    a.in = f->in->cells;
    a.Ein = f->in->cells ? f->in->E : 0;
    a.n = K.built_K;
    a.elem_order = laspj::etf_dict_elem_order(K.etf);
    a.grank = static_cast<const uint32_t*>(K.grank);
    a.evaluated = fold_eval_d(f);
    a.pmask = fold_pmask_d(f);
    a.frow = fold_frow_d(f);
    a.fmapped = fold_fmapped_d(f);
    a.ykey = fold_ykey_d(f);
    a.tmap = fold_tmap_d(f);
    a.E = f->E;
    a.words = f->words;
    a.rows = f->rows_up;
    return a;
}

// rec known zero ahead of a pass (ctx->mu held)
int fold_rec_clean(laspj_ctx* ctx, laspj_fold* f) {
    if (!f->rec_dirty) return LASPJ_OK;
    LJ_HIP(ctx, hipMemsetAsync(f->dev, 0, kFoldHead, ctx->stream));
    f->rec_dirty = false;
    return LASPJ_OK;
}

// laspj_fold_run with S->mu held and the handle checked
int fold_run_locked(laspj_ctx* ctx, NifState* S, laspj_fold* f, int32_t* status, uint32_t* pending,
                    int32_t* verdict) {
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *pending = 0;
    if (int s = fold_ready(ctx, S, f, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    KindState& K = *f->ns;
    laspj_lvar* out = f->out;
    if (!K.dict || laspj::dict_elements(K.dict) == 0) return LASPJ_OK;     // nothing held
    for (int attempt = 0;; ++attempt) {
        // the images up to the dictionary (which hands this fold the slots whose tokens
        // grew), those tokens named under their rows' keys, the images up to that
        if (int s = laspj::lvar_images(ctx, S, K)) return s;
        bool refused = false;
        if (int s = fold_new_tokens(ctx, S, f, attempt > 0, &refused)) return s;
        if (refused) {
            *verdict = LASPJ_NIF_FALLBACK;
            return laspj::fallback(S);
        }
        if (int s = laspj::lvar_images(ctx, S, K)) return s;
        const uint32_t n = K.built_K;
        // the output's size from the mirrors: every row, and every row times the tokens its
        // slot has registered
        const uint64_t ub_e = std::max<uint64_t>(fold_rows(f), 1);
        const uint64_t ub_t = std::max<uint64_t>(f->sum_rt, 1);
        if (ub_e > 0xFFFFFFF0ull || ub_t > 0xFFFFFFF0ull)
            return fail(ctx, LASPJ_E_RANGE, "fold_run: too many entries or tokens");
        const uint64_t t0 = laspj::now_ns();
        {
            // the count, the write and (below) the bind enqueued together: the merge lands
            // in out's spare batch, so a pass that turns out pending or unmapped is dropped
            // without out having changed
            laspj::Guard g(ctx);
            if (int s = laspj::lvar_ranks(ctx, S, K)) return s;
            if (int s = laspj::lvar_scratch(ctx, S, laspj::lv_isect_tiles(n))) return s;
            if (int s = fold_fit(ctx, f, K.E)) return s;
            if (int s = fold_rec_clean(ctx, f)) return s;
            if (int s = laspj::list_reserve(ctx, out->val, (uint32_t)ub_e, (uint32_t)ub_t)) return s;
            S->lv_ans[2] = 2;                                   // (not written yet)
            S->lv_ans[5] = 0;
            f->rec_dirty = true;
            LJ_HIP(ctx, laspj::launch_lf_fold(ctx, fold_args_dev(f, K), laspj::list_dev(out->val),
                                              static_cast<uint64_t*>(S->lv_tiles),
                                              reinterpret_cast<uint32_t*>(f->dev), S->lv_ans_d,
                                              false));
            f->rec_dirty = false;                               // (the writer zeroes it)
            // upper bounds until the bind's synchronisation brings the totals
            out->val->known_e = (uint32_t)std::min<uint64_t>(out->val->cap_e, ub_e);
            out->val->known_t = (uint32_t)std::min<uint64_t>(out->val->cap_t, ub_t);
            out->val->not_asc = f->val_not_asc;
            out->val->no_spec = false;
        }
        S->stats[laspj::ST_NS_ENQUEUE] += laspj::now_ns() - t0;
        const laspj::LvOrder ord(ctx, K);
        uint8_t st = 0;
        const uint64_t t1 = laspj::now_ns();
        if (int s = laspj::list_bind_tail(ctx, out->dst, out->list, out->val, &ord.o, &st, nullptr,
                                          0, nullptr))
            return s;
        ++S->stats[laspj::ST_PASSES];
        S->stats[laspj::ST_NS_WAIT] += laspj::now_ns() - t1;
        f->val_not_asc = out->val->not_asc;
        f->pmask_valid = true;
        if (S->lv_ans[2] != 0)
            return fail(ctx, LASPJ_E_RANGE, "fold_run: the producer's output bound did not hold "
                        "(%u entries, %u tokens)", S->lv_ans[0], S->lv_ans[1]);
        if (S->lv_ans[5] != 0)
            return fail(ctx, LASPJ_E_DEVICE, "fold_run: the row tables are at odds with fmapped");
        out->val->known_e = S->lv_ans[0];
        out->val->known_t = S->lv_ans[1];
        *pending = S->lv_ans[3];
        if (*pending) return LASPJ_OK;                          // the merge is dropped
        if (S->lv_ans[4]) {
            // a present token the host had not named (the device is the source of truth):
            // every token of every evaluated slot, then the pass again
            if (attempt)
                return fail(ctx, LASPJ_E_DEVICE, "fold_run: %u tokens stay unmapped", S->lv_ans[4]);
            continue;
        }
        if (st == 1) {
            std::swap(out->list, out->dst);
            laspj::llazy_clear(out);                            // write/4: a fresh #dv
        }
        *status = st;
        return LASPJ_OK;
    }
}

// laspj_fold_args with S->mu held and the handle checked
int fold_args_locked(laspj_ctx* ctx, NifState* S, laspj_fold* f, const uint8_t** out,
                     uint64_t* out_len, uint32_t* count, int32_t* verdict) {
    if (int s = fold_ready(ctx, S, f, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    KindState& K = *f->ns;
    std::vector<uint64_t> pm;
    if (K.dict && laspj::dict_elements(K.dict)) {
        if (int s = laspj::lvar_images(ctx, S, K)) return s;
        laspj::Guard g(ctx);
        const bool fitted = f->dev && f->E == K.E && f->up_lo > f->up_hi;
        if (!f->pmask_valid || !fitted) {
            // no run since the tables last changed: the count launch alone
            if (int s = laspj::lvar_scratch(ctx, S, laspj::lv_isect_tiles(K.built_K))) return s;
            if (int s = fold_fit(ctx, f, K.E)) return s;
            f->rec_dirty = true;                                // (no writer behind it)
            LJ_HIP(ctx, laspj::launch_lf_fold(ctx, fold_args_dev(f, K), laspj::ListDev{},
                                              static_cast<uint64_t*>(S->lv_tiles),
                                              reinterpret_cast<uint32_t*>(f->dev), nullptr, true));
            ++S->stats[laspj::ST_PASSES];
            f->pmask_valid = true;
        }
        pm.resize(f->words);
        LJ_HIP(ctx, laspj::readback(ctx, pm.data(), fold_pmask_d(f), 8ull * f->words));
    }
    std::vector<uint32_t> slots;
    laspj::proc_args_image(K, pm, f->h_eval, false, &slots, &f->image);
    f->listed.swap(slots);
    f->outstanding = true;
    f->dropped = false;
    *out = reinterpret_cast<const uint8_t*>(f->image.data());
    *out_len = f->image.size();
    *count = (uint32_t)f->listed.size();
    return LASPJ_OK;
}

// One F(X) (a term inside the results' image) as its elements' images; false: not a proper
// list (the reference's comprehension raises bad_generator).  A STRING_EXT's integers are
// written out in `store`.
bool fold_split(std::string_view t, std::vector<std::string_view>* out, std::deque<std::string>* store) {
    out->clear();
    const uint8_t* p = reinterpret_cast<const uint8_t*>(t.data());
    const size_t n = t.size();
    if (!n) return false;
    if (p[0] == 106) return n == 1;
    if (p[0] == 107) {
        if (n < 3) return false;
        const size_t cnt = ((size_t)p[1] << 8) | p[2];
        if (n != 3 + cnt) return false;
        store->emplace_back(2 * cnt, (char)97);
        std::string& s = store->back();
        for (size_t i = 0; i < cnt; ++i) {
            s[2 * i + 1] = (char)p[3 + i];
            out->emplace_back(s.data() + 2 * i, 2);
        }
        return true;
    }
    if (p[0] != 108 || n < 6) return false;
    const uint32_t cnt = ((uint32_t)p[1] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 8) | p[4];
    size_t off = 5;
    for (uint32_t i = 0; i < cnt; ++i) {
        const size_t l = off < n ? laspj::list_term_len(p + off, n - off) : 0;
        if (!l) return false;
        out->emplace_back(t.data() + off, l);
        off += l;
    }
    return off + 1 == n && p[off] == 106;
}

// laspj_fold_results past its checks: every V registered, the rows appended and the tables
// edited under one journal; *refused: rolled back, nothing recorded
int fold_record(laspj_ctx* ctx, NifState* S, laspj_fold* f,
                const std::vector<std::vector<std::string_view>>& res, bool* refused) {
    KindState& K = *f->ns;
    *refused = false;
    const laspj::RegMark mark = laspj::reg_mark(K);
    const uint64_t t0 = laspj::now_ns();
    FoldUndo u(f);
    laspj::dict_begin(K.dict);
    int st = LASPJ_DEC_OK;
    fold_host_fit(f, laspj::dict_elements(K.dict));
    // every V as an element slot of the input's namespace (one that exists already, or new),
    // a row each in F's own order
    for (size_t k = 0; k < res.size() && st == LASPJ_DEC_OK; ++k) {
        const uint32_t e = f->listed[k];
        const uint64_t first = f->h_ykey.size();
        if (first + res[k].size() > 0xFFFFFFF0ull) {
            st = LASPJ_DEC_UNREPRESENTABLE;
            break;
        }
        for (size_t i = 0; i < res[k].size() && st == LASPJ_DEC_OK; ++i) {
            uint32_t y = 0;
            st = laspj::dict_reg_elem(K.dict, reinterpret_cast<const uint8_t*>(res[k][i].data()),
                                      res[k][i].size(), &y);
            if (st != LASPJ_DEC_OK) break;
            f->h_ykey.push_back(y);
            f->h_tmap.insert(f->h_tmap.end(), 64, 0xFF);
        }
        if (st != LASPJ_DEC_OK) break;
        fold_host_fit(f, laspj::dict_elements(K.dict));
        u.eds.push_back({0, e >> 6, f->h_eval[e >> 6]});
        f->h_eval[e >> 6] |= 1ull << (e & 63u);
        u.eds.push_back({1, e, f->h_frow[e]});
        f->h_frow[e] = first | ((uint64_t)res[k].size() << 32);
        u.eds.push_back({5, e, f->h_fmapped[e]});
        f->h_fmapped[e] = 0;
        f->up_lo = std::min(f->up_lo, e);
        f->up_hi = std::max(f->up_hi, e);
    }
    // then X's tokens as tokens of every V
    for (size_t k = 0; k < res.size() && st == LASPJ_DEC_OK; ++k)
        st = fold_slot_tokens(f, K, f->listed[k], false, &u);
    S->stats[laspj::ST_NS_REGISTER] += laspj::now_ns() - t0;
    if (st != LASPJ_DEC_OK) {
        laspj::dict_rollback(K.dict);
        u.back(f);
        if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "fold_results: host allocation");
        f->refused = *refused = true;
        return LASPJ_OK;
    }
    laspj::dict_begin(K.dict);
    laspj::reg_note(S, K, mark);
    f->pmask_valid = false;
    return LASPJ_OK;
}

}  // namespace

namespace laspj {

void folds_var_gone(NifState* S, laspj_var* v) {
    for (laspj_fold* f : S->folds)
        if (f->in == v) fold_kill(v->ctx, f);
}

void folds_lvar_gone(NifState* S, laspj_lvar* lv) {
    for (laspj_fold* f : S->folds)
        if (f->out == lv) {
            Guard g(lv->ctx);
            fold_kill(lv->ctx, f);
        }
}

void folds_ctx_gone(laspj_ctx* ctx, NifState* S) {
    for (laspj_fold* f : S->folds) {
        fold_kill(ctx, f);
        f->ctx = nullptr;
    }
    S->folds.clear();
}

}  // namespace laspj

extern "C" {

int laspj_fold_create(laspj_var* in, laspj_lvar* out, laspj_fold** f) {
    if (!in || !out || !f) return LASPJ_E_INVAL;
    *f = nullptr;
    if (in->gc) {
        // riak_dt_gcounter is no type fold/6 folds over
        laspj_ctx* c = out->ctx;
        return c ? fail(c, LASPJ_E_KIND, "fold_create: an OR-Set variable") : LASPJ_E_KIND;
    }
    NifState* S = laspj::var_state(in);
    if (!S || !out->ctx) return LASPJ_E_INVAL;
    laspj_ctx* ctx = in->ctx;
    if (out->ctx != ctx) return fail(ctx, LASPJ_E_INVAL, "fold_create: variables of different contexts");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(in) || !S->lvars.count(out)) return laspj::unknown_variable(ctx, "fold_create");
    if (in->kind != LASPJ_KIND_ORSET)
        return fail(ctx, LASPJ_E_KIND, "fold_create: an OR-Set variable (a list variable holds OR-Set lists)");
    if (out->pairs)
        return fail(ctx, LASPJ_E_KIND, "fold_create: a pair-keyed list variable takes product/7's output only");
    if (in->ns != out->ns)
        return fail(ctx, LASPJ_E_UNSUPPORTED, "fold_create: variables of one namespace");
    auto* p = new (std::nothrow) laspj_fold;
    if (!p) return fail(ctx, LASPJ_E_NOMEM, "fold_create: host allocation");
    p->ctx = ctx;
    p->in = in;
    p->out = out;
    p->ns = in->ns;
    p->epoch = in->ns->epoch;
    const int s = laspj::nomem_guard(ctx, "fold_create", [&] {
        S->folds.insert(p);
        try {
            p->ns->folds.insert(p);
        } catch (const std::bad_alloc&) {
            S->folds.erase(p);
            throw;
        }
        return LASPJ_OK;
    }, "registry");
    if (s) {
        delete p;
        return s;
    }
    *f = p;
    return LASPJ_OK;
}

int laspj_fold_destroy(laspj_fold* f) {
    if (!f) return LASPJ_E_INVAL;
    if (NifState* S = fold_state(f)) {
        std::lock_guard<std::mutex> lk(S->mu);
        if (f->ctx) {
            S->folds.erase(f);
            laspj::Guard g(f->ctx);
            fold_kill(f->ctx, f);
        }
    }
    delete f;
    return LASPJ_OK;
}

int laspj_fold_run(laspj_fold* f, int32_t* status, uint32_t* pending, int32_t* verdict) {
    const laspj::Entry e = enter_fold(f, "fold_run", status && pending && verdict);
    if (e.rc) return e.rc;
    return laspj::nomem_guard(e.ctx, "fold_run", [&] {
        return fold_run_locked(e.ctx, e.S, f, status, pending, verdict);
    });
}

int laspj_fold_args(laspj_fold* f, const uint8_t** out, uint64_t* out_len, uint32_t* count,
                    int32_t* verdict) {
    const laspj::Entry e = enter_fold(f, "fold_args", out && out_len && count && verdict);
    if (e.rc) return e.rc;
    ++e.S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *count = 0;
    return laspj::nomem_guard(e.ctx, "fold_args", [&] {
        return fold_args_locked(e.ctx, e.S, f, out, out_len, count, verdict);
    });
}

int laspj_fold_results(laspj_fold* f, const uint8_t* results, uint64_t n, int32_t* verdict) {
    const laspj::Entry en = enter_fold(f, "fold_results", verdict != nullptr);
    if (en.rc) return en.rc;
    laspj_ctx* ctx = en.ctx;
    NifState* S = en.S;
    ++S->stats[laspj::ST_CALLS];
    *verdict = LASPJ_NIF_OK;
    fold_sync(ctx, f);
    if (!f->outstanding) {
        if (f->dropped) {
            // a dictionary reset took the list: nothing recorded, the next run asks again
            f->dropped = false;
            return LASPJ_OK;
        }
        return fail(ctx, LASPJ_E_INVAL, "fold_results: no argument list outstanding");
    }
    return laspj::nomem_guard(ctx, "fold_results", [&]() -> int {
        std::vector<std::string_view> res;
        std::string bytes;
        if (!laspj::image_list(results, n, &res, &bytes) || res.size() != f->listed.size())
            return fail(ctx, LASPJ_E_INVAL, "fold_results: %zu results for %zu arguments",
                        res.size(), f->listed.size());
        // every F(X) a proper list, before anything is recorded
        std::vector<std::vector<std::string_view>> vs(res.size());
        std::deque<std::string> store;
        for (size_t k = 0; k < res.size(); ++k)
            if (!fold_split(res[k], &vs[k], &store))
                return fail(ctx, LASPJ_E_INVAL, "fold_results: result %zu is not a proper list", k);
        f->outstanding = false;
        bool refused = false;
        const int s = f->listed.empty() ? LASPJ_OK : fold_record(ctx, S, f, vs, &refused);
        f->listed.clear();
        if (s) return s;
        if (refused) {
            *verdict = LASPJ_NIF_FALLBACK;
            return laspj::fallback(S);
        }
        return LASPJ_OK;
    });
}

}  // extern "C"
