// Resident map processes (include/laspj.h "resident map processes": laspj_map_*).
// lasp_process:process/3 re-runs (lasp_process.erl:61-95) of map/6's body (lasp_core.erl:
// 641-667): AccValue = [{F(X), Cx} || {X, Cx} <- Value], bound with bind/3 (:291-312) into a
// list-valued variable of the input's namespace.  The fun's results live beside the
// namespace as two tables — ymap (the element slot F(X) took) and tmap (per input token, the
// slot its image holds under that element) — so every id the producer emits is one the
// walker of a peer's image would give the same term (laspj_lvar_etf_bind).  The kernels are
// laspj_lvars.hip's (k_lm_count, k_lm_write); the argument list is the filter's.

#include "laspj_nif_internal.h"

using laspj::fail;

namespace {

using laspj::KindState;
using laspj::NifState;

constexpr uint64_t kMapHead = 256;          // rec {pending, unmapped}, padded

// the map's context state; null: the context is gone
NifState* map_state(laspj_map* m) {
    if (!m || !m->ctx) return nullptr;
    return laspj::state(m->ctx);
}

// (S->mu held) the handle is this context's and both its variables are alive
bool map_alive(const NifState* S, laspj_map* m) {
    return m && S->maps.count(m) && m->in && m->out;
}

laspj::Entry enter_map(laspj_map* m, const char* name, bool args_ok) {
    laspj::Entry e = laspj::enter(map_state(m), m ? m->ctx : nullptr, name, args_ok);
    if (e.rc == LASPJ_OK && !map_alive(e.S, m))
        e.rc = fail(e.ctx, LASPJ_E_INVAL, "%s: a variable of the map was destroyed", name);
    return e;
}

// the device tables given back and the map taken off its variables (ctx->mu held)
void map_kill(laspj_ctx* ctx, laspj_map* m) {
    if (m->dev) laspj::dev_release(ctx, m->dev, m->dev_bytes);
    m->dev = nullptr;
    m->dev_bytes = 0;
    if (m->ns) m->ns->maps.erase(m);
    m->in = nullptr;
    m->out = nullptr;
    m->ns.reset();
}

// The tables follow the namespace's generation: a dictionary reset renumbers the element
// and token slots, so the tables are released, the mirrors cleared, an outstanding argument
// list dropped and a refusal forgotten (F is asked again).  Call without ctx->mu held.
void map_sync(laspj_ctx* ctx, laspj_map* m) {
    if (m->epoch == m->ns->epoch) return;
    if (m->dev) {
        laspj::Guard g(ctx);
        laspj::dev_release(ctx, m->dev, m->dev_bytes);
    }
    m->dev = nullptr;
    m->dev_bytes = 0;
    m->E = m->words = 0;
    m->h_eval.clear();
    m->h_ymap.clear();
    m->h_tmap.clear();
    m->h_mine.clear();
    m->h_seen.clear();
    m->up_lo = ~0u;
    m->up_hi = 0;
    m->up_rows.clear();
    m->pmask_valid = false;
    m->rec_dirty = true;
    m->refused = false;
    m->val_not_asc = false;
    m->tok_dirty.clear();
    m->tok_all = true;
    m->listed.clear();
    if (m->outstanding) m->dropped = true;
    m->outstanding = false;
    m->epoch = m->ns->epoch;
}

// the mirrors sized to n element slots (zero-extended; tmap with 0xFF)
void map_host_fit(laspj_map* m, uint32_t n) {
    if (m->h_ymap.size() >= n) return;
    const size_t cap = std::max<size_t>(n, m->h_ymap.size() + m->h_ymap.size() / 2);
    m->h_eval.resize((cap + 63) / 64, 0);
    m->h_ymap.resize(cap, 0);
    m->h_tmap.resize(64 * cap, 0xFF);
    m->h_mine.resize(cap, 0);
    m->h_seen.resize(cap, 0);
}

uint64_t* map_eval_d(const laspj_map* m) { return reinterpret_cast<uint64_t*>(m->dev + kMapHead); }
uint64_t* map_pmask_d(const laspj_map* m) { return map_eval_d(m) + m->words; }
uint32_t* map_ymap_d(const laspj_map* m) {
    return reinterpret_cast<uint32_t*>(map_pmask_d(m) + m->words);
}
uint8_t* map_tmap_d(const laspj_map* m) {
    return reinterpret_cast<uint8_t*>(map_ymap_d(m) + m->E);
}

// The device tables sized to the namespace's E element slots and brought up to the mirrors:
// a new block takes the whole mirrors (growth: the bitmaps zero-extended, tmap 0xFF-
// extended), else only the rows that changed since the last pass.  ctx->mu held.
int map_fit(laspj_ctx* ctx, laspj_map* m, uint32_t E) {
    map_host_fit(m, E);
    if (!m->dev || m->E != E) {
        const uint32_t words = (E + 63u) / 64u;
        const uint64_t bytes = kMapHead + 16ull * words + 4ull * E + 64ull * E;
        void* p = nullptr;
        if (laspj::dev_alloc(ctx, bytes, &p) != hipSuccess) {
            hipGetLastError();
            return fail(ctx, LASPJ_E_NOMEM, "map: device tables (%llu bytes)",
                        (unsigned long long)bytes);
        }
        if (m->dev) laspj::dev_release(ctx, m->dev, m->dev_bytes);
        m->dev = static_cast<uint8_t*>(p);
        m->dev_bytes = bytes;
        m->E = E;
        m->words = words;
        // rec and both bitmaps zero, then the mirrors
        hipError_t e = hipMemsetAsync(m->dev, 0, kMapHead + 16ull * words, ctx->stream);
        if (e == hipSuccess)
            e = laspj::proc_upload(ctx, map_eval_d(m), m->h_eval.data(), 8ull * words);
        if (e == hipSuccess) e = laspj::proc_upload(ctx, map_ymap_d(m), m->h_ymap.data(), 4ull * E);
        if (e == hipSuccess) e = laspj::proc_upload(ctx, map_tmap_d(m), m->h_tmap.data(), 64ull * E);
        if (e != hipSuccess) {
            laspj::dev_release(ctx, m->dev, m->dev_bytes);
            m->dev = nullptr;
            return fail(ctx, LASPJ_E_DEVICE, "map: table upload: %s", hipGetErrorString(e));
        }
        m->rec_dirty = false;
        m->pmask_valid = false;
        m->up_lo = ~0u;
        m->up_hi = 0;
        m->up_rows.clear();
        return LASPJ_OK;
    }
    if (m->up_lo <= m->up_hi) {
        // results: the evaluated words and ymap entries of the slots answered, as one range
        const uint32_t lo = m->up_lo, hi = std::min(m->up_hi, E - 1);
        if (lo <= hi) {
            const uint32_t w0 = lo >> 6, w1 = hi >> 6;
            LJ_HIP(ctx, laspj::proc_upload(ctx, map_eval_d(m) + w0, m->h_eval.data() + w0,
                                           8ull * (w1 - w0 + 1)));
            LJ_HIP(ctx, laspj::proc_upload(ctx, map_ymap_d(m) + lo, m->h_ymap.data() + lo,
                                           4ull * (hi - lo + 1)));
        }
        m->up_lo = ~0u;
        m->up_hi = 0;
        m->pmask_valid = false;
    }
    if (!m->up_rows.empty()) {
        std::vector<uint32_t>& r = m->up_rows;
        std::sort(r.begin(), r.end());
        r.erase(std::unique(r.begin(), r.end()), r.end());
        while (!r.empty() && r.back() >= E) r.pop_back();
        // runs of neighbouring rows in one copy each; many scattered rows as their span
        size_t runs = 0;
        for (size_t i = 0; i < r.size(); ++i) runs += i == 0 || r[i] != r[i - 1] + 1;
        if (runs > 8) {
            const uint32_t lo = r.front(), hi = r.back();
            LJ_HIP(ctx, laspj::proc_upload(ctx, map_tmap_d(m) + 64ull * lo,
                                           m->h_tmap.data() + 64ull * lo, 64ull * (hi - lo + 1)));
        } else {
            for (size_t i = 0; i < r.size();) {
                size_t j = i + 1;
                while (j < r.size() && r[j] == r[j - 1] + 1) ++j;
                LJ_HIP(ctx, laspj::proc_upload(ctx, map_tmap_d(m) + 64ull * r[i],
                                               m->h_tmap.data() + 64ull * r[i], 64ull * (j - i)));
                i = j;
            }
        }
        r.clear();
    }
    return LASPJ_OK;
}

// the mirrors' edits of one call, undone when the call refuses the map
struct MapUndo {
    struct Ed {
        uint8_t what;               // 0 evaluated word, 1 ymap, 2 tmap byte, 3 mine, 4 seen
        uint64_t at, old;
    };
    std::vector<Ed> eds;
    void back(laspj_map* m) {
        for (size_t i = eds.size(); i-- > 0;) {
            const Ed& d = eds[i];
            switch (d.what) {
                case 0: m->h_eval[d.at] = d.old; break;
                case 1: m->h_ymap[d.at] = (uint32_t)d.old; break;
                case 2: m->h_tmap[d.at] = (uint8_t)d.old; break;
                case 3: m->h_mine[d.at] = d.old; break;
                default: m->h_seen[d.at] = (uint8_t)d.old; break;
            }
        }
        eds.clear();
    }
};

// Slot e's tokens the map has not named yet, each registered under y = ymap[e] as the walker
// of a peer's image would (dict_reg_tok: an image already there keeps its slot) and entered
// in tmap.  Tokens this map itself put under e stand for another input's and are passed over
// unless `all` (the device found one present).  LASPJ_DEC_OK, another DEC status (the map is
// refused: an `==`-equal token under another image, y full — dict_reg_tok stops at
// dict_tok_cap, so the namespace is never widened) or LASPJ_E_NOMEM.
int map_slot_tokens(laspj_map* m, KindState& K, uint32_t e, bool all, MapUndo* u) {
    const uint32_t cnt = std::min(laspj::dict_token_count(K.dict, e), 64u);
    const uint32_t y = m->h_ymap[e];
    bool row = false;
    for (uint32_t k = all ? 0 : m->h_seen[e]; k < cnt; ++k) {
        const uint64_t at = 64ull * e + k;
        if (m->h_tmap[at] != 0xFF) continue;
        if (!all && ((m->h_mine[e] >> k) & 1ull)) continue;
        uint32_t k2 = k;
        if (y != e) {
            const std::string_view img = laspj::list_tok_image(K.dict, at);
            const uint32_t before = laspj::dict_token_count(K.dict, y);
            const int st = laspj::dict_reg_tok(K.dict, y, reinterpret_cast<const uint8_t*>(img.data()),
                                               img.size(), &k2);
            if (st != LASPJ_DEC_OK) return st;
            if (k2 >= 64u) return LASPJ_DEC_UNREPRESENTABLE;
            if (laspj::dict_token_count(K.dict, y) != before) {
                u->eds.push_back({3, y, m->h_mine[y]});
                m->h_mine[y] |= 1ull << k2;
            }
        }
        u->eds.push_back({2, at, 0xFF});
        m->h_tmap[at] = (uint8_t)k2;
        row = true;
    }
    if (m->h_seen[e] != cnt) {
        u->eds.push_back({4, e, m->h_seen[e]});
        m->h_seen[e] = (uint8_t)cnt;
    }
    if (row) m->up_rows.push_back(e);
    return LASPJ_DEC_OK;
}

// The tokens minted since the last look (the slots patch_etf handed over, or every evaluated
// slot after a rebuild; `all`: every token of every evaluated slot) mapped under one
// journal.  *refused: the map is refused from here on (everything of this call undone).
// S->mu held, ctx->mu not.
int map_new_tokens(laspj_ctx* ctx, NifState* S, laspj_map* m, bool all, bool* refused) {
    KindState& K = *m->ns;
    *refused = false;
    const uint32_t known = laspj::dict_elements(K.dict);
    map_host_fit(m, known);
    std::vector<uint32_t> slots;
    if (all || m->tok_all) {
        for (uint32_t e = 0; e < known; ++e)
            if ((m->h_eval[e >> 6] >> (e & 63u)) & 1ull) slots.push_back(e);
    } else {
        std::sort(m->tok_dirty.begin(), m->tok_dirty.end());
        m->tok_dirty.erase(std::unique(m->tok_dirty.begin(), m->tok_dirty.end()), m->tok_dirty.end());
        for (uint32_t e : m->tok_dirty)
            if (e < known && ((m->h_eval[e >> 6] >> (e & 63u)) & 1ull)) slots.push_back(e);
    }
    m->tok_dirty.clear();
    m->tok_all = false;
    if (slots.empty()) return LASPJ_OK;
    const laspj::RegMark mark = laspj::reg_mark(K);
    const uint64_t t0 = laspj::now_ns();
    const size_t rows0 = m->up_rows.size();
    MapUndo u;
    laspj::dict_begin(K.dict);
    int st = LASPJ_DEC_OK;
    for (size_t i = 0; i < slots.size() && st == LASPJ_DEC_OK; ++i)
        st = map_slot_tokens(m, K, slots[i], all, &u);
    S->stats[laspj::ST_NS_REGISTER] += laspj::now_ns() - t0;
    if (st != LASPJ_DEC_OK) {
        laspj::dict_rollback(K.dict);
        u.back(m);
        m->up_rows.resize(rows0);
        if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "map: host allocation");
        m->refused = *refused = true;
        return LASPJ_OK;
    }
    laspj::dict_begin(K.dict);
    laspj::reg_note(S, K, mark);
    return LASPJ_OK;
}

// in and out on the device over the current dictionary and the map's tables of its
// generation; *verdict FALLBACK (counted) otherwise, or when the map is refused.  S->mu held.
int map_ready(laspj_ctx* ctx, NifState* S, laspj_map* m, int32_t* verdict) {
    *verdict = LASPJ_NIF_FALLBACK;
    KindState& K = *m->ns;
    bool a = false, b = false;
    if (int s = laspj::hydrate(ctx, S, m->in, &a)) return s;
    if (a && !K.wide)
        if (int s = laspj::lvar_ready(ctx, S, m->out, &b)) return s;
    // (a decode above may have widened the namespace or started its dictionary afresh)
    if (!a || !b || K.wide || !laspj::var_current(m->in) || m->out->epoch != K.epoch)
        return laspj::fallback(S);
    map_sync(ctx, m);
    if (m->refused) return laspj::fallback(S);
    *verdict = LASPJ_NIF_OK;
    return LASPJ_OK;
}

laspj::LmMap map_args_dev(const laspj_map* m, const KindState& K) {
    laspj::LmMap a;
    a.in = m->in->cells;
    a.Ein = m->in->cells ? m->in->E : 0;
    a.n = K.built_K;
    a.elem_order = laspj::etf_dict_elem_order(K.etf);
    a.grank = static_cast<const uint32_t*>(K.grank);
    a.evaluated = map_eval_d(m);
    a.pmask = map_pmask_d(m);
    a.ymap = map_ymap_d(m);
    a.tmap = map_tmap_d(m);
    a.E = m->E;
    a.words = m->words;
    return a;
}

// rec known zero ahead of a pass (ctx->mu held)
int map_rec_clean(laspj_ctx* ctx, laspj_map* m) {
    if (!m->rec_dirty) return LASPJ_OK;
    LJ_HIP(ctx, hipMemsetAsync(m->dev, 0, kMapHead, ctx->stream));
    m->rec_dirty = false;
    return LASPJ_OK;
}

// laspj_map_run with S->mu held and the handle checked
int map_run_locked(laspj_ctx* ctx, NifState* S, laspj_map* m, int32_t* status, uint32_t* pending,
                   int32_t* verdict) {
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *pending = 0;
    if (int s = map_ready(ctx, S, m, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    KindState& K = *m->ns;
    laspj_lvar* out = m->out;
    if (!K.dict || laspj::dict_elements(K.dict) == 0) return LASPJ_OK;     // nothing held
    for (int attempt = 0;; ++attempt) {
        // the images up to the dictionary (which hands this map the slots whose tokens
        // grew), those tokens named under their keys, the images up to that
        if (int s = laspj::lvar_images(ctx, S, K)) return s;
        bool refused = false;
        if (int s = map_new_tokens(ctx, S, m, attempt > 0, &refused)) return s;
        if (refused) {
            *verdict = LASPJ_NIF_FALLBACK;
            return laspj::fallback(S);
        }
        if (int s = laspj::lvar_images(ctx, S, K)) return s;
        const uint32_t n = K.built_K;
        const uint64_t ub_t = std::max<uint64_t>(K.built_toks, 1);
        if (ub_t > 0xFFFFFFF0ull) return fail(ctx, LASPJ_E_RANGE, "map_run: too many tokens");
        const uint64_t t0 = laspj::now_ns();
        {
            // the count, the write and (below) the bind enqueued together: the merge lands
            // in out's spare batch, so a pass that turns out pending or unmapped is dropped
            // without out having changed
            laspj::Guard g(ctx);
            if (int s = laspj::lvar_ranks(ctx, S, K)) return s;
            if (int s = laspj::lvar_scratch(ctx, S, laspj::lv_isect_tiles(n))) return s;
            if (int s = map_fit(ctx, m, K.E)) return s;
            if (int s = map_rec_clean(ctx, m)) return s;
            if (int s = laspj::list_reserve(ctx, out->val, std::max(n, 1u), (uint32_t)ub_t)) return s;
            S->lv_ans[2] = 2;                                   // (not written yet)
            m->rec_dirty = true;
            LJ_HIP(ctx, laspj::launch_lm_map(ctx, map_args_dev(m, K), laspj::list_dev(out->val),
                                             static_cast<uint64_t*>(S->lv_tiles),
                                             reinterpret_cast<uint32_t*>(m->dev), S->lv_ans_d,
                                             false));
            m->rec_dirty = false;                               // (the writer zeroes it)
            // upper bounds until the bind's synchronisation brings the totals
            out->val->known_e = std::min(out->val->cap_e, std::max(n, 1u));
            out->val->known_t = (uint32_t)std::min<uint64_t>(out->val->cap_t, ub_t);
            out->val->not_asc = m->val_not_asc;
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
        // (a pass that emitted fewer entries emitted a sublist: what it learnt of the keys'
        // order holds for the whole list too)
        m->val_not_asc = out->val->not_asc;
        m->pmask_valid = true;
        if (S->lv_ans[2] != 0)
            return fail(ctx, LASPJ_E_RANGE, "map_run: the producer's output bound did not hold "
                        "(%u entries, %u tokens)", S->lv_ans[0], S->lv_ans[1]);
        out->val->known_e = S->lv_ans[0];
        out->val->known_t = S->lv_ans[1];
        *pending = S->lv_ans[3];
        if (*pending) return LASPJ_OK;                          // the merge is dropped
        if (S->lv_ans[4]) {
            // a present token the host had not named (the device is the source of truth):
            // every token of every evaluated slot, then the pass again
            if (attempt)
                return fail(ctx, LASPJ_E_DEVICE, "map_run: %u tokens stay unmapped", S->lv_ans[4]);
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

// laspj_map_args with S->mu held and the handle checked
int map_args_locked(laspj_ctx* ctx, NifState* S, laspj_map* m, const uint8_t** out,
                    uint64_t* out_len, uint32_t* count, int32_t* verdict) {
    if (int s = map_ready(ctx, S, m, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    KindState& K = *m->ns;
    std::vector<uint64_t> pm;
    if (K.dict && laspj::dict_elements(K.dict)) {
        if (int s = laspj::lvar_images(ctx, S, K)) return s;
        laspj::Guard g(ctx);
        const bool fitted = m->dev && m->E == K.E && m->up_lo > m->up_hi;
        if (!m->pmask_valid || !fitted) {
            // no run since the tables last changed: the count launch alone
            if (int s = laspj::lvar_scratch(ctx, S, laspj::lv_isect_tiles(K.built_K))) return s;
            if (int s = map_fit(ctx, m, K.E)) return s;
            m->rec_dirty = true;                                // (no writer behind it)
            LJ_HIP(ctx, laspj::launch_lm_map(ctx, map_args_dev(m, K), laspj::ListDev{},
                                             static_cast<uint64_t*>(S->lv_tiles),
                                             reinterpret_cast<uint32_t*>(m->dev), nullptr, true));
            ++S->stats[laspj::ST_PASSES];
            m->pmask_valid = true;
        }
        pm.resize(m->words);
        LJ_HIP(ctx, laspj::readback(ctx, pm.data(), map_pmask_d(m), 8ull * m->words));
    }
    std::vector<uint32_t> slots;
    laspj::proc_args_image(K, pm, m->h_eval, false, &slots, &m->image);
    m->listed.swap(slots);
    m->outstanding = true;
    m->dropped = false;
    *out = reinterpret_cast<const uint8_t*>(m->image.data());
    *out_len = m->image.size();
    *count = (uint32_t)m->listed.size();
    return LASPJ_OK;
}

// laspj_map_results past its checks: the results registered and the tables edited under one
// journal; *refused: rolled back, nothing recorded
int map_record(laspj_ctx* ctx, NifState* S, laspj_map* m, const std::vector<std::string_view>& res,
               bool* refused) {
    KindState& K = *m->ns;
    *refused = false;
    const laspj::RegMark mark = laspj::reg_mark(K);
    const uint64_t t0 = laspj::now_ns();
    const size_t rows0 = m->up_rows.size();
    const uint32_t lo0 = m->up_lo, hi0 = m->up_hi;
    MapUndo u;
    laspj::dict_begin(K.dict);
    int st = LASPJ_DEC_OK;
    map_host_fit(m, laspj::dict_elements(K.dict));
    // F(X) as an element slot of the input's namespace (one that exists already, or new)
    for (size_t k = 0; k < res.size() && st == LASPJ_DEC_OK; ++k) {
        const uint32_t e = m->listed[k];
        uint32_t y = 0;
        st = laspj::dict_reg_elem(K.dict, reinterpret_cast<const uint8_t*>(res[k].data()),
                                  res[k].size(), &y);
        if (st != LASPJ_DEC_OK) break;
        map_host_fit(m, laspj::dict_elements(K.dict));
        u.eds.push_back({0, e >> 6, m->h_eval[e >> 6]});
        m->h_eval[e >> 6] |= 1ull << (e & 63u);
        u.eds.push_back({1, e, m->h_ymap[e]});
        m->h_ymap[e] = y;
        m->up_lo = std::min(m->up_lo, e);
        m->up_hi = std::max(m->up_hi, e);
    }
    // then X's tokens as tokens of F(X)
    for (size_t k = 0; k < res.size() && st == LASPJ_DEC_OK; ++k)
        st = map_slot_tokens(m, K, m->listed[k], false, &u);
    S->stats[laspj::ST_NS_REGISTER] += laspj::now_ns() - t0;
    if (st != LASPJ_DEC_OK) {
        laspj::dict_rollback(K.dict);
        u.back(m);
        m->up_rows.resize(rows0);
        m->up_lo = lo0;
        m->up_hi = hi0;
        if (st == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "map_results: host allocation");
        m->refused = *refused = true;
        return LASPJ_OK;
    }
    laspj::dict_begin(K.dict);
    laspj::reg_note(S, K, mark);
    m->pmask_valid = false;
    return LASPJ_OK;
}

}  // namespace

namespace laspj {

void maps_var_gone(NifState* S, laspj_var* v) {
    for (laspj_map* m : S->maps)
        if (m->in == v) map_kill(v->ctx, m);
}

void maps_lvar_gone(NifState* S, laspj_lvar* lv) {
    for (laspj_map* m : S->maps)
        if (m->out == lv) {
            Guard g(lv->ctx);
            map_kill(lv->ctx, m);
        }
}

void maps_ctx_gone(laspj_ctx* ctx, NifState* S) {
    for (laspj_map* m : S->maps) {
        map_kill(ctx, m);
        m->ctx = nullptr;
    }
    S->maps.clear();
}

}  // namespace laspj

extern "C" {

int laspj_map_create(laspj_var* in, laspj_lvar* out, laspj_map** m) {
    if (!in || !out || !m) return LASPJ_E_INVAL;
    *m = nullptr;
    if (in->gc) {
        // riak_dt_gcounter is no type map/6 folds over
        laspj_ctx* c = out->ctx;
        return c ? fail(c, LASPJ_E_KIND, "map_create: an OR-Set variable") : LASPJ_E_KIND;
    }
    NifState* S = laspj::var_state(in);
    if (!S || !out->ctx) return LASPJ_E_INVAL;
    laspj_ctx* ctx = in->ctx;
    if (out->ctx != ctx) return fail(ctx, LASPJ_E_INVAL, "map_create: variables of different contexts");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(in) || !S->lvars.count(out)) return laspj::unknown_variable(ctx, "map_create");
    if (in->kind != LASPJ_KIND_ORSET)
        return fail(ctx, LASPJ_E_KIND, "map_create: an OR-Set variable (a list variable holds OR-Set lists)");
    if (out->pairs)
        return fail(ctx, LASPJ_E_KIND, "map_create: a pair-keyed list variable takes product/7's output only");
    if (in->ns != out->ns)
        return fail(ctx, LASPJ_E_UNSUPPORTED, "map_create: variables of one namespace");
    auto* p = new (std::nothrow) laspj_map;
    if (!p) return fail(ctx, LASPJ_E_NOMEM, "map_create: host allocation");
    p->ctx = ctx;
    p->in = in;
    p->out = out;
    p->ns = in->ns;
    p->epoch = in->ns->epoch;
    const int s = laspj::nomem_guard(ctx, "map_create", [&] {
        S->maps.insert(p);
        try {
            p->ns->maps.insert(p);
        } catch (const std::bad_alloc&) {
            S->maps.erase(p);
            throw;
        }
        return LASPJ_OK;
    }, "registry");
    if (s) {
        delete p;
        return s;
    }
    *m = p;
    return LASPJ_OK;
}

int laspj_map_destroy(laspj_map* m) {
    if (!m) return LASPJ_E_INVAL;
    if (NifState* S = map_state(m)) {
        std::lock_guard<std::mutex> lk(S->mu);
        if (m->ctx) {
            S->maps.erase(m);
            laspj::Guard g(m->ctx);
            map_kill(m->ctx, m);
        }
    }
    delete m;
    return LASPJ_OK;
}

int laspj_map_run(laspj_map* m, int32_t* status, uint32_t* pending, int32_t* verdict) {
    const laspj::Entry e = enter_map(m, "map_run", status && pending && verdict);
    if (e.rc) return e.rc;
    return laspj::nomem_guard(e.ctx, "map_run", [&] {
        return map_run_locked(e.ctx, e.S, m, status, pending, verdict);
    });
}

int laspj_map_args(laspj_map* m, const uint8_t** out, uint64_t* out_len, uint32_t* count,
                   int32_t* verdict) {
    const laspj::Entry e = enter_map(m, "map_args", out && out_len && count && verdict);
    if (e.rc) return e.rc;
    ++e.S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *count = 0;
    return laspj::nomem_guard(e.ctx, "map_args", [&] {
        return map_args_locked(e.ctx, e.S, m, out, out_len, count, verdict);
    });
}

int laspj_map_results(laspj_map* m, const uint8_t* results, uint64_t n, int32_t* verdict) {
    const laspj::Entry en = enter_map(m, "map_results", verdict != nullptr);
    if (en.rc) return en.rc;
    laspj_ctx* ctx = en.ctx;
    NifState* S = en.S;
    ++S->stats[laspj::ST_CALLS];
    *verdict = LASPJ_NIF_OK;
    map_sync(ctx, m);
    if (!m->outstanding) {
        if (m->dropped) {
            // a dictionary reset took the list: nothing recorded, the next run asks again
            m->dropped = false;
            return LASPJ_OK;
        }
        return fail(ctx, LASPJ_E_INVAL, "map_results: no argument list outstanding");
    }
    return laspj::nomem_guard(ctx, "map_results", [&]() -> int {
        std::vector<std::string_view> res;
        std::string bytes;
        if (!laspj::image_list(results, n, &res, &bytes) || res.size() != m->listed.size())
            return fail(ctx, LASPJ_E_INVAL, "map_results: %zu results for %zu arguments",
                        res.size(), m->listed.size());
        m->outstanding = false;
        bool refused = false;
        const int s = m->listed.empty() ? LASPJ_OK : map_record(ctx, S, m, res, &refused);
        m->listed.clear();
        if (s) return s;
        if (refused) {
            *verdict = LASPJ_NIF_FALLBACK;
            return laspj::fallback(S);
        }
        return LASPJ_OK;
    });
}

}  // extern "C"
