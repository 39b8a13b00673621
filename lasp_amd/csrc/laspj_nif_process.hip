// Resident processes (include/laspj.h "resident variables": laspj_filter_*,
// laspj_var_intersection):
// lasp_process:process/3 re-runs (lasp_process.erl:61-95) of the bodies whose outputs stay
// canonical values of the inputs' namespace: filter/6 (lasp_core.erl:681-712) with the fun's
// results kept beside the variable, and the G-Set intersection/7 (:569-576).  The kernels
// are laspj_process.hip's.

#include "laspj_nif_internal.h"

using laspj::fail;
using laspj::var_current;
using laspj::var_state;

namespace {

using laspj::KindState;
using laspj::NifState;
using laspj::ProcDesc;

// a 2-tuple element {A, B}: A's image length (0: not a 2-tuple); the bodies' `{X, _}`
// branch takes any such element, whatever the type (lasp_core.erl:688-695)
size_t first_of_pair(std::string_view img) {
    if (img.size() < 3 || (uint8_t)img[0] != 104 || (uint8_t)img[1] != 2) return 0;
    return laspj::list_term_len(reinterpret_cast<const uint8_t*>(img.data()) + 2, img.size() - 2);
}

// whether the namespace has registered a 2-tuple element: only the slots registered since
// the last look are read
bool ns_has_pair(KindState& K) {
    if (!K.dict) return false;
    const uint32_t n = laspj::dict_elements(K.dict);
    for (; K.pair_scanned < n && !K.has_pair; ++K.pair_scanned)
        K.has_pair = first_of_pair(laspj::list_elem_image(K.dict, K.pair_scanned)) != 0;
    return K.has_pair;
}

// `F(V) =:= true` on a result's image (any of the four atom encodings)
bool image_is_true(std::string_view v) {
    const uint8_t* p = reinterpret_cast<const uint8_t*>(v.data());
    if (v.size() == 7 && (p[0] == 100 || p[0] == 118) && p[1] == 0 && p[2] == 4)
        return std::memcmp(p + 3, "true", 4) == 0;
    if (v.size() == 6 && (p[0] == 115 || p[0] == 119) && p[1] == 4)
        return std::memcmp(p + 2, "true", 4) == 0;
    return false;
}

}  // namespace

bool laspj::image_list(const uint8_t* p, uint64_t n, std::vector<std::string_view>* out,
                       std::string* bytes) {
    out->clear();
    if (!p || n < 2 || p[0] != 131 || laspj::list_term_len(p + 1, n - 1) != n - 1) return false;
    const uint8_t* t = p + 1;
    const size_t tn = n - 1;
    if (t[0] == 106) return true;
    if (t[0] == 107) {
        const size_t cnt = ((size_t)t[1] << 8) | t[2];
        out->assign(cnt, std::string_view());
        if (bytes) {
            bytes->resize(2 * cnt);
            for (size_t i = 0; i < cnt; ++i) {
                (*bytes)[2 * i] = (char)97;
                (*bytes)[2 * i + 1] = (char)t[3 + i];
                (*out)[i] = std::string_view(bytes->data() + 2 * i, 2);
            }
        }
        return true;
    }
    if (t[0] != 108) return false;
    const uint32_t cnt = ((uint32_t)t[1] << 24) | ((uint32_t)t[2] << 16) | ((uint32_t)t[3] << 8) | t[4];
    size_t off = 5;
    for (uint32_t i = 0; i < cnt; ++i) {
        const size_t l = off < tn ? laspj::list_term_len(t + off, tn - off) : 0;
        if (!l) return false;
        out->emplace_back(reinterpret_cast<const char*>(t) + off, l);
        off += l;
    }
    return off < tn && t[off] == 106;
}

namespace {

using laspj::image_list;

// term images -> 131 + the list as term_to_binary/1 writes it (STRING_EXT for a list of
// integers 0..255, NIL_EXT when empty)
void image_write_list(const std::vector<std::string_view>& items, std::string* o) {
    o->assign(1, (char)131);
    const size_t n = items.size();
    if (!n) {
        o->push_back((char)106);
        return;
    }
    bool bytes = n < 65536;
    for (size_t i = 0; bytes && i < n; ++i) bytes = items[i].size() == 2 && (uint8_t)items[i][0] == 97;
    if (bytes) {
        o->push_back((char)107);
        o->push_back((char)(n >> 8));
        o->push_back((char)(n & 0xFF));
        for (const auto& it : items) o->push_back(it[1]);
        return;
    }
    o->push_back((char)108);
    for (int sh = 24; sh >= 0; sh -= 8) o->push_back((char)((n >> sh) & 0xFF));
    for (const auto& it : items) o->append(it.data(), it.size());
    o->push_back((char)106);
}

}  // namespace

hipError_t laspj::proc_upload(laspj_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    if (!bytes) return hipSuccess;
    const void* staged = laspj::stage_small(ctx, src, bytes);
    return hipMemcpyAsync(dst, staged ? staged : src, bytes, hipMemcpyHostToDevice, ctx->stream);
}

void laspj::proc_args_image(const KindState& K, const std::vector<uint64_t>& pm,
                            const std::vector<uint64_t>& h_eval, bool pair_first,
                            std::vector<uint32_t>* slots, std::string* image) {
    // the pending slots (results recorded since the pass taken off) in term order: the
    // order the body calls F in over a canonical value
    slots->clear();
    const uint32_t known = K.dict ? laspj::dict_elements(K.dict) : 0;
    for (uint32_t w = 0; w < pm.size(); ++w)
        for (uint64_t m = pm[w] & ~(w < h_eval.size() ? h_eval[w] : 0ull); m; m &= m - 1) {
            const uint32_t e = 64u * w + (uint32_t)__builtin_ctzll(m);
            if (e < known) slots->push_back(e);
        }
    auto img = [&](uint32_t e) { return laspj::list_elem_image(K.dict, e); };
    std::sort(slots->begin(), slots->end(), [&](uint32_t a, uint32_t b) {
        const std::string_view x = img(a), y = img(b);
        int c = 0;
        laspj_term_compare(reinterpret_cast<const uint8_t*>(x.data()), x.size(),
                           reinterpret_cast<const uint8_t*>(y.data()), y.size(), &c);
        return c < 0;
    });
    // F's argument: the element; a G-Set 2-tuple element's first component
    std::vector<std::string_view> items;
    items.reserve(slots->size());
    for (uint32_t e : *slots) {
        const std::string_view x = img(e);
        const size_t l0 = pair_first ? first_of_pair(x) : 0;
        items.push_back(l0 ? x.substr(2, l0) : x);
    }
    image_write_list(items, image);
}

namespace {

using laspj::proc_upload;

// the filter's context state; null: the context is gone
NifState* filter_state(laspj_filter* f) {
    if (!f || !f->ctx) return nullptr;
    return laspj::state(f->ctx);
}

// (S->mu held) the handle is this context's and both its variables are alive
bool filter_alive(const NifState* S, laspj_filter* f) {
    return f && S->filters.count(f) && f->in && f->out;
}

// a filter call's opening (laspj::enter, then the handle checked under the call lock)
laspj::Entry enter_filter(laspj_filter* f, const char* name, bool args_ok) {
    laspj::Entry e = laspj::enter(filter_state(f), f ? f->ctx : nullptr, name, args_ok);
    if (e.rc == LASPJ_OK && !filter_alive(e.S, f))
        e.rc = fail(e.ctx, LASPJ_E_INVAL, "%s: a variable of the filter was destroyed", name);
    return e;
}

// The tables follow the namespace's generation: a dictionary reset renumbers the element
// slots, so both bitmaps start over and an outstanding argument list is dropped (F is
// asked again, which a pure fun allows).  Call without ctx->mu held.
void filter_sync(laspj_ctx* ctx, laspj_filter* f) {
    if (f->epoch == f->ns->epoch) return;
    if (f->dev) {
        laspj::Guard g(ctx);
        laspj::dev_release(ctx, f->dev, f->dev_bytes);
    }
    f->dev = nullptr;
    f->dev_bytes = 0;
    f->words = 0;
    f->h_eval.clear();
    f->h_keep.clear();
    f->pmask_valid = false;
    f->listed.clear();
    if (f->outstanding) f->dropped = true;
    f->outstanding = false;
    f->epoch = f->ns->epoch;
}

// the tables sized to the namespace's E element slots (growth extends them with zeros:
// slots are append-only within a generation); ctx->mu held
int filter_fit(laspj_ctx* ctx, laspj_filter* f, uint32_t E) {
    const uint32_t words = (E + 63u) / 64u;
    if (f->dev && f->words == words) return LASPJ_OK;
    const int grown = laspj::nomem_guard(ctx, "filter", [&] {
        f->h_eval.resize(words, 0);
        f->h_keep.resize(words, 0);
        return LASPJ_OK;
    }, "host tables");
    if (grown) return grown;
    const uint64_t bytes = std::max<uint64_t>(24ull * words, 256);
    void* p = nullptr;
    if (laspj::dev_alloc(ctx, bytes, &p) != hipSuccess) {
        hipGetLastError();
        return fail(ctx, LASPJ_E_NOMEM, "filter: device tables (%llu bytes)",
                    (unsigned long long)bytes);
    }
    uint64_t* d = static_cast<uint64_t*>(p);
    hipError_t e = proc_upload(ctx, d, f->h_eval.data(), 8ull * words);
    if (e == hipSuccess) e = proc_upload(ctx, d + words, f->h_keep.data(), 8ull * words);
    if (e != hipSuccess) {
        laspj::dev_release(ctx, p, bytes);
        return fail(ctx, LASPJ_E_DEVICE, "filter: table upload: %s", hipGetErrorString(e));
    }
    if (f->dev) laspj::dev_release(ctx, f->dev, f->dev_bytes);
    f->dev = d;
    f->dev_bytes = bytes;
    f->words = words;
    f->pmask_valid = false;
    return LASPJ_OK;
}

// one device pass over some processes: their descriptors, the records read back, the device
// block (records, then the descriptors of a launch over many) kept for the write launch;
// lives inside a Guard
struct ProcPass {
    laspj_ctx* ctx;
    std::vector<uint32_t> live;     // the filters (indices of the call) with a descriptor
    std::vector<ProcDesc> descs;
    std::vector<uint32_t> rec;      // {pending, changed} per descriptor
    uint32_t blocks = 0;
    void* blk = nullptr;
    uint64_t blk_bytes = 0, desc_off = 0;
    explicit ProcPass(laspj_ctx* c) : ctx(c) {}
    ~ProcPass() {
        if (blk) laspj::dev_release(ctx, blk, blk_bytes);
    }
};

hipError_t proc_launch(laspj_ctx* ctx, const ProcPass& P, uint32_t pass) {
    uint32_t* rec = static_cast<uint32_t*>(P.blk);
    if (P.descs.size() == 1) return laspj::launch_proc_one(ctx, P.descs[0], rec, pass);
    const auto* dd = reinterpret_cast<const ProcDesc*>(static_cast<uint8_t*>(P.blk) + P.desc_off);
    return laspj::launch_proc_many(ctx, dd, (uint32_t)P.descs.size(), P.blocks, rec, pass);
}

// (ctx->mu held) P's descriptors through a check or fused pass: the records zeroed, one
// launch, the records read back in the call's one synchronisation (P->rec)
int proc_pass(laspj_ctx* ctx, NifState* S, ProcPass* P, uint32_t pass) {
    const uint32_t m = (uint32_t)P->descs.size();
    const uint64_t t0 = laspj::now_ns();
    P->desc_off = laspj::al(8ull * m, 256);
    P->blk_bytes = P->desc_off + (m > 1 ? sizeof(ProcDesc) * (uint64_t)m : 0);
    if (laspj::dev_alloc(ctx, P->blk_bytes, &P->blk) != hipSuccess) {
        hipGetLastError();
        P->blk = nullptr;
        return fail(ctx, LASPJ_E_NOMEM, "process pass: records");
    }
    P->rec.assign(2ull * m, 0);
    LJ_HIP(ctx, hipMemsetAsync(P->blk, 0, 8ull * m, ctx->stream));
    if (m > 1)
        LJ_HIP(ctx, proc_upload(ctx, static_cast<uint8_t*>(P->blk) + P->desc_off, P->descs.data(),
                                sizeof(ProcDesc) * (uint64_t)m));
    LJ_HIP(ctx, proc_launch(ctx, *P, pass));
    const uint64_t t1 = laspj::now_ns();
    LJ_HIP(ctx, laspj::readback(ctx, P->rec.data(), P->blk, 8ull * m));
    ++S->stats[laspj::ST_PASSES];
    S->stats[laspj::ST_NS_ENQUEUE] += t1 - t0;
    S->stats[laspj::ST_NS_WAIT] += laspj::now_ns() - t1;
    return LASPJ_OK;
}

// the variables of n filters brought onto the device (S->mu held, ctx->mu not): verdict[i]
// FALLBACK (counted) when in or out stays host-held, else the filter's tables follow the
// namespace's generation
int filters_ready(laspj_ctx* ctx, NifState* S, uint32_t n, laspj_filter* const* fs,
                  int32_t* verdict) {
    for (uint32_t i = 0; i < n; ++i) {
        bool a = false, b = false;
        if (int s = laspj::hydrate(ctx, S, fs[i]->in, &a)) return s;
        if (int s = laspj::hydrate(ctx, S, fs[i]->out, &b)) return s;
        verdict[i] = a && b ? LASPJ_NIF_OK : LASPJ_NIF_FALLBACK;
    }
    for (uint32_t i = 0; i < n; ++i) {
        // (a decode above may have started a dictionary afresh and written cells decoded
        // before it out again: such a filter answers FALLBACK this once)
        if (verdict[i] == LASPJ_NIF_OK && !(var_current(fs[i]->in) && var_current(fs[i]->out)))
            verdict[i] = LASPJ_NIF_FALLBACK;
        if (verdict[i] == LASPJ_NIF_OK) filter_sync(ctx, fs[i]);
        else ++S->stats[laspj::ST_FALLBACKS];
    }
    return LASPJ_OK;
}

// (ctx->mu held) the check pass of the filters whose verdict is OK: cells and tables fitted
// to the namespace, one launch, one synchronisation; P->rec answers, in P->live's order.
// A namespace with no element yet takes no part (nothing held: pending 0, NOOP).
int filters_check(laspj_ctx* ctx, NifState* S, uint32_t n, laspj_filter* const* fs,
                  const int32_t* verdict, ProcPass* P) {
    for (uint32_t i = 0; i < n; ++i) {
        laspj_filter* f = fs[i];
        if (verdict[i] != LASPJ_NIF_OK) continue;
        const KindState& K = *f->ns;
        if (!K.dict || K.E == 0) continue;
        const uint32_t tw = laspj::ktw(K);
        if (int s = laspj::fit_var(ctx, f->in, K.E, tw)) return s;
        if (int s = laspj::fit_var(ctx, f->out, K.E, tw)) return s;
        if (int s = filter_fit(ctx, f, K.E)) return s;
        const bool gset = f->in->kind == LASPJ_KIND_GSET;
        ProcDesc d;
        d.in = f->in->cells;
        d.out = f->out->cells;
        d.evaluated = f->dev;
        d.keep = f->dev + f->words;
        d.pmask = f->dev + 2ull * f->words;
        d.n = gset ? f->words : K.E;
        d.tw = gset ? 1 : tw;
        d.mode = gset ? laspj::kProcGset : tw > 1 ? laspj::kProcWide : laspj::kProcNarrow;
        d.block0 = P->blocks;
        P->blocks += laspj::proc_blocks(d);
        P->descs.push_back(d);
        P->live.push_back(i);
    }
    if (P->descs.empty()) return LASPJ_OK;
    if (int s = proc_pass(ctx, S, P, laspj::kProcCheck)) return s;
    for (uint32_t i : P->live) fs[i]->pmask_valid = true;
    return LASPJ_OK;
}

// laspj_filter_run / _run_many with S->mu held and the handles checked
int filter_run_locked(laspj_ctx* ctx, NifState* S, uint32_t n, laspj_filter* const* fs,
                      int32_t* status, uint32_t* pending, int32_t* verdict) {
    ++S->stats[laspj::ST_CALLS];
    for (uint32_t i = 0; i < n; ++i) {
        status[i] = LASPJ_BIND_NOOP;
        pending[i] = 0;
    }
    if (int s = filters_ready(ctx, S, n, fs, verdict)) return s;
    laspj::Guard g(ctx);
    ProcPass P(ctx);
    if (int s = filters_check(ctx, S, n, fs, verdict, &P)) return s;
    bool any = false;
    for (size_t a = 0; a < P.live.size(); ++a) {
        const uint32_t i = P.live[a];
        pending[i] = P.rec[2 * a];
        // F's result for some held element is not on the device: out stays as it is
        if (pending[i] == 0 && P.rec[2 * a + 1]) {
            status[i] = LASPJ_BIND_WRITTEN;
            lazy_clear(S, fs[i]->out, true);
            any = true;
        }
    }
    // out |= AccValue of the filters known ready and unequal, behind the readback: the
    // stream orders it ahead of every later use, so no second synchronisation
    if (any) LJ_HIP(ctx, proc_launch(ctx, P, laspj::kProcWrite));
    return LASPJ_OK;
}

// laspj_filter_run_many with S->mu held: the handles checked, then the pass
int filter_run_many_locked(laspj_ctx* ctx, NifState* S, uint32_t n, laspj_filter* const* fs,
                           int32_t* status, uint32_t* pending, int32_t* verdict) {
    std::unordered_set<const void*> seen, outs;
    for (uint32_t i = 0; i < n; ++i) {
        if (!fs[i] || fs[i]->ctx != ctx || !filter_alive(S, fs[i]))
            return fail(ctx, LASPJ_E_INVAL, "filter_run: filter %u is not a live one of this context", i);
        if (!seen.insert(fs[i]).second)
            return fail(ctx, LASPJ_E_INVAL, "filter_run: filter %u named twice", i);
        if (!outs.insert(fs[i]->out).second)
            return fail(ctx, LASPJ_E_INVAL, "filter_run: filter %u shares its out (the binds would race)", i);
    }
    // (one's out read as another's in would see a half-written value in the same pass)
    for (uint32_t i = 0; i < n; ++i)
        if (fs[i]->in != fs[i]->out && outs.count(fs[i]->in))
            return fail(ctx, LASPJ_E_INVAL, "filter_run: filter %u reads another's out", i);
    return filter_run_locked(ctx, S, n, fs, status, pending, verdict);
}

// laspj_filter_args with S->mu held and the handle checked
int filter_args_locked(laspj_ctx* ctx, NifState* S, laspj_filter* f, const uint8_t** out,
                       uint64_t* out_len, uint32_t* count, int32_t* verdict) {
    if (int s = filters_ready(ctx, S, 1, &f, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    const KindState& K = *f->ns;
    std::vector<uint64_t> pm;
    if (K.dict && K.E) {
        laspj::Guard g(ctx);
        if (!f->pmask_valid) {
            // no run since the tables last changed size or generation: the check pass here
            ProcPass P(ctx);
            if (int s = filters_check(ctx, S, 1, &f, verdict, &P)) return s;
        }
        pm.resize(f->words);
        LJ_HIP(ctx, laspj::readback(ctx, pm.data(), f->dev + 2ull * f->words, 8ull * f->words));
    }
    std::vector<uint32_t> slots;
    laspj::proc_args_image(K, pm, f->h_eval, f->in->kind == LASPJ_KIND_GSET, &slots, &f->image);
    f->listed.swap(slots);
    f->outstanding = true;
    f->dropped = false;
    *out = reinterpret_cast<const uint8_t*>(f->image.data());
    *out_len = f->image.size();
    *count = (uint32_t)f->listed.size();
    return LASPJ_OK;
}

}  // namespace

extern "C" {

int laspj_filter_create(laspj_var* in, laspj_var* out, laspj_filter** f) {
    if (!in || !out || !f) return LASPJ_E_INVAL;
    *f = nullptr;
    if (in->gc || out->gc) {
        // riak_dt_gcounter is no type filter/6 folds over
        laspj_ctx* c = in->ctx ? in->ctx : out->ctx;
        return c ? fail(c, LASPJ_E_KIND, "filter_create: OR-Set or G-Set variables")
                 : LASPJ_E_KIND;
    }
    NifState* S = var_state(in);
    if (!S || !out->ctx) return LASPJ_E_INVAL;
    laspj_ctx* ctx = in->ctx;
    if (out->ctx != ctx)
        return fail(ctx, LASPJ_E_INVAL, "filter_create: variables of different contexts");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(in) || !S->vars.count(out))
        return laspj::unknown_variable(ctx, "filter_create");
    if (in->kind != out->kind)
        return fail(ctx, LASPJ_E_KIND, "filter_create: variables of one kind");
    if (in->ns != out->ns)
        return fail(ctx, LASPJ_E_UNSUPPORTED, "filter_create: variables of one namespace");
    auto* p = new (std::nothrow) laspj_filter;
    if (!p) return fail(ctx, LASPJ_E_NOMEM, "filter_create: host allocation");
    p->ctx = ctx;
    p->in = in;
    p->out = out;
    p->ns = in->ns;
    p->epoch = in->ns->epoch;
    const int s = laspj::nomem_guard(ctx, "filter_create", [&] {
        S->filters.insert(p);
        return LASPJ_OK;
    }, "registry");
    if (s) {
        delete p;
        return s;
    }
    *f = p;
    return LASPJ_OK;
}

int laspj_filter_destroy(laspj_filter* f) {
    if (!f) return LASPJ_E_INVAL;
    if (NifState* S = filter_state(f)) {
        std::lock_guard<std::mutex> lk(S->mu);
        if (f->ctx) {
            S->filters.erase(f);
            if (f->dev) {
                laspj::Guard g(f->ctx);
                laspj::dev_release(f->ctx, f->dev, f->dev_bytes);
            }
        }
    }
    delete f;
    return LASPJ_OK;
}

int laspj_filter_run(laspj_filter* f, int32_t* status, uint32_t* pending, int32_t* verdict) {
    const laspj::Entry e = enter_filter(f, "filter_run", status && pending && verdict);
    if (e.rc) return e.rc;
    return laspj::nomem_guard(e.ctx, "filter_run", [&] {
        return filter_run_locked(e.ctx, e.S, 1, &f, status, pending, verdict);
    });
}

int laspj_filter_run_many(laspj_ctx* ctx, uint32_t n, laspj_filter* const* fs, int32_t* status,
                          uint32_t* pending, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!n) return LASPJ_OK;
    if (!fs || !status || !pending || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "filter_run: null array");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    return laspj::nomem_guard(ctx, "filter_run", [&] {
        return filter_run_many_locked(ctx, e.S, n, fs, status, pending, verdict);
    });
}

int laspj_filter_args(laspj_filter* f, const uint8_t** out, uint64_t* out_len, uint32_t* count,
                      int32_t* verdict) {
    const laspj::Entry e = enter_filter(f, "filter_args", out && out_len && count && verdict);
    if (e.rc) return e.rc;
    ++e.S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *count = 0;
    return laspj::nomem_guard(e.ctx, "filter_args", [&] {
        return filter_args_locked(e.ctx, e.S, f, out, out_len, count, verdict);
    });
}

int laspj_filter_results(laspj_filter* f, const uint8_t* results, uint64_t n) {
    const laspj::Entry en = enter_filter(f, "filter_results", true);
    if (en.rc) return en.rc;
    laspj_ctx* ctx = en.ctx;
    ++en.S->stats[laspj::ST_CALLS];
    filter_sync(ctx, f);
    if (!f->outstanding) {
        if (f->dropped) {
            // a dictionary reset took the list: nothing recorded, the next run asks again
            f->dropped = false;
            return LASPJ_OK;
        }
        return fail(ctx, LASPJ_E_INVAL, "filter_results: no argument list outstanding");
    }
    std::vector<std::string_view> res;
    bool parsed = false;
    const int walked = laspj::nomem_guard(ctx, "filter_results", [&] {
        parsed = image_list(results, n, &res);
        return LASPJ_OK;
    });
    if (walked) return walked;
    if (!parsed || res.size() != f->listed.size())
        return fail(ctx, LASPJ_E_INVAL, "filter_results: %zu results for %zu arguments",
                    res.size(), f->listed.size());
    f->outstanding = false;
    if (f->listed.empty()) return LASPJ_OK;
    uint32_t w0 = ~0u, w1 = 0;
    for (size_t k = 0; k < res.size(); ++k) {
        const uint32_t e = f->listed[k], w = e >> 6;
        f->h_eval[w] |= 1ull << (e & 63u);
        if (image_is_true(res[k])) f->h_keep[w] |= 1ull << (e & 63u);
        w0 = std::min(w0, w);
        w1 = std::max(w1, w);
    }
    f->listed.clear();
    if (!f->dev) return LASPJ_OK;
    // the words that changed, to both device bitmaps (enqueued: the next run is behind them)
    laspj::Guard g(ctx);
    const uint64_t bytes = 8ull * (w1 - w0 + 1);
    LJ_HIP(ctx, proc_upload(ctx, f->dev + w0, f->h_eval.data() + w0, bytes));
    LJ_HIP(ctx, proc_upload(ctx, f->dev + f->words + w0, f->h_keep.data() + w0, bytes));
    return LASPJ_OK;
}

int laspj_var_intersection(laspj_var* out, laspj_var* l, laspj_var* r, int32_t* status,
                           int32_t* verdict) {
    if (out && out->gc) {
        // riak_dt_gcounter is no type lasp_core:intersection/7 takes: the NIF runs the reference's
        if (!l || !r || !status) return LASPJ_E_INVAL;
        *status = LASPJ_BIND_NOOP;
        return laspj::gc_refuse(out->gc, verdict);
    }
    NifState* S = var_state(out);
    if (!S || !l || !r) return LASPJ_E_INVAL;
    laspj_ctx* ctx = out->ctx;
    if (!status || !verdict) return fail(ctx, LASPJ_E_INVAL, "var_intersection: null argument");
    if (l->ctx != ctx || r->ctx != ctx)
        return fail(ctx, LASPJ_E_INVAL, "var_intersection: variables of different contexts");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(out) || !S->vars.count(l) || !S->vars.count(r))
        return laspj::unknown_variable(ctx, "var_intersection");
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    // G-Sets of one namespace only: the OR-Set body's `Cx ++ Cy` is a list value, and cells
    // of two namespaces name different terms by one slot
    if (out->kind != LASPJ_KIND_GSET || l->kind != LASPJ_KIND_GSET ||
        r->kind != LASPJ_KIND_GSET || l->ns != out->ns || r->ns != out->ns)
        return laspj::fallback(S);
    for (laspj_var* v : {out, l, r}) {
        bool ok = false;
        if (int s = laspj::hydrate(ctx, S, v, &ok)) return s;
        if (!ok) return laspj::fallback(S);
    }
    for (laspj_var* v : {out, l, r})
        if (!var_current(v)) return laspj::fallback(S);
    KindState& K = *out->ns;
    // a 2-tuple element goes down the body's OR-Set branch (keyfind, then ++ on a causality
    // that is no list): the reference's to run, as on the image path
    if (ns_has_pair(K)) return laspj::fallback(S);
    *verdict = LASPJ_NIF_OK;
    if (!K.dict || K.E == 0) return LASPJ_OK;             // three new() values
    laspj::Guard g(ctx);
    for (laspj_var* v : {out, l, r})
        if (int s = laspj::fit_var(ctx, v, K.E, 1)) return s;
    ProcPass P(ctx);
    ProcDesc d;
    d.in = l->cells;
    d.out = out->cells;
    d.keep = r->cells;                                    // [X || lists:member(X, RValue)]
    d.evaluated = nullptr;
    d.pmask = nullptr;
    d.n = (K.E + 63u) / 64u;
    d.tw = 1;
    d.mode = laspj::kProcGset;
    d.block0 = 0;
    P.descs.push_back(d);
    P.blocks = laspj::proc_blocks(d);
    if (int s = proc_pass(ctx, S, &P, laspj::kProcFused)) return s;
    *status = P.rec[1] ? LASPJ_BIND_WRITTEN : LASPJ_BIND_NOOP;
    if (P.rec[1]) lazy_clear(S, out, true);
    return LASPJ_OK;
}

}  // extern "C"
