// Device-resident variables (include/laspj.h "resident variables"): their lifecycle,
// the group-commit bind queue, write / read / value / threshold, union/7 and update/4 with
// their kernels.  The passes themselves are laspj_nif.hip's run().

#include "laspj_nif_internal.h"

namespace laspj {
namespace {

// lasp_core:update/4 (lasp_core.erl:283-312) of one call on a resident variable's cells:
// Type:update/3 (lasp_orset.erl:99-117, 222-259; lasp_gset.erl:84-88) — the ops in order, all
// or nothing — then bind/3 of its Value, which writes merge(Value0, Value).  lasp_orset:merge
// ORs the flags of a token both hold (lasp_orset.erl:128-136), so per token bit the call gives
// p' = p0 | pV, r' = r0 | rV: an ADD by a token Value0 holds removed leaves it removed (update/3
// alone stores `false`, the bind's merge makes it `true` again), and an ADD after a REMOVE of
// its element in the same call takes the bit back to r0, not to the 1 the REMOVE put there.
// A REMOVE whose element is absent — not in the cells and not added earlier in the
// call — fails the call ({error, {precondition, {not_present, E}}}, remove_elems / apply_ops
// stop there and the state is kept); element 0xFFFFFFFF is an element the dictionary has
// never held.  Few ops travel as kernel arguments (no upload on the update path); one lane
// walks them (a call is a handful of ops).  tw {p, r} pairs per element (a wide namespace:
// token slot t in pair t / 64, the slot's bits 8..15 in the op's pad byte).
constexpr uint32_t kUpdArgOps = 24;
struct UpdArgs {
    laspj_op op[kUpdArgOps];
};
constexpr uint32_t kNoElem = 0xFFFFFFFFu;

__device__ inline uint32_t op_slot(const laspj_op& o) { return o.slot | (uint32_t)o.pad << 8; }

__global__ void __launch_bounds__(64) k_var_update(uint64_t* __restrict__ cells, int32_t kind,
                                                   uint32_t tw, UpdArgs a,
                                                   const laspj_op* __restrict__ dops,
                                                   uint32_t nops, int32_t* __restrict__ status) {
    if (threadIdx.x != 0) return;
    auto op = [&](uint32_t k) -> laspj_op { return dops ? dops[k] : a.op[k]; };
    uint32_t bad = nops;
    if (kind == LASPJ_KIND_ORSET) {
        for (uint32_t k = 0; k < nops && bad == nops; ++k) {
            const laspj_op o = op(k);
            if (o.kind != LASPJ_OP_REMOVE) continue;
            bool present = false;
            if (o.element != kNoElem)
                for (uint32_t j = 0; j < tw && !present; ++j)
                    present = cells[2ull * ((uint64_t)o.element * tw + j)] != 0;
            for (uint32_t j = 0; j < k && !present; ++j) {
                const laspj_op q = op(j);
                present = q.kind == LASPJ_OP_ADD && q.element == o.element;
            }
            if (!present) bad = k;
        }
    }
    // a call with a REMOVE (status is its answer array): every ADD's removed bit as Value0
    // has it, read before the first op lands and parked in the op's status word
    const bool keep_r0 = kind == LASPJ_KIND_ORSET && status && bad == nops;
    if (keep_r0)
        for (uint32_t k = 0; k < nops; ++k) {
            const laspj_op o = op(k);
            if (o.kind != LASPJ_OP_ADD) continue;
            const uint32_t t = op_slot(o);
            status[k] = (int32_t)(cells[2ull * ((uint64_t)o.element * tw + (t >> 6)) + 1] >>
                                  (t & 63u) & 1u);
        }
    for (uint32_t k = 0; k < nops; ++k) {
        if (bad < nops) {
            if (status) status[k] = k == bad ? LASPJ_OPST_NOT_PRESENT : LASPJ_OPST_ROLLED_BACK;
            continue;
        }
        const laspj_op o = op(k);
        if (kind == LASPJ_KIND_ORSET) {
            uint64_t* c = cells + 2ull * (uint64_t)o.element * tw;
            if (o.kind == LASPJ_OP_ADD) {
                // orddict:store(Token, false, Tokens) merged with Value0: present, the flag
                // Value0's (without a REMOVE in the call the word still holds it)
                const uint32_t t = op_slot(o);
                const uint64_t bit = 1ull << (t & 63u);
                c[2 * (t >> 6)] |= bit;
                if (keep_r0) {
                    uint64_t& r = c[2 * (t >> 6) + 1];
                    r = status[k] ? r | bit : r & ~bit;
                }
            } else {
                for (uint32_t j = 0; j < tw; ++j)
                    c[2 * j + 1] = c[2 * j];           // every token of Elem := true
            }
        } else {
            cells[o.element >> 6] |= 1ull << (o.element & 63u);
        }
        if (status) status[k] = LASPJ_OPST_APPLIED;
    }
}

// the same for a call of ADDs only (add_all over many elements): commutative, one op per
// lane; with no REMOVE in the call every removed bit stays Value0's
__global__ void __launch_bounds__(256) k_var_adds(uint64_t* __restrict__ cells, int32_t kind,
                                                  uint32_t tw, const laspj_op* __restrict__ ops,
                                                  uint32_t nops) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nops) return;
    const laspj_op o = ops[k];
    if (kind == LASPJ_KIND_ORSET) {
        const uint32_t t = op_slot(o);
        unsigned long long* c = reinterpret_cast<unsigned long long*>(
            cells + 2ull * ((uint64_t)o.element * tw + (t >> 6)));
        atomicOr(c, 1ull << (t & 63u));
    } else {
        atomicOr(reinterpret_cast<unsigned long long*>(cells + (o.element >> 6)),
                 1ull << (o.element & 63u));
    }
}

// lasp_core:union/7's body for OR-Sets (lasp_core.erl:602-627: orddict:merge keeping the
// left value of a key both hold) over resident l and r, bound into out (bind/3, :291-312:
// out := merge(out, AccValue), the OR of the cells): per element slot, l's cell where l
// holds the element (any pair's present word nonzero), else r's; *changed set when
// `Value0 =:= AccValue` fails (the bind's no-op test: canonical values of one namespace
// are equal exactly when their cells are; a wave's lanes agree on one atomic).  tw pairs
// per element.
// (out may be l or r: no restrict)
__global__ void __launch_bounds__(256) k_var_union(uint64_t* out, const uint64_t* l,
                                                   const uint64_t* r, uint32_t E, uint32_t tw,
                                                   uint32_t* __restrict__ changed) {
    const uint32_t e = blockIdx.x * blockDim.x + threadIdx.x;
    bool ch = false;
    if (e < E) {
        const uint64_t base = 2ull * e * tw;
        bool inl = false;
        for (uint32_t j = 0; j < tw; ++j) inl |= l[base + 2 * j] != 0;
        const uint64_t* src = inl ? l : r;
        for (uint32_t j = 0; j < tw; ++j) {
            const uint64_t op = out[base + 2 * j], oq = out[base + 2 * j + 1];
            const uint64_t ap = src[base + 2 * j], aq = src[base + 2 * j + 1];
            ch |= op != ap || oq != aq;                    // Value0 =/= AccValue
            if ((op | ap) != op || (oq | aq) != oq) {
                out[base + 2 * j] = op | ap;
                out[base + 2 * j + 1] = oq | aq;
            }
        }
    }
    if (__ballot(ch) && (threadIdx.x & 63u) == 0) atomicOr(changed, 1u);
}

// passes a group-commit leader runs back to back while binds keep queueing
constexpr int kLeadRounds = 8;
// waiters' staging blocks: payloads of at least kPinMin bytes, at most kPinSlots blocks
constexpr uint64_t kPinMin = 64ull << 10;
constexpr uint32_t kPinSlots = 64;

// a waiter's pinned block grown to `need` bytes (false: no pinned memory; the leader then
// copies that payload itself)
bool pin_grow(PinSlot* s, uint64_t need) {
    if (s->h) hipHostFree(s->h);
    *s = PinSlot{};
    const uint64_t cap = std::max<uint64_t>((need + (1ull << 20) - 1) & ~((1ull << 20) - 1), 1ull << 20);
    void* h = nullptr;
    if (hipHostMalloc(&h, cap, hipHostMallocCoherent) != hipSuccess) {
        hipGetLastError();
        return false;
    }
    void* d = nullptr;
    if (hipHostGetDevicePointer(&d, h, 0) != hipSuccess) {
        hipGetLastError();
        hipHostFree(h);
        return false;
    }
    *s = PinSlot{static_cast<uint8_t*>(h), static_cast<const uint8_t*>(d), cap};
    return true;
}

}  // namespace

// A variable whose value sits in its host image (written out by a dictionary reset) gets
// cells again: write/4 of that image.  *ok: the variable is resident over the current
// dictionary (false: it stays host-held; its calls answer FALLBACK)
int hydrate(laspj_ctx* ctx, NifState* S, laspj_var* v, bool* ok) {
    KindState& K = *v->ns;
    *ok = v->resident && v->epoch == K.epoch;
    // (a value write/4 could not represent stays an image until the next write)
    if (*ok || v->image.empty() || v->held) return LASPJ_OK;
    const std::vector<uint8_t> img = v->image;
    Call c = var_call(Op::WRITE, v, img.data(), img.size());
    {
        Guard g(ctx);
        release_cells(ctx, v);
    }
    v->resident = true;                   // (fit_var gives it zeroed cells)
    v->epoch = K.epoch;
    std::vector<int32_t> vd;
    const int s = run(ctx, S, c, &vd);
    if (s == LASPJ_OK && vd[0] == LASPJ_NIF_OK) {
        v->image.clear();
        v->image.shrink_to_fit();
        *ok = true;
        ++S->stats[ST_HYDRATED];
        return LASPJ_OK;
    }
    // (a reset inside the call may have written the empty cells out over the image)
    v->image = img;
    v->resident = false;
    v->held = s == LASPJ_OK;
    {
        Guard g(ctx);
        release_cells(ctx, v);
    }
    return s;
}

// the variable's context state (its S->mu is taken by the caller)
laspj::NifState* var_state(laspj_var* v) {
    if (!v || !v->ctx) return nullptr;
    return laspj::state(v->ctx);
}

// a variable in namespace `ns` (a fresh one when null); call with S->mu held
int var_new(laspj_ctx* ctx, laspj::NifState* S, int32_t kind,
            std::shared_ptr<laspj::KindState> ns, laspj_var** out) {
    auto* v = new (std::nothrow) laspj_var;
    if (!v) return fail(ctx, LASPJ_E_NOMEM, "var_create: host allocation");
    v->ctx = ctx;
    v->kind = kind;
    const int s = laspj::nomem_guard(ctx, "var_create", [&]() -> int {
        if (!ns) {
            ns = std::make_shared<laspj::KindState>();
            ns->kind = kind;
        }
        v->ns = ns;
        if (!ns->dict && laspj::reset_dict(ctx, S, *ns)) return LASPJ_E_NOMEM;
        v->epoch = ns->epoch;         // new(): no cells until the first call sizes them
        S->vars.insert(v);
        try {
            ns->vars.insert(v);
        } catch (const std::bad_alloc&) {
            S->vars.erase(v);
            throw;
        }
        return LASPJ_OK;
    }, "registry");
    if (s) {
        delete v;
        return s;
    }
    *out = v;
    return LASPJ_OK;
}

// write/4 builds a fresh #dv (lasp_core.erl:842-843): the variable's lazy threads go, their
// hidden cells with them (S->mu held; locked: ctx->mu is held too)
void lazy_clear(laspj::NifState* S, laspj_var* v, bool locked) {
    if (v->lazy.empty()) return;
    for (laspj::Waiter& z : v->lazy) {
        laspj_var* c = z.cells;
        if (c && c->ctx) {
            S->vars.erase(c);
            c->ns->vars.erase(c);
            if (locked) {
                laspj::release_cells(c->ctx, c);
            } else {
                std::lock_guard<std::mutex> lk(c->ctx->mu);
                hipSetDevice(c->ctx->device);
                laspj::release_cells(c->ctx, c);
            }
        }
        delete c;
    }
    v->lazy.clear();
}

// the kinds named in a list of variables: bit 0 sets, bit 1 counters
int kinds_of(uint32_t n, laspj_var* const* vars) {
    int k = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (vars[i]) k |= vars[i]->gc ? 2 : 1;
    return k;
}

// write/4 (lasp_core.erl:839-844) with S->mu held (laspj_var_etf_write's body; a waiter's
// threshold is written into its hidden variable the same way)
int var_write_locked(laspj_ctx* ctx, laspj::NifState* S, laspj_var* var, const uint8_t* value,
                     uint64_t n, int32_t* verdict) {
    laspj::KindState& K = *var->ns;
    if (!K.dict && laspj::reset_dict(ctx, S, K)) return LASPJ_E_NOMEM;
    // write/4 replaces the value: the old cells (or image) are not read — but a write that
    // fails with an error status (no memory, a device error) leaves the variable as it was
    const bool was_resident = var->resident, was_held = var->held;
    const uint64_t was_epoch = var->epoch;
    std::vector<uint8_t> was_image;
    was_image.swap(var->image);
    const bool had_cells = was_resident && was_epoch == K.epoch;
    var->resident = true;
    var->held = false;
    var->epoch = K.epoch;
    laspj::Call c = laspj::var_call(laspj::Op::WRITE, var, value, n);
    std::vector<int32_t> vd;
    const int s = laspj::run(ctx, S, c, &vd);
    auto drop_cells = [&] {
        std::lock_guard<std::mutex> lk2(ctx->mu);
        hipSetDevice(ctx->device);
        laspj::release_cells(ctx, var);
    };
    if (s) {
        // the write never answered (no memory, a device error): the old value stands
        if (!var->image.empty()) {
            // a reset inside the call wrote the old cells out: the image is the old value
            drop_cells();
            var->resident = false;
            var->held = false;
        } else if (had_cells) {
            var->epoch = was_epoch;   // the old cells (widened, perhaps): the old value
            var->held = was_held;
        } else {
            drop_cells();             // host-held before: cells the call sized are dropped
            var->resident = was_resident;
            var->epoch = was_epoch;
            var->held = was_held;
            var->image.swap(was_image);
        }
        return s;
    }
    *verdict = vd[0];
    if (vd[0] == LASPJ_NIF_OK) {
        var->image.clear();       // (a reset inside the call wrote the old cells out)
        return LASPJ_OK;
    }
    // not representable here: the variable holds the image on the host, and its calls
    // answer FALLBACK until a value the device takes is written
    const int held = laspj::nomem_guard(ctx, "var_write", [&] {
        var->image.assign(value, value + n);
        return LASPJ_OK;
    }, "host image");
    if (held) return held;
    var->resident = false;
    var->held = true;
    drop_cells();
    return LASPJ_OK;
}

}  // namespace laspj

using laspj::fail;
using laspj::kinds_of;
using laspj::var_state;

namespace {

int var_image_call(laspj_var* var, bool value, const uint8_t** out, uint64_t* out_len,
                   int32_t* verdict) {
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!out || !out_len || !verdict) return fail(ctx, LASPJ_E_INVAL, "var: null output");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return laspj::unknown_variable(ctx, "var");
    bool ok = false;
    if (int s = laspj::hydrate(ctx, S, var, &ok)) return s;
    if (!ok) {
        // host-held: read answers the image itself; value/1 is the reference's to compute
        *out = !value ? var->image.data() : nullptr;
        *out_len = !value ? var->image.size() : 0;
        *verdict = !value ? LASPJ_NIF_OK : LASPJ_NIF_FALLBACK;
        return LASPJ_OK;
    }
    laspj::Call c;
    // value/1 of a G-Set is its own term (ordsets:to_list, lasp_gset.erl:74-76)
    c.op = value && var->kind == LASPJ_KIND_ORSET ? laspj::Op::VVALUE : laspj::Op::READ;
    c.kind = var->kind;
    c.n = 1;
    c.m = 0;
    c.vars.push_back(var);
    laspj::one_group(c, var->ns.get());
    std::vector<int32_t> vd;
    if (int s = laspj::run(ctx, S, c, &vd)) return s;
    *verdict = vd[0];
    *out = vd[0] == LASPJ_NIF_OK ? c.obase + c.ooff[0] : nullptr;
    *out_len = vd[0] == LASPJ_NIF_OK ? c.ooff[1] - c.ooff[0] : 0;
    return LASPJ_OK;
}

// the tokens unique/1 mints (lasp_orset.erl:261-262: crypto:strong_rand_bytes(20)), from the
// kernel's CSPRNG
bool strong_rand(uint8_t* p, size_t n) {
    while (n) {
        const ssize_t r = getrandom(p, n, 0);
        if (r < 0) {
            if (errno == EINTR) continue;
            return false;
        }
        p += r;
        n -= (size_t)r;
    }
    return true;
}

// bind_many with S->mu held (laspj_var_etf_bind_many's body)
int bind_many_locked(laspj_ctx* ctx, laspj::NifState* S, uint32_t n, laspj_var* const* vars,
                     const uint8_t* const* values, const uint64_t* lens, int32_t* status,
                     int32_t* verdict, const uint8_t* const* pre = nullptr) {
    const int32_t kind = vars[0] ? vars[0]->kind : 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!vars[i] || vars[i]->ctx != ctx || !S->vars.count(vars[i]))
            return fail(ctx, LASPJ_E_INVAL, "var_bind: variable %u is not this context's", i);
        if (vars[i]->kind != kind)
            return fail(ctx, LASPJ_E_KIND, "var_bind: variables of one kind per call");
        if (!values[i] && lens[i]) return fail(ctx, LASPJ_E_INVAL, "var_bind: null payload");
    }
    {
        std::unordered_set<laspj_var*> seen;
        for (uint32_t i = 0; i < n; ++i)
            if (!seen.insert(vars[i]).second)
                return fail(ctx, LASPJ_E_INVAL, "var_bind: variable %u named twice", i);
    }
    // variables whose value sits in an image (after a dictionary reset) are decoded first;
    // one that stays host-held answers FALLBACK (the NIF binds its read image in Erlang)
    for (uint32_t i = 0; i < n; ++i) {
        bool ok = false;
        if (int s = laspj::hydrate(ctx, S, vars[i], &ok)) return s;
        verdict[i] = LASPJ_NIF_FALLBACK;
        status[i] = 0;
    }
    std::vector<uint32_t> live;
    for (uint32_t i = 0; i < n; ++i)
        if (vars[i]->resident && vars[i]->epoch == vars[i]->ns->epoch) live.push_back(i);
    if (live.empty()) return LASPJ_OK;
    // one decode per namespace (its own dictionary): the payloads grouped by namespace
    std::stable_sort(live.begin(), live.end(), [&](uint32_t x, uint32_t y) {
        return std::less<const laspj::KindState*>()(vars[x]->ns.get(), vars[y]->ns.get());
    });
    laspj::Call c;
    c.op = laspj::Op::BIND;
    c.kind = kind;
    c.n = c.m = (uint32_t)live.size();
    for (uint32_t k = 0; k < live.size(); ++k) {
        const uint32_t i = live[k];
        c.p.push_back(values[i]);
        c.len.push_back(lens[i]);
        c.pre.push_back(pre ? pre[i] : nullptr);
        c.vars.push_back(vars[i]);
        if (k == 0 || vars[live[k - 1]]->ns != vars[i]->ns)
            c.groups.push_back(laspj::Group{vars[i]->ns.get(), k, k + 1});
        else
            c.groups.back().p1 = k + 1;
    }
    std::vector<int32_t> vd;
    if (int s = laspj::run(ctx, S, c, &vd)) return s;
    for (size_t k = 0; k < live.size(); ++k) {
        verdict[live[k]] = vd[k];
        status[live[k]] = vd[k] == LASPJ_NIF_OK ? (int32_t)c.res[k] : 0;
        if (status[live[k]] == LASPJ_BIND_WRITTEN) lazy_clear(S, vars[live[k]]);
    }
    return LASPJ_OK;
}

// a LASPJ_KIND_GCOUNTER variable: the handle only carries its counter (laspj_counters.hip)
int counter_new(laspj_ctx* ctx, laspj::GcVar* peer, laspj_var** out) {
    auto* v = new (std::nothrow) laspj_var;
    if (!v) return fail(ctx, LASPJ_E_NOMEM, "var_create: host allocation");
    v->kind = LASPJ_KIND_GCOUNTER;
    v->resident = false;
    if (int s = laspj::gc_var_create(ctx, peer, &v->gc)) {
        delete v;
        return s;
    }
    *out = v;
    return LASPJ_OK;
}

}  // namespace

namespace laspj {
namespace {

// one batch of queued single binds (laspj_var_etf_bind's group commit), S->mu held: the
// requests of each kind that name distinct variables go into one bind_many; a request
// whose variable is not this context's answers LASPJ_E_INVAL on its own; a variable named
// again waits for the next round of the same batch (the caller marks them done)
void serve_binds(laspj_ctx* ctx, NifState* S, std::vector<BindReq*>& batch) {
    std::vector<BindReq*> todo;
    for (BindReq* r : batch) {
        if (r->var->ctx != ctx || !S->vars.count(r->var)) {
            r->rc = fail(ctx, LASPJ_E_INVAL, "var_bind: unknown variable");
        } else {
            todo.push_back(r);
        }
    }
    while (!todo.empty()) {
        std::vector<BindReq*> now, later;
        std::unordered_set<laspj_var*> seen;
        const int32_t kind = todo[0]->var->kind;
        for (BindReq* r : todo)
            (r->var->kind == kind && seen.insert(r->var).second ? now : later).push_back(r);
        const uint32_t k = (uint32_t)now.size();
        std::vector<laspj_var*> vs(k);
        std::vector<const uint8_t*> ps(k), pre(k);
        std::vector<uint64_t> ls(k);
        std::vector<int32_t> st(k, 0), vd(k, LASPJ_NIF_FALLBACK);
        for (uint32_t i = 0; i < k; ++i) {
            vs[i] = now[i]->var;
            ps[i] = now[i]->p;
            ls[i] = now[i]->n;
            // (a waiter still copying: the leader copies the payload itself)
            pre[i] = now[i]->staged.load(std::memory_order_acquire) ? now[i]->pre : nullptr;
        }
        const int rc = bind_many_locked(ctx, S, k, vs.data(), ps.data(), ls.data(), st.data(),
                                        vd.data(), pre.data());
        for (uint32_t i = 0; i < k; ++i) {
            now[i]->rc = rc;
            now[i]->status = rc ? 0 : st[i];
            now[i]->verdict = rc ? LASPJ_NIF_FALLBACK : vd[i];
        }
        todo.swap(later);
    }
}

}  // namespace
}  // namespace laspj

extern "C" {

int laspj_var_create(laspj_ctx* ctx, int32_t kind, laspj_var** out) {
    if (!ctx || !out) return LASPJ_E_INVAL;
    *out = nullptr;
    if (kind == LASPJ_KIND_GCOUNTER) return counter_new(ctx, nullptr, out);
    if (kind != LASPJ_KIND_ORSET && kind != LASPJ_KIND_GSET)
        return fail(ctx, LASPJ_E_KIND, "var_create: OR-Set, G-Set or G-Counter variables");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    return var_new(ctx, e.S, kind, nullptr, out);
}

int laspj_var_create_replica(laspj_var* peer, laspj_var** out) {
    if (peer && peer->gc) {
        if (!out || !laspj::gc_var_ctx(peer->gc)) return LASPJ_E_INVAL;
        *out = nullptr;
        return counter_new(laspj::gc_var_ctx(peer->gc), peer->gc, out);
    }
    laspj::NifState* S = var_state(peer);
    if (!S || !out) return LASPJ_E_INVAL;
    *out = nullptr;
    laspj_ctx* ctx = peer->ctx;
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(peer)) return laspj::unknown_variable(ctx, "var_create_replica");
    return var_new(ctx, S, peer->kind, peer->ns, out);
}

int laspj_var_destroy(laspj_var* v) {
    if (!v) return LASPJ_E_INVAL;
    if (v->gc) {
        laspj::gc_var_destroy(v->gc);
        delete v;
        return LASPJ_OK;
    }
    // its waiters and lazy threads go with it (a context gone first took their cells as it
    // took the variable's: only the host side is left)
    auto drop_waiters = [v](laspj::NifState* S) {
        for (laspj::Waiter& w : v->waiters) laspj::waiter_cells_drop(S, w.cells);
        for (laspj::Waiter& z : v->lazy) laspj::waiter_cells_drop(S, z.cells);
        v->waiters.clear();
        v->lazy.clear();
    };
    if (v->ctx) {
        laspj::NifState* S = laspj::state(v->ctx);
        if (S) {
            std::lock_guard<std::mutex> lk(S->mu);
            drop_waiters(S);
            S->vars.erase(v);
            v->ns->vars.erase(v);
            {
                std::lock_guard<std::mutex> lk2(v->ctx->mu);
                hipSetDevice(v->ctx->device);
                laspj::release_cells(v->ctx, v);
                // a filter naming it is dead from here on (its handle stays the caller's)
                for (laspj_filter* f : S->filters)
                    if (f->in == v || f->out == v) {
                        if (f->dev) laspj::dev_release(v->ctx, f->dev, f->dev_bytes);
                        f->dev = nullptr;
                        f->in = f->out = nullptr;
                        f->ns.reset();
                    }
                laspj::maps_var_gone(S, v);              // a map reading it, likewise
                laspj::folds_var_gone(S, v);
            }
            // the namespace's last variable: its device images go too
            if (v->ns.use_count() == 1) laspj::free_ns(*v->ns);
        }
    } else {
        drop_waiters(nullptr);
        if (v->ns && v->ns.use_count() == 1 && v->ns->dict) {
            laspj_dict_destroy(v->ns->dict);     // (its device images went with the context)
            v->ns->dict = nullptr;
        }
    }
    delete v;
    return LASPJ_OK;
}

int laspj_var_etf_bind_many(laspj_ctx* ctx, uint32_t n, laspj_var* const* vars,
                            const uint8_t* const* values, const uint64_t* lens, int32_t* status,
                            int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!n) return LASPJ_OK;
    if (!vars || !values || !lens || !status || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_bind: null array");
    if (const int k = kinds_of(n, vars); k & 2) {
        // counters: their own pass (laspj_counters.hip); never mixed with sets
        if (k & 1) return fail(ctx, LASPJ_E_KIND, "var_bind: variables of one kind per call");
        std::vector<laspj::GcVar*> gs(n, nullptr);
        for (uint32_t i = 0; i < n; ++i) gs[i] = vars[i] ? vars[i]->gc : nullptr;
        return laspj::gc_bind_many(ctx, n, gs.data(), values, lens, status, verdict);
    }
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    return bind_many_locked(ctx, e.S, n, vars, values, lens, status, verdict);
}

int laspj_var_etf_bind(laspj_var* var, const uint8_t* value, uint64_t n, int32_t* status,
                       int32_t* verdict) {
    if (var && var->gc) {
        // a counter bind takes the call lock directly (no group-commit queue)
        laspj_ctx* gctx = laspj::gc_var_ctx(var->gc);
        if (!gctx) return LASPJ_E_INVAL;
        if ((!value && n) || !status || !verdict)
            return fail(gctx, LASPJ_E_INVAL, "var_bind: null argument");
        return laspj::gc_bind_many(gctx, 1, &var->gc, &value, &n, status, verdict);
    }
    if (!var || !var->ctx) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!value && n) || !status || !verdict) return fail(ctx, LASPJ_E_INVAL, "var_bind: null argument");
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    // Group commit: schedulers binding through one context at once are served by one device
    // pass.  The caller that finds no pass running leads: it takes every queued bind (its
    // own first) and runs them as one bind_many, again while more arrive; the others wait
    // for their answers.  One context per GPU then batches many schedulers' binds
    // (lasp_vnode.erl:213-237) instead of one stream and pass per scheduler.
    laspj::BindReq r;
    r.var = var;
    r.p = value;
    r.n = n;
    laspj::PinSlot slot;
    bool want_slot = false;
    {
        std::lock_guard<std::mutex> q(S->qmu);
        if (S->leading) {
            S->queue.push_back(&r);
            // a waiter stages its own payload into a pinned block while the pass before
            // it runs (the leader then only gathers it on the device)
            if (n >= laspj::kPinMin) {
                if (!S->pins.empty()) {
                    slot = S->pins.back();
                    S->pins.pop_back();
                    want_slot = true;
                } else if (S->pins_live < laspj::kPinSlots) {
                    ++S->pins_live;
                    want_slot = true;
                }
            }
        } else {
            S->leading = true;
            r.lead = true;
        }
    }
    if (want_slot) {
        if (slot.cap < n + 16 && !laspj::pin_grow(&slot, n + 16)) {
            std::lock_guard<std::mutex> q(S->qmu);
            --S->pins_live;
            want_slot = false;
        }
        if (want_slot) {
            std::memcpy(slot.h, value, n);
            r.pre = slot.d;
            r.staged.store(true, std::memory_order_release);
        }
    }
    // (the block back to the pool once the pass that read it has answered)
    auto give_back = [&]() {
        if (!want_slot) return;
        std::lock_guard<std::mutex> q(S->qmu);
        S->pins.push_back(slot);
    };
    if (!r.lead) {
        std::unique_lock<std::mutex> lk(r.m);
        r.cv.wait(lk, [&] { return r.done || r.lead; });
        if (r.done) {
            lk.unlock();
            give_back();
            *status = r.status;
            *verdict = r.verdict;
            return r.rc;
        }
    }
    // the leader: its own request and every queued one per pass, again while binds keep
    // arriving (up to kLeadRounds), then it hands the leadership to the oldest waiter
    std::vector<laspj::BindReq*> batch;
    bool own = true;
    for (int round = 0; round < laspj::kLeadRounds; ++round) {
        batch.clear();
        {
            std::lock_guard<std::mutex> q(S->qmu);
            batch.swap(S->queue);
        }
        if (own) batch.insert(batch.begin(), &r);
        own = false;
        if (batch.empty()) break;
        {
            std::lock_guard<std::mutex> lk(S->mu);
            laspj::serve_binds(ctx, S, batch);
        }
        // (each answer published under its request's own lock; the waiter may return and
        // drop the request as soon as that lock is released)
        for (laspj::BindReq* b : batch) {
            if (b == &r) continue;
            std::lock_guard<std::mutex> lk(b->m);
            b->done = true;
            b->cv.notify_one();
        }
    }
    {
        std::lock_guard<std::mutex> q(S->qmu);
        if (S->queue.empty()) {
            S->leading = false;
        } else {
            laspj::BindReq* nx = S->queue.front();
            S->queue.erase(S->queue.begin());
            std::lock_guard<std::mutex> lk(nx->m);
            nx->lead = true;
            nx->cv.notify_one();
        }
    }
    give_back();
    *status = r.status;
    *verdict = r.verdict;
    return r.rc;
}

int laspj_var_etf_write(laspj_var* var, const uint8_t* value, uint64_t n, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_write(var->gc, value, n, verdict);
    const laspj::Entry e = laspj::enter_var(var, "var_write", (value || !n) && verdict);
    if (e.rc) return e.rc;
    const int s = var_write_locked(e.ctx, e.S, var, value, n, verdict);
    if (s == LASPJ_OK) lazy_clear(e.S, var);
    return s;
}

int laspj_var_etf_read(laspj_var* var, const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_read(var->gc, false, out, out_len, verdict);
    return var_image_call(var, false, out, out_len, verdict);
}

int laspj_var_etf_value(laspj_var* var, const uint8_t** out, uint64_t* out_len,
                        int32_t* verdict) {
    if (var && var->gc) return laspj::gc_read(var->gc, true, out, out_len, verdict);
    return var_image_call(var, true, out, out_len, verdict);
}

int laspj_var_etf_threshold(laspj_var* var, const uint8_t* threshold, uint64_t n, int strict,
                            int32_t* result, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_threshold(var->gc, threshold, n, strict, result, verdict);
    const laspj::Entry e =
        laspj::enter_var(var, "var_threshold", (threshold || !n) && result && verdict);
    if (e.rc) return e.rc;
    bool ok = false;
    if (int s = laspj::hydrate(e.ctx, e.S, var, &ok)) return s;
    *result = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    if (!ok) return LASPJ_OK;
    laspj::Call c = laspj::var_call(laspj::Op::THRESHOLD, var, threshold, n, strict ? 1 : 0);
    std::vector<int32_t> vd;
    if (int s = laspj::run(e.ctx, e.S, c, &vd)) return s;
    *verdict = vd[0];
    *result = vd[0] == LASPJ_NIF_OK ? (int32_t)(c.res[0] != 0) : 0;
    return LASPJ_OK;
}

int laspj_var_union(laspj_var* out, laspj_var* l, laspj_var* r, int32_t* status,
                    int32_t* verdict) {
    if (out && out->gc) {
        // riak_dt_gcounter is no type lasp_core:union/7 takes: the NIF runs the reference's
        if (!l || !r || !status) return LASPJ_E_INVAL;
        *status = LASPJ_BIND_NOOP;
        return laspj::gc_refuse(out->gc, verdict);
    }
    laspj::NifState* S = var_state(out);
    if (!S || !l || !r) return LASPJ_E_INVAL;
    laspj_ctx* ctx = out->ctx;
    if (!status || !verdict) return fail(ctx, LASPJ_E_INVAL, "var_union: null argument");
    if (l->ctx != ctx || r->ctx != ctx)
        return fail(ctx, LASPJ_E_INVAL, "var_union: variables of different contexts");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(out) || !S->vars.count(l) || !S->vars.count(r))
        return laspj::unknown_variable(ctx, "var_union");
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    // OR-Sets of one namespace only: a G-Set's body is `LValue ++ RValue` (a list value),
    // and cells of two namespaces name different terms by one slot
    if (out->kind != LASPJ_KIND_ORSET || l->kind != LASPJ_KIND_ORSET ||
        r->kind != LASPJ_KIND_ORSET || l->ns != out->ns || r->ns != out->ns)
        return laspj::fallback(S);
    for (laspj_var* v : {out, l, r}) {
        bool ok = false;
        if (int s = laspj::hydrate(ctx, S, v, &ok)) return s;
        if (!ok) return laspj::fallback(S);
    }
    laspj::KindState& K = *out->ns;
    *verdict = LASPJ_NIF_OK;
    if (!K.dict || K.E == 0) return LASPJ_OK;             // three new() values
    laspj::Guard g(ctx);
    const uint32_t tw = laspj::ktw(K);
    for (laspj_var* v : {out, l, r})
        if (int s = laspj::fit_var(ctx, v, K.E, tw)) return s;
    void* word = nullptr;
    if (laspj::dev_alloc(ctx, 256, &word) != hipSuccess) {
        hipGetLastError();
        return fail(ctx, LASPJ_E_NOMEM, "var_union: flag word");
    }
    uint32_t changed = 0;                                 // (Value0 =/= AccValue)
    hipError_t e = hipMemsetAsync(word, 0, 4, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(laspj::k_var_union, dim3((K.E + 255) / 256), dim3(256), 0,
                           ctx->stream, out->cells, l->cells, r->cells, K.E, tw,
                           static_cast<uint32_t*>(word));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = laspj::readback(ctx, &changed, word, 4);
    laspj::dev_release(ctx, word, 256);
    if (e != hipSuccess) return fail(ctx, LASPJ_E_DEVICE, "var_union: %s", hipGetErrorString(e));
    *status = changed ? LASPJ_BIND_WRITTEN : LASPJ_BIND_NOOP;
    if (changed) lazy_clear(S, out, true);
    return LASPJ_OK;
}

int laspj_var_resident(const laspj_var* var, int32_t* resident) {
    if (var && var->gc) return laspj::gc_resident(var->gc, resident);
    if (!var || !resident) return LASPJ_E_INVAL;
    *resident = var->ctx && var->resident ? 1 : 0;
    return LASPJ_OK;
}

int laspj_var_etf_update(laspj_var* var, const uint8_t* op, uint64_t nop, int32_t* result,
                         const uint8_t** err_elem, uint64_t* err_len, const uint8_t** minted,
                         uint32_t* nminted, int32_t* verdict) {
    if (var && var->gc) {
        // riak_dt_gcounter:update/3 needs the Actor: laspj_var_etf_increment
        if (!op || !nop || !result) return LASPJ_E_INVAL;
        *result = LASPJ_UPDATE_OK;
        if (err_elem) *err_elem = nullptr;
        if (err_len) *err_len = 0;
        if (minted) *minted = nullptr;
        if (nminted) *nminted = 0;
        return laspj::gc_refuse(var->gc, verdict);
    }
    const laspj::Entry en = laspj::enter_var(var, "var_update", op && nop && result && verdict);
    if (en.rc) return en.rc;
    laspj::NifState* S = en.S;
    laspj_ctx* ctx = en.ctx;
    ++S->stats[laspj::ST_CALLS];
    *result = LASPJ_UPDATE_OK;
    *verdict = LASPJ_NIF_FALLBACK;
    if (err_elem) *err_elem = nullptr;
    if (err_len) *err_len = 0;
    if (minted) *minted = nullptr;
    if (nminted) *nminted = 0;
    bool ok = false;
    if (int s = laspj::hydrate(ctx, S, var, &ok)) return s;
    if (!ok) return laspj::fallback(S);
    // Type:update(Op, Actor, Value0) (lasp_core.erl:283-287): the op's terms
    std::vector<laspj::UpdateOp> ops;
    const int ps = laspj::parse_update_op(var->kind, op, nop, &ops);
    if (ps == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "var_update: host allocation");
    if (ps != LASPJ_DEC_OK || ops.size() > (1u << 24)) return laspj::fallback(S);
    if (ops.empty()) {
        // {add_all, []}, {remove_all, []}, {update, []}: {ok, Value0}
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    }
    const bool orset = var->kind == LASPJ_KIND_ORSET;
    laspj::KindState& K = *var->ns;
    if (!K.dict && laspj::reset_dict(ctx, S, K)) return LASPJ_E_NOMEM;
    uint32_t nmint = 0;
    for (const auto& o : ops) nmint += o.mint ? 1u : 0u;
    S->minted.resize(20ull * nmint);
    if (nmint && !strong_rand(S->minted.data(), S->minted.size()))
        return fail(ctx, LASPJ_E_DEVICE, "var_update: getrandom failed (%d)", errno);
    // the terms registered in the variable's namespace (element slots, token slots); the
    // whole call's registrations undone when one is refused
    const uint64_t t0 = laspj::now_ns();
    const uint32_t nd0 = laspj::dict_elements(K.dict);
    std::vector<laspj_op> dops(ops.size());
    bool any_remove = false, registered = false;
    uint8_t timg[25] = {109, 0, 0, 0, 20};       // BINARY_EXT of 20 bytes
    laspj::dict_begin(K.dict);
    uint32_t mi = 0;
    for (size_t k = 0; k < ops.size(); ++k) {
        if (k == 0) {
            any_remove = registered = false;
            mi = 0;
        }
        const laspj::UpdateOp& o = ops[k];
        laspj_op& d = dops[k];
        d = laspj_op{};
        d.kind = o.kind;
        d.flags = k == 0 ? LASPJ_OP_FLAG_NEW_CALL : 0;
        const auto* eimg = reinterpret_cast<const uint8_t*>(o.elem.data());
        if (o.kind == LASPJ_OP_REMOVE) {
            // orddict:find/2 (lasp_orset.erl:233): absent unless the namespace holds it
            const int64_t e = laspj::dict_find_elem(K.dict, eimg, o.elem.size());
            if (e == -2) {
                laspj::dict_rollback(K.dict);
                return laspj::fallback(S);            // an `==`-equal key under another image
            }
            d.element = e < 0 ? laspj::kNoElem : (uint32_t)e;
            any_remove = true;
            continue;
        }
        uint32_t e = 0, t = 0;
        int st = laspj::dict_reg_elem(K.dict, eimg, o.elem.size(), &e);
        if (st == LASPJ_DEC_OK && orset) {
            const uint8_t* tp;
            size_t tl;
            if (o.mint) {
                std::memcpy(timg + 5, S->minted.data() + 20ull * mi++, 20);
                tp = timg;
                tl = sizeof(timg);
            } else {
                tp = reinterpret_cast<const uint8_t*>(o.tok.data());
                tl = o.tok.size();
            }
            const uint32_t had = laspj::dict_token_count(K.dict, e);
            st = laspj::dict_reg_tok(K.dict, e, tp, tl, &t);
            registered |= laspj::dict_token_count(K.dict, e) != had;
        }
        if (st == LASPJ_E_NOMEM) {
            laspj::dict_rollback(K.dict);
            return fail(ctx, LASPJ_E_NOMEM, "var_update: registration");
        }
        if (st == LASPJ_DEC_UNREPRESENTABLE && !K.wide) {
            // a 65th token on an element: the namespace goes wide and the call's
            // registrations start over
            laspj::dict_rollback(K.dict);
            if (laspj::go_wide(S, K)) {
                laspj::dict_begin(K.dict);
                k = (size_t)-1;
                continue;
            }
            return laspj::fallback(S);
        }
        if (st != LASPJ_DEC_OK) {
            // an `==`-equal term under another image, a token image a wide namespace cannot
            // hold: the reference's clause on the NIF side
            laspj::dict_rollback(K.dict);
            return laspj::fallback(S);
        }
        d.element = e;
        d.slot = (uint8_t)t;
        d.pad = (uint8_t)(t >> 8);
    }
    laspj::dict_begin(K.dict);                    // (the journal kept nothing)
    registered |= laspj::dict_elements(K.dict) != nd0;
    if (registered) {
        ++S->stats[laspj::ST_REGISTRATIONS];
        K.stale = true;
    }
    S->stats[laspj::ST_NS_REGISTER] += laspj::now_ns() - t0;
    // the device images learn the new terms before the namespace's next device pass: a
    // token on a known element is patched in by that pass (run() patches a stale namespace
    // first — consecutive updates batch their patches); new elements or a new width need
    // the images now (the cells' element slots and pairs come from them)
    const bool lazy = orset && K.etf && laspj::dict_elements(K.dict) == K.built_K &&
                      (!K.wide || laspj::dict_max_tokens(K.dict) <= 64u * K.tw);
    if ((K.stale || !K.etf) && !lazy)
        if (!laspj::patch_etf(ctx, S, K))
            if (int s = laspj::rebuild_etf(ctx, S, K)) return s;
    const uint32_t nops = (uint32_t)dops.size();
    bool all_add = !any_remove;
    int32_t* dstat = nullptr;
    {
        laspj::Guard g(ctx);
        const uint32_t tw = laspj::ktw(K);
        if (int s = laspj::fit_var(ctx, var, K.E, tw)) return s;
        laspj::UpdArgs args;
        std::memset(&args, 0, sizeof(args));
        const laspj_op* dev_ops = nullptr;
        void* blk = nullptr;
        const uint64_t stat_bytes = any_remove ? 4ull * nops : 0;
        const uint64_t ops_bytes = nops > laspj::kUpdArgOps ? 16ull * nops : 0;
        if (stat_bytes + ops_bytes) {
            if (laspj::dev_alloc(ctx, ((stat_bytes + 255) & ~255ull) + ops_bytes, &blk) != hipSuccess) {
                hipGetLastError();
                return fail(ctx, LASPJ_E_NOMEM, "var_update: op buffer");
            }
            dstat = static_cast<int32_t*>(blk);
            if (ops_bytes) {
                auto* p = reinterpret_cast<laspj_op*>(static_cast<uint8_t*>(blk) +
                                                      ((stat_bytes + 255) & ~255ull));
                LJ_HIP(ctx, hipMemcpyAsync(p, dops.data(), ops_bytes, hipMemcpyHostToDevice,
                                           ctx->stream));
                dev_ops = p;
            }
        }
        if (!dev_ops) std::memcpy(args.op, dops.data(), 16ull * nops);
        if (all_add && dev_ops) {
            hipLaunchKernelGGL(laspj::k_var_adds, dim3((nops + 255) / 256), dim3(256), 0,
                               ctx->stream, var->cells, var->kind, tw, dev_ops, nops);
        } else {
            hipLaunchKernelGGL(laspj::k_var_update, dim3(1), dim3(64), 0, ctx->stream, var->cells,
                               var->kind, tw, args, dev_ops, nops, any_remove ? dstat : nullptr);
        }
        LJ_LAUNCHED(ctx);
        std::vector<int32_t> st;
        if (any_remove) {
            // a precondition may fail: its statuses back (one synchronisation)
            st.resize(nops);
            LJ_HIP(ctx, laspj::readback(ctx, st.data(), dstat, 4ull * nops));
        }
        if (blk) laspj::dev_release(ctx, blk, ((stat_bytes + 255) & ~255ull) + ops_bytes);
        for (uint32_t k = 0; k < st.size(); ++k)
            if (st[k] == LASPJ_OPST_NOT_PRESENT) {
                // {error, {precondition, {not_present, Elem}}} (lasp_orset.erl:239-240)
                *result = LASPJ_UPDATE_NOT_PRESENT;
                S->err_elem = ops[k].elem;
                if (err_elem) *err_elem = reinterpret_cast<const uint8_t*>(S->err_elem.data());
                if (err_len) *err_len = S->err_elem.size();
                break;
            }
    }
    if (minted) *minted = S->minted.empty() ? nullptr : S->minted.data();
    if (nminted) *nminted = nmint;
    *verdict = LASPJ_NIF_OK;
    if (*result == LASPJ_UPDATE_OK) lazy_clear(S, var);
    return LASPJ_OK;
}

int laspj_var_etf_increment(laspj_var* var, const uint8_t* op, uint64_t nop, const uint8_t* actor,
                            uint64_t nactor, uint64_t* ids, uint32_t cap, uint32_t* nmet,
                            uint32_t* nwaiting, int32_t* verdict) {
    if (!var) return LASPJ_E_INVAL;
    if (!var->gc) {
        // lasp_orset / lasp_gset have no increment: laspj_var_etf_update serves their update/3
        if (!var->ctx) return LASPJ_E_INVAL;
        return fail(var->ctx, LASPJ_E_KIND, "var_increment: a G-Counter variable");
    }
    return laspj::gc_increment(var->gc, op, nop, actor, nactor, ids, cap, nmet, nwaiting, verdict);
}

}  // extern "C"
