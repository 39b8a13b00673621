// riak_dt_gcounter variables resident on the device: the `#dv.value` of the advertisement
// counter (riak_test/lasp_adcounter_test.erl; include/lasp.hrl:60-63, 76) beside the set
// variables of laspj_nif_vars.hip and laspj_nif_waiters.hip, whose entry points branch here for LASPJ_KIND_GCOUNTER.
//
// A variable is one row of uint64 counts over the actor slots of its namespace (a host
// dictionary of element terms, shared by the replicas made with laspj_var_create_replica).
// The host walks every incoming image (laspj_counter_host.cpp) and stages {slot, count}
// pairs in pinned memory; one kernel per call gathers them, decides `Value0 =:= Value`,
// writes the per-actor max, sums the row and compares the sum with the planned thresholds
// of the variable's waiters, and writes {status, sum, met-mask words} into pinned memory:
// one launch and one synchronisation per call.
//
// Widths (tests/test_gpu_counters.py derives its shapes from them): one wave of 64 lanes
// per variable; the row is summed S = 128 slots per iteration (16 bytes per lane); pairs are
// gathered 64 per iteration; V = 4 variables per 256-thread block; W = 64 waiters per ballot
// step (one mask word).  k_gc_incr serves one variable with a whole block: 512 slots per
// iteration, four ballot steps side by side.
//
// Locking as the set path's: the context's call lock (NifState::mu) for the whole call,
// ctx->mu for the device phase.  Every call that stages operands synchronises before it
// returns, so the staging is free again; the one call that does not wait (an increment
// without a re-check) takes its operands as kernel arguments.

#include <algorithm>
#include <cstring>
#include <memory>
#include <new>
#include <unordered_set>
#include <vector>

#include "laspj_internal.h"

namespace laspj {

struct GcNs {
    laspj_dict* dict = nullptr;          // actor terms -> slots (element terms only)
    std::vector<uint32_t> order;         // the slots read so far, in term order
    ~GcNs() {
        if (dict) laspj_dict_destroy(dict);
    }
};

// one entry of `#dv.waiting_threads`: its image as registered and its plan
struct GcWaiter {
    uint64_t id = 0;
    int32_t strict = 0;
    std::vector<uint8_t> image;
    int32_t plan = LASPJ_GC_NEVER;       // LASPJ_GC_NEVER: kept in list order, never fires
    uint64_t t = 0;                      // LASPJ_GC_T: met when t =< value
    bool met = false;                    // the last check's answer (valid while `checked`)
};

struct GcVar {
    laspj_ctx* ctx = nullptr;            // null once the context is gone
    std::shared_ptr<GcNs> ns;
    uint64_t* row = nullptr;             // cap counts (null: new())
    uint32_t cap = 0;                    // a power of two >= kGcRow0
    bool resident = true;                // the row holds the value (else `image` does)
    bool held = false;                   // `image` is a value write/4 could not represent
    std::vector<uint8_t> image;
    std::vector<GcWaiter> waiters;       // in list order
    bool checked = true;                 // every waiter's `met` is of the current value
    uint64_t bound = 0;                  // no count of the row is above this
};

struct GcState {
    std::unordered_set<GcVar*> vars;
    // pinned, coherent staging: kernels read the operands from one and write the answers
    // into the other
    void* hin = nullptr;
    uint64_t hin_bytes = 0;
    uint8_t* hin_d = nullptr;
    void* hout = nullptr;
    uint64_t hout_bytes = 0;
    uint8_t* hout_d = nullptr;
    std::string answer;                  // read / value: valid until the context's next call
};

namespace {

constexpr uint32_t kGcRow0 = 64;         // a row's first capacity
constexpr int ST_CALLS = 0, ST_PASSES = 1, ST_REGISTRATIONS = 2, ST_FALLBACKS = 6;

// what a kernel reads per variable (32 bytes, in the pinned in-region)
struct GcDesc {
    uint64_t* row;
    uint32_t cap, npairs, pair_off, nthr, thr_off, out_off;
};
static_assert(sizeof(GcDesc) == 32 && sizeof(GcPair) == 16, "staging layout");
typedef unsigned long long gc2 __attribute__((ext_vector_type(2)));

__device__ inline uint64_t wave_sum(uint64_t x) {
    for (int o = 32; o; o >>= 1) x += __shfl_xor((unsigned long long)x, o, 64);
    return x;
}
__device__ inline uint32_t wave_sum32(uint32_t x) {
    for (int o = 32; o; o >>= 1) x += __shfl_xor(x, o, 64);
    return x;
}

// a wave's share of a row's sum and non-zero count: 128 slots per iteration
__device__ inline void row_scan(const uint64_t* row, uint32_t cap, uint32_t lane, uint32_t stride,
                                uint64_t* sum, uint32_t* nnz) {
    const gc2* r2 = reinterpret_cast<const gc2*>(row);
    for (uint32_t i = lane; i < cap / 2; i += stride) {
        const gc2 x = r2[i];
        *sum += x.x + x.y;
        *nnz += (x.x != 0) + (x.y != 0);
    }
}

// the sum against a variable's planned thresholds, 64 per ballot: one mask word each
__device__ inline void wave_thresholds(uint64_t sum, const uint64_t* thr, uint32_t nthr,
                                       uint32_t first, uint32_t step, uint32_t lane,
                                       uint64_t* masks) {
    for (uint32_t w0 = first; w0 < nthr; w0 += step) {
        const uint32_t w = w0 + lane;
        const bool met = w < nthr && thr[w] <= sum;
        const uint64_t m = __ballot(met);
        if (lane == 0) masks[w0 / 64] = m;
    }
}

// lasp_core:bind/3 (lasp_core.erl:291-312) of n counters, a wave each: `Value0 =:= Value`
// (the pair count against the row's non-zero count, each count against its slot), the
// per-actor max written, the new sum, the waiters' thresholds.
__global__ void __launch_bounds__(256) k_gc_bind(const GcDesc* __restrict__ descs,
                                                 const GcPair* __restrict__ pairs,
                                                 const uint64_t* __restrict__ thr,
                                                 uint64_t* __restrict__ out, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;
    const GcDesc d = descs[v];
    uint64_t sum = 0, delta = 0;
    uint32_t nnz = 0, neq = 0;
    row_scan(d.row, d.cap, lane, 64, &sum, &nnz);          // Value0, before the max lands
    const gc2* pp = reinterpret_cast<const gc2*>(pairs + d.pair_off);
    for (uint32_t i = lane; i < d.npairs; i += 64) {
        const gc2 p = pp[i];                               // {count, slot}
        const uint32_t slot = (uint32_t)p.y;
        if (slot >= d.cap) {                               // (the host grew the row: never)
            neq = 1;
            continue;
        }
        const uint64_t old = d.row[slot];
        neq |= old != p.x;
        if (p.x > old) {
            d.row[slot] = p.x;                             // slots of one image are distinct
            delta += p.x - old;
        }
    }
    sum = wave_sum(sum) + wave_sum(delta);
    nnz = wave_sum32(nnz);
    neq = wave_sum32(neq);
    uint64_t* o = out + d.out_off;
    wave_thresholds(sum, thr + d.thr_off, d.nthr, 0, 64, lane, o + 2);
    if (lane == 0) {
        o[0] = (neq == 0 && nnz == d.npairs) ? LASPJ_BIND_NOOP : LASPJ_BIND_WRITTEN;
        o[1] = sum;
    }
}

// the sum and the waiter check of n counters (recheck, recheck_many, threshold, wait, value)
__global__ void __launch_bounds__(256) k_gc_check(const GcDesc* __restrict__ descs,
                                                  const uint64_t* __restrict__ thr,
                                                  uint64_t* __restrict__ out, uint32_t n) {
    const uint32_t lane = threadIdx.x & 63, v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= n) return;
    const GcDesc d = descs[v];
    uint64_t sum = 0;
    uint32_t nnz = 0;
    row_scan(d.row, d.cap, lane, 64, &sum, &nnz);
    sum = wave_sum(sum);
    uint64_t* o = out + d.out_off;
    wave_thresholds(sum, thr + d.thr_off, d.nthr, 0, 64, lane, o + 2);
    if (lane == 0) {
        o[0] = 0;
        o[1] = sum;
    }
}

// riak_dt_gcounter:update({increment, N}, Actor, V) on one counter and its waiters against
// the new sum; out (or null: nobody reads the answer): {0 | 1 the count would pass 2^64 - 1
// (nothing written), sum, mask words}
__global__ void __launch_bounds__(256) k_gc_incr(uint64_t* __restrict__ row, uint32_t cap,
                                                 uint32_t slot, uint64_t N,
                                                 const uint64_t* __restrict__ thr, uint32_t nthr,
                                                 uint64_t* __restrict__ out) {
    __shared__ uint64_t part[4];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const bool in = slot < cap;                            // (the host grew the row: always)
    const uint64_t old = in ? row[slot] : 0;
    const bool ok = in && old + N >= old;
    uint64_t sum = 0;
    uint32_t nnz = 0;
    row_scan(row, cap, threadIdx.x, 256, &sum, &nnz);
    sum = wave_sum(sum);
    if (lane == 0) part[wave] = sum;
    __syncthreads();                                       // every read of the old row is done
    sum = part[0] + part[1] + part[2] + part[3] + (ok ? N : 0);
    if (threadIdx.x == 0 && ok) row[slot] = old + N;
    if (!out) return;
    wave_thresholds(sum, thr, nthr, wave * 64, 256, lane, out + 2);
    if (threadIdx.x == 0) {
        out[0] = ok ? 0 : 1;
        out[1] = sum;
    }
}

// a row at its new capacity: the old counts, zero behind them (src null: new())
__global__ void __launch_bounds__(256) k_gc_grow(uint64_t* __restrict__ dst,
                                                 const uint64_t* __restrict__ src,
                                                 uint32_t old_cap, uint32_t new_cap) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < new_cap; i += gridDim.x * 256)
        dst[i] = i < old_cap ? src[i] : 0;
}

// write/4: an image's pairs into a zeroed row
__global__ void __launch_bounds__(256) k_gc_scatter(uint64_t* __restrict__ row, uint32_t cap,
                                                    const GcPair* __restrict__ pairs, uint32_t n) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
        const GcPair p = pairs[i];
        if (p.slot < cap) row[p.slot] = p.count;
    }
}

struct DevGuard {
    std::lock_guard<std::mutex> lk;
    explicit DevGuard(laspj_ctx* c) : lk(c->mu) { hipSetDevice(c->device); }
};

// the context's counter state (call lock held)
GcState* gstate(const GcHooks& h) {
    if (!*h.slot) *h.slot = new (std::nothrow) GcState;
    return *h.slot;
}

int grow_pinned(laspj_ctx* ctx, void** p, uint64_t* have, uint8_t** dev, uint64_t need) {
    if (*have >= need) return LASPJ_OK;
    const uint64_t want = std::max<uint64_t>(std::max<uint64_t>(need, 2 * *have), 64ull << 10);
    if (*p) {
        hipStreamSynchronize(ctx->stream);
        hipHostFree(*p);
        *p = nullptr;
        *have = 0;
    }
    void* d = nullptr;
    if (hipHostMalloc(p, want, hipHostMallocCoherent) != hipSuccess ||
        hipHostGetDevicePointer(&d, *p, 0) != hipSuccess) {
        hipGetLastError();
        if (*p) hipHostFree(*p);
        *p = nullptr;
        return fail(ctx, LASPJ_E_NOMEM, "counters: pinned allocation of %llu bytes",
                    (unsigned long long)want);
    }
    *dev = static_cast<uint8_t*>(d);
    *have = want;
    return LASPJ_OK;
}

void release_row(laspj_ctx* ctx, GcVar* v) {
    if (v->row) dev_release(ctx, v->row, 8ull * v->cap);
    v->row = nullptr;
    v->cap = 0;
}

// the row holds `slots` slots at least: capacity doubles, the counts are copied on the
// device and the old block released in stream order (ctx->mu held)
int fit_row(laspj_ctx* ctx, GcVar* v, uint32_t slots) {
    uint32_t cap = v->cap ? v->cap : kGcRow0;
    while (cap < slots) cap *= 2;
    if (v->row && cap == v->cap) return LASPJ_OK;
    void* p = nullptr;
    if (dev_alloc(ctx, 8ull * cap, &p) != hipSuccess) {
        hipGetLastError();
        return fail(ctx, LASPJ_E_NOMEM, "counters: a row of %u slots", cap);
    }
    hipLaunchKernelGGL(k_gc_grow, dim3(std::min<uint32_t>((cap + 255) / 256, 1024)), dim3(256), 0,
                       ctx->stream, static_cast<uint64_t*>(p), v->row, v->cap, cap);
    LJ_LAUNCHED(ctx);
    release_row(ctx, v);
    v->row = static_cast<uint64_t*>(p);
    v->cap = cap;
    return LASPJ_OK;
}

bool ensure_dict(GcNs* ns) {
    return ns->dict || laspj_dict_create(&ns->dict) == LASPJ_OK;
}

// one variable of a device pass and its answer
struct Item {
    GcVar* v = nullptr;
    std::vector<GcPair> pairs;           // (bind) the image's
    bool extra = false;                  // a threshold checked beside the waiters'
    uint64_t extra_t = 0;
    uint32_t status = 0;
    uint64_t sum = 0;
    bool extra_met = false;
};

// the waiters a kernel checks (plan T), in list order
uint32_t checkable(const GcVar* v) {
    uint32_t k = 0;
    for (const GcWaiter& w : v->waiters) k += w.plan == LASPJ_GC_T ? 1 : 0;
    return k;
}

enum class Pass { BIND, CHECK };

// One launch and one synchronisation over the items: rows grown, descriptors, pairs and
// thresholds staged, the kernel, the answers read; every item's waiters get their `met`.
int run_pass(laspj_ctx* ctx, GcState* G, const GcHooks& h, Pass kind, std::vector<Item>& items) {
    const uint32_t n = (uint32_t)items.size();
    uint64_t npairs = 0, nthr = 0, nout = 0;
    for (const Item& it : items) {
        npairs += it.pairs.size();
        const uint32_t k = checkable(it.v) + (it.extra ? 1 : 0);
        nthr += k;
        nout += 2 + (k + 63) / 64;
    }
    const uint64_t pair_at = 32ull * n, thr_at = pair_at + 16ull * npairs;
    DevGuard g(ctx);
    if (int s = grow_pinned(ctx, &G->hin, &G->hin_bytes, &G->hin_d, thr_at + 8ull * nthr + 16)) return s;
    if (int s = grow_pinned(ctx, &G->hout, &G->hout_bytes, &G->hout_d, 8ull * nout)) return s;
    uint8_t* in = static_cast<uint8_t*>(G->hin);
    GcDesc* descs = reinterpret_cast<GcDesc*>(in);
    GcPair* pairs = reinterpret_cast<GcPair*>(in + pair_at);
    uint64_t* thr = reinterpret_cast<uint64_t*>(in + thr_at);
    uint32_t pa = 0, ta = 0, oa = 0;
    for (uint32_t i = 0; i < n; ++i) {
        Item& it = items[i];
        uint32_t need = 1;
        for (const GcPair& p : it.pairs) need = std::max(need, p.slot + 1);
        if (int s = fit_row(ctx, it.v, need)) return s;
        GcDesc& d = descs[i];
        d.row = it.v->row;
        d.cap = it.v->cap;
        d.npairs = (uint32_t)it.pairs.size();
        d.pair_off = pa;
        d.thr_off = ta;
        d.out_off = oa;
        if (d.npairs) std::memcpy(pairs + pa, it.pairs.data(), 16ull * d.npairs);
        pa += d.npairs;
        uint32_t k = 0;
        for (const GcWaiter& w : it.v->waiters)
            if (w.plan == LASPJ_GC_T) thr[ta + k++] = w.t;
        if (it.extra) thr[ta + k++] = it.extra_t;
        d.nthr = k;
        ta += k;
        oa += 2 + (k + 63) / 64;
    }
    const GcDesc* ddescs = reinterpret_cast<const GcDesc*>(G->hin_d);
    const GcPair* dpairs = reinterpret_cast<const GcPair*>(G->hin_d + pair_at);
    const uint64_t* dthr = reinterpret_cast<const uint64_t*>(G->hin_d + thr_at);
    uint64_t* dout = reinterpret_cast<uint64_t*>(G->hout_d);
    if (kind == Pass::BIND)
        hipLaunchKernelGGL(k_gc_bind, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, ddescs, dpairs,
                           dthr, dout, n);
    else
        hipLaunchKernelGGL(k_gc_check, dim3((n + 3) / 4), dim3(256), 0, ctx->stream, ddescs, dthr,
                           dout, n);
    LJ_LAUNCHED(ctx);
    LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ++h.stats[ST_PASSES];
    const uint64_t* out = static_cast<const uint64_t*>(G->hout);
    for (uint32_t i = 0; i < n; ++i) {
        Item& it = items[i];
        const uint64_t* o = out + descs[i].out_off;
        it.status = (uint32_t)o[0];
        it.sum = o[1];
        uint32_t k = 0;
        for (GcWaiter& w : it.v->waiters) {
            w.met = w.plan == LASPJ_GC_T && ((o[2 + k / 64] >> (k % 64)) & 1);
            k += w.plan == LASPJ_GC_T ? 1 : 0;
        }
        if (it.extra) it.extra_met = (o[2 + k / 64] >> (k % 64)) & 1;
        it.v->checked = true;
    }
    return LASPJ_OK;
}

// write/4 (lasp_core.erl:839-844) of an image, call lock held: parsed, the row zeroed and
// its pairs scattered; an image the row cannot hold is kept on the host
int write_locked(laspj_ctx* ctx, GcState* G, const GcHooks& h, GcVar* v, const uint8_t* p,
                 uint64_t n, int32_t* verdict) {
    *verdict = LASPJ_NIF_FALLBACK;
    if (!ensure_dict(v->ns.get())) return fail(ctx, LASPJ_E_NOMEM, "counters: dictionary");
    std::vector<GcPair> pairs;
    const uint32_t before = dict_elements(v->ns->dict);
    const int st = gc_parse(v->ns->dict, p, n, &pairs);
    if (st < 0) return fail(ctx, st, "counters: host allocation");
    v->checked = false;
    if (st != LASPJ_DEC_OK) {
        try {
            std::vector<uint8_t> img(p, p + n);            // (p may be the old image itself)
            v->image.swap(img);
        } catch (const std::bad_alloc&) {
            return fail(ctx, LASPJ_E_NOMEM, "counters: host allocation");
        }
        v->held = true;
        v->resident = false;
        DevGuard g(ctx);
        release_row(ctx, v);
        ++h.stats[ST_FALLBACKS];
        return LASPJ_OK;
    }
    if (dict_elements(v->ns->dict) != before) ++h.stats[ST_REGISTRATIONS];
    uint32_t need = 1;
    uint64_t top = 0;
    for (const GcPair& q : pairs) {
        need = std::max(need, q.slot + 1);
        top = std::max(top, q.count);
    }
    {
        DevGuard g(ctx);
        if (int s = grow_pinned(ctx, &G->hin, &G->hin_bytes, &G->hin_d, 16ull * pairs.size() + 16)) return s;
        if (!pairs.empty()) std::memcpy(G->hin, pairs.data(), 16ull * pairs.size());
        if (int s = fit_row(ctx, v, need)) return s;
        hipLaunchKernelGGL(k_gc_grow, dim3(std::min<uint32_t>((v->cap + 255) / 256, 1024)), dim3(256),
                           0, ctx->stream, v->row, (const uint64_t*)nullptr, 0u, v->cap);
        LJ_LAUNCHED(ctx);
        if (!pairs.empty()) {
            hipLaunchKernelGGL(k_gc_scatter,
                               dim3(std::min<uint32_t>(((uint32_t)pairs.size() + 255) / 256, 1024)),
                               dim3(256), 0, ctx->stream, v->row, v->cap,
                               reinterpret_cast<const GcPair*>(G->hin_d), (uint32_t)pairs.size());
            LJ_LAUNCHED(ctx);
        }
        LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ++h.stats[ST_PASSES];
    }
    v->resident = true;
    v->held = false;
    std::vector<uint8_t>().swap(v->image);
    v->bound = top;
    *verdict = LASPJ_NIF_OK;
    return LASPJ_OK;
}

// a variable written out by laspj_nif_reset gets its row again; *ok: it is resident
int hydrate(laspj_ctx* ctx, GcState* G, const GcHooks& h, GcVar* v, bool* ok) {
    *ok = v->resident;
    if (v->resident || v->held) return LASPJ_OK;
    int32_t vd = LASPJ_NIF_FALLBACK;
    if (int s = write_locked(ctx, G, h, v, v->image.data(), v->image.size(), &vd)) return s;
    *ok = vd == LASPJ_NIF_OK;
    return LASPJ_OK;
}

// the slots in term order, the ones registered since the last read inserted
int term_order(laspj_ctx* ctx, GcNs* ns) {
    const uint32_t n = ns->dict ? dict_elements(ns->dict) : 0;
    try {
        for (uint32_t s = (uint32_t)ns->order.size(); s < n; ++s) {
            const std::string_view a = list_elem_image(ns->dict, s);
            size_t lo = 0, hi = ns->order.size();
            while (lo < hi) {
                const size_t mid = (lo + hi) / 2;
                const std::string_view b = list_elem_image(ns->dict, ns->order[mid]);
                int c = 0;
                laspj_term_compare((const uint8_t*)b.data(), b.size(), (const uint8_t*)a.data(),
                                   a.size(), &c);
                if (c < 0) lo = mid + 1; else hi = mid;
            }
            ns->order.insert(ns->order.begin() + (ptrdiff_t)lo, s);
        }
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "counters: host allocation");
    }
    return LASPJ_OK;
}

// the row read back and encoded as term_to_binary/1 of the orddict (ctx->mu not held)
int row_image(laspj_ctx* ctx, GcState* G, const GcHooks& h, GcVar* v, std::string* img) {
    std::vector<GcPair> pairs;
    if (v->row) {
        DevGuard g(ctx);
        if (int s = grow_pinned(ctx, &G->hout, &G->hout_bytes, &G->hout_d, 8ull * v->cap)) return s;
        LJ_HIP(ctx, hipMemcpyAsync(G->hout, v->row, 8ull * v->cap, hipMemcpyDeviceToHost, ctx->stream));
        LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ++h.stats[ST_PASSES];
        if (int s = term_order(ctx, v->ns.get())) return s;
        const uint64_t* row = static_cast<const uint64_t*>(G->hout);
        try {
            for (uint32_t s : v->ns->order)
                if (s < v->cap && row[s]) pairs.push_back(GcPair{row[s], s, 0});
        } catch (const std::bad_alloc&) {
            return fail(ctx, LASPJ_E_NOMEM, "counters: host allocation");
        }
    }
    try {
        gc_encode(v->ns->dict, pairs.data(), pairs.size(), img);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "counters: host allocation");
    }
    return LASPJ_OK;
}

// `increment` | `{increment, N}` from Op's image: false when riak_dt_gcounter:update/3 has
// no clause for it or N does not fit a count
bool parse_increment(const uint8_t* p, uint64_t n, uint64_t* N) {
    std::string_view img((const char*)p, n);
    auto atom = [](std::string_view s, size_t* used) {
        if (s.size() >= 3 && (s[0] == 100 || s[0] == 118) && s[1] == 0 && s[2] == 9 &&
            s.size() >= 12 && s.substr(3, 9) == "increment") {
            *used = 12;
            return true;
        }
        if (s.size() >= 11 && (s[0] == 115 || s[0] == 119) && s[1] == 9 &&
            s.substr(2, 9) == "increment") {
            *used = 11;
            return true;
        }
        return false;
    };
    if (n < 2 || p[0] != 131 || list_term_len(p + 1, n - 1) != n - 1) return false;
    size_t used = 0;
    if (atom(img.substr(1), &used) && used == n - 1) {
        *N = 1;
        return true;
    }
    if (n < 4 || p[1] != 104 || p[2] != 2 || !atom(img.substr(3), &used)) return false;
    // N: a positive integer below 2^64, through the threshold planner's exact reading
    // (`N =< V` non-strict plans t = N for exactly those)
    std::string num;
    num.push_back((char)131);
    num.append(img.substr(3 + used));
    const uint8_t tag = (uint8_t)num[1];
    if (tag != 97 && tag != 98 && tag != 110 && tag != 111) return false;
    return gc_threshold_plan((const uint8_t*)num.data(), num.size(), false, N) == LASPJ_GC_T;
}

// the met waiters' ids in list order, removed (reply_to_all, lasp_core.erl:765-825)
uint32_t count_met(const GcVar* v) {
    uint32_t k = 0;
    for (const GcWaiter& w : v->waiters) k += w.met ? 1 : 0;
    return k;
}

struct Entry {
    laspj_ctx* ctx = nullptr;
    GcHooks h;
    GcState* G = nullptr;
    std::unique_lock<std::mutex> lk;
};

// the call lock taken and the variable found in its context's state
int enter(GcVar* v, Entry* e) {
    if (!v || !v->ctx) return LASPJ_E_INVAL;
    e->ctx = v->ctx;
    if (!nif_gc_hooks(e->ctx, &e->h)) return fail(e->ctx, LASPJ_E_NOMEM, "nif: state allocation");
    e->lk = std::unique_lock<std::mutex>(*e->h.mu);
    e->G = gstate(e->h);
    if (!e->G) return fail(e->ctx, LASPJ_E_NOMEM, "counters: state allocation");
    if (!e->G->vars.count(v)) return fail(e->ctx, LASPJ_E_INVAL, "counters: unknown variable");
    return LASPJ_OK;
}

}  // namespace

laspj_ctx* gc_var_ctx(const GcVar* v) { return v ? v->ctx : nullptr; }

int gc_var_create(laspj_ctx* ctx, GcVar* peer, GcVar** out) {
    GcHooks h;
    if (!nif_gc_hooks(ctx, &h)) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(*h.mu);
    GcState* G = gstate(h);
    if (!G) return fail(ctx, LASPJ_E_NOMEM, "counters: state allocation");
    if (peer && !G->vars.count(peer))
        return fail(ctx, LASPJ_E_INVAL, "var_create_replica: unknown variable");
    try {
        std::unique_ptr<GcVar> v(new GcVar);
        v->ctx = ctx;
        v->ns = peer ? peer->ns : std::make_shared<GcNs>();
        G->vars.insert(v.get());
        *out = v.release();
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "var_create: host allocation");
    }
    return LASPJ_OK;
}

int gc_var_destroy(GcVar* v) {
    if (!v) return LASPJ_E_INVAL;
    if (v->ctx) {
        Entry e;
        if (enter(v, &e) == LASPJ_OK) {
            e.G->vars.erase(v);
            DevGuard g(e.ctx);
            release_row(e.ctx, v);
        }
    }
    delete v;
    return LASPJ_OK;
}

int gc_bind_many(laspj_ctx* ctx, uint32_t n, GcVar* const* vars, const uint8_t* const* values,
                 const uint64_t* lens, int32_t* status, int32_t* verdict) {
    GcHooks h;
    if (!nif_gc_hooks(ctx, &h)) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(*h.mu);
    GcState* G = gstate(h);
    if (!G) return fail(ctx, LASPJ_E_NOMEM, "counters: state allocation");
    try {
        std::unordered_set<const GcVar*> seen;
        for (uint32_t i = 0; i < n; ++i) {
            if (!vars[i] || vars[i]->ctx != ctx || !G->vars.count(vars[i]))
                return fail(ctx, LASPJ_E_INVAL, "var_bind: variable %u is not this context's", i);
            if (!values[i] && lens[i]) return fail(ctx, LASPJ_E_INVAL, "var_bind: null payload");
            if (!seen.insert(vars[i]).second)
                return fail(ctx, LASPJ_E_INVAL, "var_bind: variable %u named twice", i);
        }
        ++h.stats[ST_CALLS];
        std::vector<Item> items;
        std::vector<uint32_t> at;
        bool registered = false;
        for (uint32_t i = 0; i < n; ++i) {
            GcVar* v = vars[i];
            status[i] = LASPJ_BIND_NOOP;
            verdict[i] = LASPJ_NIF_FALLBACK;
            bool ok = false;
            if (int s = hydrate(ctx, G, h, v, &ok)) return s;
            Item it;
            it.v = v;
            int st = LASPJ_DEC_UNREPRESENTABLE;
            if (ok) {
                if (!ensure_dict(v->ns.get())) return fail(ctx, LASPJ_E_NOMEM, "counters: dictionary");
                const uint32_t before = dict_elements(v->ns->dict);
                st = gc_parse(v->ns->dict, values[i], lens[i], &it.pairs);
                if (st < 0) return fail(ctx, st, "counters: host allocation");
                registered |= dict_elements(v->ns->dict) != before;
            }
            if (st != LASPJ_DEC_OK) {
                ++h.stats[ST_FALLBACKS];
                continue;
            }
            items.push_back(std::move(it));
            at.push_back(i);
        }
        if (registered) ++h.stats[ST_REGISTRATIONS];
        if (items.empty()) return LASPJ_OK;
        if (int s = run_pass(ctx, G, h, Pass::BIND, items)) return s;
        for (size_t k = 0; k < items.size(); ++k) {
            status[at[k]] = (int32_t)items[k].status;
            verdict[at[k]] = LASPJ_NIF_OK;
            for (const GcPair& p : items[k].pairs)
                items[k].v->bound = std::max(items[k].v->bound, p.count);
        }
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "var_bind: host allocation");
    }
    return LASPJ_OK;
}

int gc_write(GcVar* v, const uint8_t* value, uint64_t n, int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if ((!value && n) || !verdict) return fail(e.ctx, LASPJ_E_INVAL, "var_write: null argument");
    ++e.h.stats[ST_CALLS];
    return write_locked(e.ctx, e.G, e.h, v, value, n, verdict);
}

int gc_read(GcVar* v, bool value, const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if (!out || !out_len || !verdict) return fail(e.ctx, LASPJ_E_INVAL, "var: null output");
    ++e.h.stats[ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    bool ok = false;
    if (int s = hydrate(e.ctx, e.G, e.h, v, &ok)) return s;
    try {
        if (!ok) {
            // a host-held value: read answers its image, value/1 is the NIF's to compute
            if (value) {
                ++e.h.stats[ST_FALLBACKS];
                return LASPJ_OK;
            }
            e.G->answer.assign((const char*)v->image.data(), v->image.size());
        } else if (!value) {
            if (!ensure_dict(v->ns.get())) return fail(e.ctx, LASPJ_E_NOMEM, "counters: dictionary");
            if (int s = row_image(e.ctx, e.G, e.h, v, &e.G->answer)) return s;
        } else {
            // riak_dt_gcounter:value/1: the sum (it wraps at 2^64, as the batch path's)
            std::vector<Item> items(1);
            items[0].v = v;
            if (int s = run_pass(e.ctx, e.G, e.h, Pass::CHECK, items)) return s;
            e.G->answer.assign(1, (char)131);
            gc_put_uint(&e.G->answer, items[0].sum);
        }
    } catch (const std::bad_alloc&) {
        return fail(e.ctx, LASPJ_E_NOMEM, "var: host allocation");
    }
    *out = (const uint8_t*)e.G->answer.data();
    *out_len = e.G->answer.size();
    *verdict = LASPJ_NIF_OK;
    return LASPJ_OK;
}

int gc_threshold(GcVar* v, const uint8_t* threshold, uint64_t n, int strict, int32_t* result,
                 int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if ((!threshold && n) || !result || !verdict)
        return fail(e.ctx, LASPJ_E_INVAL, "var_threshold: null argument");
    ++e.h.stats[ST_CALLS];
    *result = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    bool ok = false;
    if (int s = hydrate(e.ctx, e.G, e.h, v, &ok)) return s;
    uint64_t t = 0;
    const int plan = gc_threshold_plan(threshold, n, strict != 0, &t);
    if (!ok || plan < 0) {
        ++e.h.stats[ST_FALLBACKS];
        return LASPJ_OK;
    }
    *verdict = LASPJ_NIF_OK;
    if (plan != LASPJ_GC_T) {
        *result = plan == LASPJ_GC_ALWAYS;
        return LASPJ_OK;
    }
    try {
        std::vector<Item> items(1);
        items[0].v = v;
        items[0].extra = true;
        items[0].extra_t = t;
        if (int s = run_pass(e.ctx, e.G, e.h, Pass::CHECK, items)) return s;
        *result = items[0].extra_met;
    } catch (const std::bad_alloc&) {
        return fail(e.ctx, LASPJ_E_NOMEM, "var_threshold: host allocation");
    }
    return LASPJ_OK;
}

int gc_resident(const GcVar* v, int32_t* resident) {
    if (!v || !resident) return LASPJ_E_INVAL;
    *resident = v->ctx && v->resident ? 1 : 0;
    return LASPJ_OK;
}

int gc_refuse(GcVar* v, int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if (!verdict) return fail(e.ctx, LASPJ_E_INVAL, "var: null argument");
    ++e.h.stats[ST_CALLS];
    ++e.h.stats[ST_FALLBACKS];
    *verdict = LASPJ_NIF_FALLBACK;
    return LASPJ_OK;
}

int gc_wait(GcVar* v, const uint8_t* threshold, uint64_t n, int strict, uint64_t id, int32_t* met,
            int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if ((!threshold && n) || !met || !verdict)
        return fail(e.ctx, LASPJ_E_INVAL, "var_wait: null argument");
    ++e.h.stats[ST_CALLS];
    *met = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    bool ok = false;
    if (int s = hydrate(e.ctx, e.G, e.h, v, &ok)) return s;
    uint64_t t = 0;
    const int plan = gc_threshold_plan(threshold, n, strict != 0, &t);
    if (!ok || plan < 0) {
        ++e.h.stats[ST_FALLBACKS];
        return LASPJ_OK;
    }
    try {
        if (plan == LASPJ_GC_T) {
            std::vector<Item> items(1);
            items[0].v = v;
            items[0].extra = true;
            items[0].extra_t = t;
            if (int s = run_pass(e.ctx, e.G, e.h, Pass::CHECK, items)) return s;
            if (items[0].extra_met) *met = 1;
        } else if (plan == LASPJ_GC_ALWAYS) {
            *met = 1;
        }
        *verdict = LASPJ_NIF_OK;
        if (*met) return LASPJ_OK;
        // unmet (lasp_core.erl:355-364): appended to waiting_threads
        GcWaiter w;
        w.id = id;
        w.strict = strict ? 1 : 0;
        w.image.assign(threshold, threshold + n);
        w.plan = plan;
        w.t = t;
        v->waiters.push_back(std::move(w));
    } catch (const std::bad_alloc&) {
        *verdict = LASPJ_NIF_FALLBACK;
        return fail(e.ctx, LASPJ_E_NOMEM, "var_wait: host allocation");
    }
    return LASPJ_OK;
}

int gc_recheck_check(laspj_ctx* ctx, uint32_t n, GcVar* const* vars, uint32_t* nmet,
                     int32_t* verdict) {
    GcHooks h;
    if (!nif_gc_hooks(ctx, &h)) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    GcState* G = gstate(h);
    if (!G) return fail(ctx, LASPJ_E_NOMEM, "counters: state allocation");
    try {
        std::vector<Item> items;
        for (uint32_t i = 0; i < n; ++i) {
            GcVar* v = vars[i];
            if (!v || v->ctx != ctx || !G->vars.count(v))
                return fail(ctx, LASPJ_E_INVAL, "var_recheck: variable %u is not this context's", i);
            nmet[i] = 0;
            verdict[i] = LASPJ_NIF_FALLBACK;
            bool ok = false;
            if (int s = hydrate(ctx, G, h, v, &ok)) return s;
            if (!ok) {
                ++h.stats[ST_FALLBACKS];
                continue;
            }
            verdict[i] = LASPJ_NIF_OK;
            // (a variable with no waiter a kernel could fire does no device work, and one
            // whose waiters the last pass checked against this value keeps its answers)
            if (!v->checked && checkable(v)) {
                Item it;
                it.v = v;
                items.push_back(std::move(it));
            }
        }
        if (!items.empty())
            if (int s = run_pass(ctx, G, h, Pass::CHECK, items)) return s;
        for (uint32_t i = 0; i < n; ++i)
            if (verdict[i] == LASPJ_NIF_OK) nmet[i] = count_met(vars[i]);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "var_recheck: host allocation");
    }
    return LASPJ_OK;
}

void gc_recheck_take(GcVar* v, uint64_t* ids) {
    size_t keep = 0, at = 0;
    for (size_t k = 0; k < v->waiters.size(); ++k) {
        if (v->waiters[k].met) {
            ids[at++] = v->waiters[k].id;
        } else {
            if (keep != k) v->waiters[keep] = std::move(v->waiters[k]);
            ++keep;
        }
    }
    v->waiters.resize(keep);
}

int gc_recheck(GcVar* v, uint64_t* ids, uint32_t cap, uint32_t* nmet, uint32_t* nwaiting,
               int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if ((!ids && cap) || !nmet || !nwaiting || !verdict)
        return fail(e.ctx, LASPJ_E_INVAL, "var_recheck: null argument");
    ++e.h.stats[ST_CALLS];
    *nmet = 0;
    const int s = gc_recheck_check(e.ctx, 1, &v, nmet, verdict);
    if (s == LASPJ_OK && *nmet && *nmet <= cap) gc_recheck_take(v, ids);
    *nwaiting = (uint32_t)v->waiters.size();
    return s;
}

int gc_wait_cancel(GcVar* v, uint64_t id, int32_t* found) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if (!found) return fail(e.ctx, LASPJ_E_INVAL, "var_wait_cancel: null argument");
    *found = 0;
    for (size_t k = 0; k < v->waiters.size(); ++k)
        if (v->waiters[k].id == id) {
            v->waiters.erase(v->waiters.begin() + (ptrdiff_t)k);
            *found = 1;
            break;
        }
    return LASPJ_OK;
}

int gc_waiter_count(const GcVar* v, uint32_t* n) {
    Entry e;
    if (int s = enter(const_cast<GcVar*>(v), &e)) return s;
    if (!n) return LASPJ_E_INVAL;
    *n = (uint32_t)v->waiters.size();
    return LASPJ_OK;
}

int gc_waiter_at(GcVar* v, uint32_t k, uint64_t* id, int32_t* strict, const uint8_t** threshold,
                 uint64_t* n) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    if (!id || !strict || !threshold || !n)
        return fail(e.ctx, LASPJ_E_INVAL, "var_waiter_at: null argument");
    if (k >= v->waiters.size()) return fail(e.ctx, LASPJ_E_RANGE, "var_waiter_at: no waiter %u", k);
    const GcWaiter& w = v->waiters[k];
    *id = w.id;
    *strict = w.strict;
    *threshold = w.image.data();
    *n = w.image.size();
    return LASPJ_OK;
}

int gc_increment(GcVar* v, const uint8_t* op, uint64_t nop, const uint8_t* actor, uint64_t nactor,
                 uint64_t* ids, uint32_t cap, uint32_t* nmet, uint32_t* nwaiting,
                 int32_t* verdict) {
    Entry e;
    if (int s = enter(v, &e)) return s;
    laspj_ctx* ctx = e.ctx;
    if (!op || !nop || !actor || !nactor || !verdict || (!ids && cap) || (ids && (!nmet || !nwaiting)))
        return fail(ctx, LASPJ_E_INVAL, "var_increment: null argument");
    ++e.h.stats[ST_CALLS];
    *verdict = LASPJ_NIF_FALLBACK;
    if (nmet) *nmet = 0;
    if (nwaiting) *nwaiting = (uint32_t)v->waiters.size();
    bool ok = false;
    if (int s = hydrate(ctx, e.G, e.h, v, &ok)) return s;
    uint64_t N = 0;
    uint32_t slot = 0;
    bool fresh = false;
    if (ok) ok = parse_increment(op, nop, &N);
    if (ok) {
        // Actor joins the namespace (undone below when the call answers FALLBACK)
        ok = nactor >= 2 && actor[0] == 131 && list_term_len(actor + 1, nactor - 1) == nactor - 1 &&
             ensure_dict(v->ns.get());
        if (ok) {
            const uint32_t before = dict_elements(v->ns->dict);
            dict_begin(v->ns->dict);
            const int st = dict_reg_elem(v->ns->dict, actor + 1, nactor - 1, &slot);
            if (st < 0) return fail(ctx, st, "var_increment: host allocation");
            fresh = dict_elements(v->ns->dict) != before;
            ok = st == LASPJ_DEC_OK && dict_elements(v->ns->dict) <= kGcMaxActors;
            if (!ok) dict_rollback(v->ns->dict);
        }
    }
    if (!ok) {
        ++e.h.stats[ST_FALLBACKS];
        return LASPJ_OK;
    }
    // a count could pass 2^64 - 1 only above the row's bound: then the kernel's own check
    // is read back even when nobody asked for the waiters
    const bool may_wrap = v->bound > ~0ull - N;
    const bool answer = ids || may_wrap;
    const uint32_t k = answer ? checkable(v) : 0;
    uint64_t status = 0;
    {
        DevGuard g(ctx);
        if (answer) {
            if (int s = grow_pinned(ctx, &e.G->hin, &e.G->hin_bytes, &e.G->hin_d, 8ull * k + 16)) return s;
            if (int s = grow_pinned(ctx, &e.G->hout, &e.G->hout_bytes, &e.G->hout_d,
                                    8ull * (2 + (k + 63) / 64)))
                return s;
            uint64_t* thr = static_cast<uint64_t*>(e.G->hin);
            uint32_t j = 0;
            for (const GcWaiter& w : v->waiters)
                if (w.plan == LASPJ_GC_T) thr[j++] = w.t;
        }
        if (int s = fit_row(ctx, v, slot + 1)) return s;
        hipLaunchKernelGGL(k_gc_incr, dim3(1), dim3(256), 0, ctx->stream, v->row, v->cap, slot, N,
                           answer ? reinterpret_cast<const uint64_t*>(e.G->hin_d) : nullptr, k,
                           answer ? reinterpret_cast<uint64_t*>(e.G->hout_d) : nullptr);
        LJ_LAUNCHED(ctx);
        ++e.h.stats[ST_PASSES];
        if (answer) {
            LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
            status = static_cast<const uint64_t*>(e.G->hout)[0];
        }
    }
    if (status) {
        // the count would pass 2^64 - 1: nothing was written (its actor held a count already)
        if (fresh) dict_rollback(v->ns->dict);
        ++e.h.stats[ST_FALLBACKS];
        return LASPJ_OK;
    }
    if (fresh) ++e.h.stats[ST_REGISTRATIONS];
    v->bound = may_wrap ? ~0ull : v->bound + N;
    *verdict = LASPJ_NIF_OK;
    if (!answer) {
        v->checked = false;                                // returned once enqueued
        return LASPJ_OK;
    }
    const uint64_t* o = static_cast<const uint64_t*>(e.G->hout);
    uint32_t j = 0;
    for (GcWaiter& w : v->waiters) {
        w.met = w.plan == LASPJ_GC_T && ((o[2 + j / 64] >> (j % 64)) & 1);
        j += w.plan == LASPJ_GC_T ? 1 : 0;
    }
    v->checked = true;
    if (!ids) return LASPJ_OK;
    // answered as laspj_var_recheck would have
    *nmet = count_met(v);
    if (*nmet && *nmet <= cap) gc_recheck_take(v, ids);
    *nwaiting = (uint32_t)v->waiters.size();
    return LASPJ_OK;
}

uint64_t gc_dict_elements(const GcState* G) {
    uint64_t tot = 0;
    if (!G) return 0;
    std::unordered_set<const GcNs*> seen;
    for (const GcVar* v : G->vars)
        if (v->ns->dict && seen.insert(v->ns.get()).second) tot += dict_elements(v->ns->dict);
    return tot;
}

int gc_ctx_reset(laspj_ctx* ctx, GcState* G) {
    if (!G) return LASPJ_OK;
    GcHooks h;
    if (!nif_gc_hooks(ctx, &h)) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    // every resident row written out to its image (decoded again by the variable's next
    // call), then each namespace starts afresh
    for (GcVar* v : G->vars) {
        if (!v->resident || !v->row) continue;
        std::string img;
        if (int s = row_image(ctx, G, h, v, &img)) return s;
        try {
            v->image.assign(img.begin(), img.end());
        } catch (const std::bad_alloc&) {
            return fail(ctx, LASPJ_E_NOMEM, "counters: host allocation");
        }
        v->resident = false;
        v->checked = false;
        DevGuard g(ctx);
        release_row(ctx, v);
    }
    for (GcVar* v : G->vars) {
        if (v->ns->dict) laspj_dict_destroy(v->ns->dict);
        v->ns->dict = nullptr;
        v->ns->order.clear();
    }
    return LASPJ_OK;
}

void gc_ctx_destroy(laspj_ctx* ctx, GcState* G) {
    if (!G) return;
    {
        DevGuard g(ctx);
        for (GcVar* v : G->vars) {
            release_row(ctx, v);                           // (into the cache the context frees)
            v->ctx = nullptr;
            v->resident = false;
        }
        hipStreamSynchronize(ctx->stream);
        if (G->hin) hipHostFree(G->hin);
        if (G->hout) hipHostFree(G->hout);
    }
    delete G;
}

}  // namespace laspj
