// Waiting and lazy threads of resident variables (include/laspj.h "resident variables":
// laspj_var_wait*, _recheck*, _waiter_*, _wait_needed, _read, _read_any,
// _lazy_*): the waiter re-check and its kernels, and the one-pass blocking reads (the read
// check's kernels are laspj_reads.hip's).

#include "laspj_nif_internal.h"

namespace laspj {
namespace {

// write/4's reply_to_all (lasp_core.erl:839-844, 765-825) over resident variables: every
// waiter's threshold_met(Type, Value, Threshold) (lasp_lattice.erl:62-75) in one launch.
// A wave item is (variable, tile of kWaitTile 16-byte units of its value, chunk of
// kWaitChunk of its waiters): the value's tile is read once into registers and compared
// with the same units of each waiter of the chunk.  A unit is a {p, r} pair of an OR-Set
// cell (tw of them per element in a wide namespace) or two bitmap words of a G-Set; units
// past the end of a block of cells are absent (a waiter registered before its namespace
// grew covers fewer element slots than the value; null cells — a [] threshold, a variable
// still holding new() — cover none).
//   OR-Set (lasp_lattice.erl:153-161): violation = some cell has pP & ~pC; strict
//     (:235-253) also needs a common element's cell to differ, removed flags included
//     (`Ids =/= Ids1`), or np < nc (which is also the [] -> non-empty clause)
//   wide: the same per {p, r} pair; strict = and some pair differs
//   G-Set (:137-140, 212-215): violation = p & ~c; strict also needs the words to differ
// Records (zeroed ahead of the launch): per waiter {flags: 1 violation, 2 changed; np},
// per variable nc (a property of the value alone: counted by the first chunk's waves);
// device-scope atomics, one per wave and nonzero result.  The met flags are written to
// the pinned answer area by a one-block finish launch behind the check.
constexpr uint32_t kWaitTile = 128;     // units per wave item: two per lane
constexpr uint32_t kWaitChunk = 16;     // waiters per wave item
constexpr uint32_t kWaitNarrow = 0, kWaitWide = 1, kWaitGset = 2;
struct WaitVar {
    const uint64_t* cells;
    uint32_t words;                     // u64 words of `cells`
    uint32_t mode;
    uint32_t w0, nw;                    // its waiters: WaitDesc [w0, w0 + nw)
    uint64_t item0;                     // its first wave item
};
struct WaitDesc {
    const uint64_t* cells;
    uint32_t words;
    uint32_t var_strict;                // variable index << 1 | strict
};
static_assert(sizeof(WaitVar) == 32 && sizeof(WaitDesc) == 16, "descriptor layout");
typedef unsigned long long wait2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ wait2 wait_ld(const uint64_t* base, uint64_t q, uint32_t words) {
    wait2 v = {0ull, 0ull};
    if (2 * q + 1 < words) v = *reinterpret_cast<const wait2*>(base + 2 * q);
    else if (2 * q < words) v.x = base[2 * q];
    return v;
}

__device__ __forceinline__ void wait_finish(uint32_t j, const WaitVar* vars, const WaitDesc* ws,
                                            uint32_t* rec, uint32_t* nc, uint8_t* met) {
    const uint32_t vs = ws[j].var_strict, v = vs >> 1;
    const uint32_t f = __hip_atomic_load(rec + 2 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t np = __hip_atomic_load(rec + 2 * j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint32_t ncv = __hip_atomic_load(nc + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool infl = !(f & 1u);
    bool res = infl;
    if (vs & 1u) res = infl && ((f & 2u) || (vars[v].mode == kWaitNarrow && np < ncv));
    met[j] = res ? 1 : 0;
}

__global__ void __launch_bounds__(256) k_waiter_check(const WaitVar* vars, uint32_t nv,
                                                      const WaitDesc* ws, uint64_t items,
                                                      uint32_t* rec, uint32_t* nc) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t s = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; s < items; s += nwaves) {
        uint32_t lo = 0, hi = nv;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (vars[mid].item0 <= s) lo = mid;
            else hi = mid;
        }
        const WaitVar V = vars[lo];
        const uint32_t nch = (V.nw + kWaitChunk - 1) / kWaitChunk;
        const uint64_t local = s - V.item0, tile = local / nch;
        const uint32_t ch = (uint32_t)(local - tile * nch);
        const uint64_t q0 = tile * kWaitTile + lane, q1 = q0 + 64;
        const wait2 c0 = wait_ld(V.cells, q0, V.words), c1 = wait_ld(V.cells, q1, V.words);
        if (ch == 0 && V.mode == kWaitNarrow) {
            const uint32_t n = __popcll(__ballot(c0.x != 0)) + __popcll(__ballot(c1.x != 0));
            if (lane == 0 && n) atomicAdd(nc + lo, n);
        }
        const uint32_t j0 = V.w0 + ch * kWaitChunk, j1 = min(V.w0 + V.nw, j0 + kWaitChunk);
        // the chunk's descriptors: one per lane, handed round by shuffles
        uint64_t dp = 0;
        uint32_t dw = 0;
        if (j0 + lane < j1) {
            dp = reinterpret_cast<uint64_t>(ws[j0 + lane].cells);
            dw = ws[j0 + lane].words;
        }
        for (uint32_t j = j0; j < j1; j += 4) {
            wait2 p0[4], p1[4];
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                // (lanes past the chunk hold no words: nothing is read for them)
                const auto* P = reinterpret_cast<const uint64_t*>(
                    (uint64_t)__shfl((unsigned long long)dp, (int)(j + k - j0), 64));
                const uint32_t w = __shfl(dw, (int)(j + k - j0), 64);
                p0[k] = wait_ld(P, q0, w);
                p1[k] = wait_ld(P, q1, w);
            }
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k) {
                if (j + k >= j1) break;
                const wait2 a = p0[k], b = p1[k];
                bool viol, changed;
                uint32_t np = 0;
                if (V.mode == kWaitNarrow) {
                    viol = ((a.x & ~c0.x) | (b.x & ~c1.x)) != 0;
                    changed = ((a.x != 0) & (c0.x != 0) & ((a.x != c0.x) | (a.y != c0.y))) |
                              ((b.x != 0) & (c1.x != 0) & ((b.x != c1.x) | (b.y != c1.y)));
                    np = __popcll(__ballot(a.x != 0)) + __popcll(__ballot(b.x != 0));
                } else if (V.mode == kWaitWide) {
                    viol = ((a.x & ~c0.x) | (b.x & ~c1.x)) != 0;
                    changed = (a.x != c0.x) | (a.y != c0.y) | (b.x != c1.x) | (b.y != c1.y);
                } else {
                    viol = ((a.x & ~c0.x) | (a.y & ~c0.y) | (b.x & ~c1.x) | (b.y & ~c1.y)) != 0;
                    changed = (a.x != c0.x) | (a.y != c0.y) | (b.x != c1.x) | (b.y != c1.y);
                }
                const uint32_t f = (__ballot(viol) != 0 ? 1u : 0u) | (__ballot(changed) != 0 ? 2u : 0u);
                if (lane == 0) {
                    if (f) atomicOr(rec + 2 * (j + k), f);
                    if (np) atomicAdd(rec + 2 * (j + k) + 1, np);
                }
            }
        }
    }
}

__global__ void __launch_bounds__(256) k_waiter_finish(const WaitVar* vars, const WaitDesc* ws,
                                                       uint32_t nws, uint32_t* rec, uint32_t* nc,
                                                       uint8_t* met) {
    for (uint32_t j = threadIdx.x; j < nws; j += 256) wait_finish(j, vars, ws, rec, nc, met);
}

// reply_to_all's test (lasp_core.erl:765-825) for every waiter of n variables in one device
// pass (S->mu held).  verdict[i]: FALLBACK when variable i's value, or one of its waiters'
// thresholds, is held on the host; met[i]: one flag per waiter of variable i, in list
// order (empty when it has no waiters or answered FALLBACK).  No device work when no
// variable has a waiter to check.
int recheck_pass(laspj_ctx* ctx, NifState* S, uint32_t n, laspj_var* const* vars,
                 int32_t* verdict, std::vector<std::vector<uint8_t>>* met) {
    ++S->stats[ST_CALLS];
    met->assign(n, {});
    std::vector<uint32_t> live;
    uint32_t nws = 0;
    for (uint32_t i = 0; i < n; ++i) {
        laspj_var* v = vars[i];
        bool ok = false;
        if (int s = hydrate(ctx, S, v, &ok)) return s;
        verdict[i] = ok ? LASPJ_NIF_OK : LASPJ_NIF_FALLBACK;
        for (size_t k = 0; ok && k < v->waiters.size(); ++k)
            if (int s = hydrate(ctx, S, v->waiters[k].cells, &ok)) return s;
        if (!ok) verdict[i] = LASPJ_NIF_FALLBACK;
    }
    for (uint32_t i = 0; i < n; ++i) {
        // (a decode above may have started a namespace's dictionary afresh and written the
        // cells decoded before it out again: such a variable answers FALLBACK this once)
        laspj_var* v = vars[i];
        bool ok = verdict[i] == LASPJ_NIF_OK && laspj::var_current(v);
        for (const Waiter& w : v->waiters) ok = ok && laspj::var_current(w.cells);
        verdict[i] = ok ? LASPJ_NIF_OK : LASPJ_NIF_FALLBACK;
        if (!ok) {
            ++S->stats[ST_FALLBACKS];
        } else if (!v->waiters.empty()) {
            live.push_back(i);
            nws += (uint32_t)v->waiters.size();
        }
    }
    if (live.empty()) return LASPJ_OK;
    const uint64_t t0 = now_ns();
    const uint32_t nv = (uint32_t)live.size();
    // in region (pinned, read by the kernel in place): [WaitVar x nv | WaitDesc x nws];
    // device words: [{flags, np} x nws | nc x nv]; answers: nws bytes
    const uint64_t i_ws = 32ull * nv, in_bytes = i_ws + 16ull * nws;
    const uint64_t z_nc = 8ull * nws, z_bytes = al(z_nc + 4ull * nv, 16);
    Guard g(ctx);
    if (int s = grow_dev(ctx, &S->dblk, &S->dblk_bytes, z_bytes)) return s;
    if (int s = fit_staging(ctx, S, in_bytes, nws)) return s;
    auto* hv = reinterpret_cast<WaitVar*>(S->hin);
    auto* hw = reinterpret_cast<WaitDesc*>(static_cast<uint8_t*>(S->hin) + i_ws);
    uint64_t items = 0;
    uint32_t w0 = 0;
    for (uint32_t a = 0; a < nv; ++a) {
        laspj_var* v = vars[live[a]];
        const KindState& K = *v->ns;
        const uint32_t tw = ktw(K);
        // the value over the namespace's element slots (new(): zeroed cells); a waiter's
        // cells are re-laid only when the pairs per element changed (the namespace went
        // wide since): the slots it does not cover are absent
        if (K.E)
            if (int s = fit_var(ctx, v, K.E, tw)) return s;
        const uint32_t nw = (uint32_t)v->waiters.size();
        WaitVar& d = hv[a];
        d.cells = v->cells;
        d.words = v->cells ? (uint32_t)wpr_of(v->kind, v->E, v->tw) : 0;
        d.mode = v->kind == LASPJ_KIND_GSET ? kWaitGset : tw > 1 ? kWaitWide : kWaitNarrow;
        d.w0 = w0;
        d.nw = nw;
        d.item0 = items;
        const uint64_t units = (d.words + 1ull) / 2;
        items += ((units + kWaitTile - 1) / kWaitTile) * ((nw + kWaitChunk - 1) / kWaitChunk);
        for (uint32_t k = 0; k < nw; ++k) {
            laspj_var* c = v->waiters[k].cells;
            if (c->cells && v->kind == LASPJ_KIND_ORSET && c->tw != tw)
                if (int s = fit_var(ctx, c, K.E, tw)) return s;
            WaitDesc& e = hw[w0 + k];
            e.cells = c->cells;
            e.words = c->cells ? (uint32_t)wpr_of(c->kind, c->E, c->tw) : 0;
            e.var_strict = a << 1 | (v->waiters[k].strict ? 1u : 0u);
        }
        w0 += nw;
    }
    uint8_t* dz = static_cast<uint8_t*>(S->dblk);
    auto* rec = reinterpret_cast<uint32_t*>(dz);
    auto* nc = reinterpret_cast<uint32_t*>(dz + z_nc);
    const auto* dv = reinterpret_cast<const WaitVar*>(S->hin_d);
    const auto* dw = reinterpret_cast<const WaitDesc*>(S->hin_d + i_ws);
    LJ_HIP(ctx, hipMemsetAsync(dz, 0, z_bytes, ctx->stream));
    const unsigned grid = (unsigned)std::max<uint64_t>(
        1, std::min<uint64_t>((items + 3) / 4, (uint64_t)ctx->cus * 8));
    hipLaunchKernelGGL(k_waiter_check, dim3(grid), dim3(256), 0, ctx->stream, dv, nv, dw, items,
                       rec, nc);
    LJ_LAUNCHED(ctx);
    hipLaunchKernelGGL(k_waiter_finish, dim3(1), dim3(256), 0, ctx->stream, dv, dw, nws, rec, nc,
                       S->hout_d);
    LJ_LAUNCHED(ctx);
    const uint64_t t1 = now_ns();
    LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t t2 = now_ns();
    ++S->stats[ST_PASSES];
    S->stats[ST_NS_ENQUEUE] += t1 - t0;
    S->stats[ST_NS_WAIT] += t2 - t1;
    const uint8_t* hout = static_cast<const uint8_t*>(S->hout);
    w0 = 0;
    for (uint32_t a = 0; a < nv; ++a) {
        const uint32_t nw = (uint32_t)vars[live[a]]->waiters.size();
        (*met)[live[a]].assign(hout + w0, hout + w0 + nw);
        w0 += nw;
    }
    S->stats[ST_NS_ANSWERS] += now_ns() - t2;
    return LASPJ_OK;
}

}  // namespace

// a waiter's hidden variable leaves the registries and the device (S->mu held when the
// context is alive)
void waiter_cells_drop(laspj::NifState* S, laspj_var* c) {
    if (!c) return;
    if (c->ctx && S) {
        S->vars.erase(c);
        c->ns->vars.erase(c);
        std::lock_guard<std::mutex> lk(c->ctx->mu);
        hipSetDevice(c->ctx->device);
        laspj::release_cells(c->ctx, c);
    }
    delete c;
}

}  // namespace laspj

using laspj::fail;
using laspj::kinds_of;
using laspj::var_state;

namespace {

// reply_to_all (lasp_core.erl:765-825) over n variables, S->mu held: the met waiters' ids
// in list order per variable; removed unless more than cap are met
int recheck_locked(laspj_ctx* ctx, laspj::NifState* S, uint32_t n, laspj_var* const* vars,
                   uint64_t* ids, uint32_t cap, uint32_t* nmet, int32_t* verdict) {
    std::vector<std::vector<uint8_t>> met;
    if (int s = laspj::recheck_pass(ctx, S, n, vars, verdict, &met)) return s;
    uint64_t total = 0;
    for (uint32_t i = 0; i < n; ++i) {
        nmet[i] = 0;
        for (uint8_t m : met[i]) nmet[i] += m ? 1u : 0u;
        total += nmet[i];
    }
    if (total > cap || (total && !ids)) return LASPJ_OK;
    uint64_t at = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (!nmet[i]) continue;
        std::vector<laspj::Waiter>& ws = vars[i]->waiters;
        size_t keep = 0;
        for (size_t k = 0; k < ws.size(); ++k) {
            if (met[i][k]) {
                ids[at++] = ws[k].id;
                waiter_cells_drop(S, ws[k].cells);
            } else {
                if (keep != k) ws[keep] = std::move(ws[k]);
                ++keep;
            }
        }
        ws.resize(keep);
    }
    return LASPJ_OK;
}

// recheck_many over counters (and sets beside them), S->mu held: the counters are checked
// first and nothing removed; the sets then answer as ever with the room the counters leave
// (more met than that: they remove nothing either); the ids are laid out in argument order
int recheck_mixed(laspj_ctx* ctx, laspj::NifState* S, uint32_t n, laspj_var* const* vars,
                  uint64_t* ids, uint32_t cap, uint32_t* nmet, int32_t* verdict) {
    std::vector<laspj_var*> sets;
    std::vector<laspj::GcVar*> gcs;
    std::vector<uint32_t> sat, gat;
    std::unordered_set<laspj_var*> seen;
    for (uint32_t i = 0; i < n; ++i) {
        if (!vars[i] || !seen.insert(vars[i]).second)
            return fail(ctx, LASPJ_E_INVAL, "var_recheck: variable %u null or named twice", i);
        if (vars[i]->gc) {
            gcs.push_back(vars[i]->gc);
            gat.push_back(i);
        } else {
            if (vars[i]->ctx != ctx || !S->vars.count(vars[i]))
                return fail(ctx, LASPJ_E_INVAL, "var_recheck: variable %u is not this context's", i);
            sets.push_back(vars[i]);
            sat.push_back(i);
        }
    }
    std::vector<uint32_t> gmet(gcs.size(), 0), smet(sets.size(), 0);
    std::vector<int32_t> gvd(gcs.size(), LASPJ_NIF_FALLBACK), svd(sets.size(), LASPJ_NIF_FALLBACK);
    if (int s = laspj::gc_recheck_check(ctx, (uint32_t)gcs.size(), gcs.data(), gmet.data(), gvd.data()))
        return s;
    uint64_t gtotal = 0;
    for (uint32_t m : gmet) gtotal += m;
    const uint32_t room = gtotal <= cap ? cap - (uint32_t)gtotal : 0;
    std::vector<uint64_t> sids(room);
    uint64_t stotal = 0;
    if (!sets.empty()) {
        if (int s = recheck_locked(ctx, S, (uint32_t)sets.size(), sets.data(),
                                   room ? sids.data() : nullptr, room, smet.data(), svd.data()))
            return s;
        for (uint32_t m : smet) stotal += m;
    }
    for (size_t k = 0; k < gcs.size(); ++k) {
        nmet[gat[k]] = gmet[k];
        verdict[gat[k]] = gvd[k];
    }
    for (size_t k = 0; k < sets.size(); ++k) {
        nmet[sat[k]] = smet[k];
        verdict[sat[k]] = svd[k];
    }
    if (gtotal > cap || stotal > room || (gtotal + stotal && !ids)) return LASPJ_OK;
    uint64_t at = 0, sfrom = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (vars[i]->gc) {
            if (nmet[i]) laspj::gc_recheck_take(vars[i]->gc, ids + at);
        } else {
            for (uint32_t k = 0; k < nmet[i]; ++k) ids[at + k] = sids[sfrom + k];
            sfrom += nmet[i];
        }
        at += nmet[i];
    }
    return LASPJ_OK;
}

// one read of a read pass: a threshold image against the variable's value and — walk:
// reply_to_all's (lasp_core.erl:795-813) — against its lazy thresholds
struct ReadReq {
    laspj_var* var;
    const uint8_t* p;
    uint64_t len;
    int strict;
    bool walk;
};

// The device's half of read/6, read_any/3 and wait_needed/6 (lasp_core.erl:331-420,
// 730-758) over n reads of set variables of this context, S->mu held.  All n thresholds are
// decoded into fresh hidden variables of their variables' namespaces by the multi-operand
// write path (Op::WRITE, grouped by namespace as bind_many groups its payloads; unknown
// terms register and decode again as there; one run per kind named, since a pass decodes
// one kind), and k_read_check rides on the last run's passes behind the decode: one
// synchronisation when every term is known and the reads are of one kind.  verdict OK:
// hidden[i] holds threshold i's cells (the caller keeps it as a waiter's or a lazy entry's,
// or drops it) and ans[i] the met bytes of read i — the value's, then one per lazy entry
// when it walks.  verdict FALLBACK (a host-held value or lazy threshold, a threshold the
// namespace cannot represent): no hidden variable is left.
int read_pass(laspj_ctx* ctx, laspj::NifState* S, uint32_t n, const ReadReq* rq,
              std::vector<laspj_var*>* hidden, std::vector<std::vector<uint8_t>>* ans,
              int32_t* verdict) {
    using laspj::KindState;
    *verdict = LASPJ_NIF_FALLBACK;
    hidden->assign(n, nullptr);
    ans->assign(n, {});
    auto drop_all = [&] {
        for (laspj_var*& h : *hidden) {
            waiter_cells_drop(S, h);
            h = nullptr;
        }
    };
    auto fallback = [&] {
        drop_all();
        return laspj::fallback(S);
    };
    // every block of cells the check reads is of its namespace's current dictionary
    auto all_current = [&] {
        for (uint32_t i = 0; i < n; ++i) {
            if (!laspj::var_current(rq[i].var)) return false;
            if ((*hidden)[i] && !laspj::var_current((*hidden)[i])) return false;
            if (rq[i].walk)
                for (const laspj::Waiter& z : rq[i].var->lazy)
                    if (!laspj::var_current(z.cells)) return false;
        }
        return true;
    };
    for (uint32_t i = 0; i < n; ++i) {
        bool ok = false;
        if (int s = laspj::hydrate(ctx, S, rq[i].var, &ok)) return s;
        for (size_t k = 0; ok && rq[i].walk && k < rq[i].var->lazy.size(); ++k)
            if (int s = laspj::hydrate(ctx, S, rq[i].var->lazy[k].cells, &ok)) return s;
        if (!ok) return fallback();
    }
    // (a decode above may have started a namespace's dictionary afresh and written the
    // cells decoded before it out again: FALLBACK this once, as recheck_pass answers)
    if (!all_current()) return fallback();
    uint32_t ncs = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (int s = var_new(ctx, S, rq[i].var->kind, rq[i].var->ns, &(*hidden)[i])) {
            drop_all();
            return s;
        }
        ncs += 1 + (rq[i].walk ? (uint32_t)rq[i].var->lazy.size() : 0);
    }
    // pinned: [ReadDesc x n | ReadCur x ncs | met x ncs]; device: the records
    const uint64_t o_cs = 32ull * n, o_met = o_cs + 16ull * ncs, h_bytes = o_met + ncs;
    {
        laspj::Guard g(ctx);
        int s = laspj::grow_host(ctx, &S->rd_h, &S->rd_h_bytes, h_bytes);
        if (!s) s = laspj::grow_dev(ctx, &S->rd_d, &S->rd_d_bytes, laspj::read_rec_bytes(n, ncs));
        if (!s && S->rd_hkey != S->rd_h) {
            void* hd = nullptr;
            if (hipHostGetDevicePointer(&hd, S->rd_h, 0) != hipSuccess) {
                hipGetLastError();
                s = fail(ctx, LASPJ_E_DEVICE, "var_read: pinned block's device address");
            } else {
                S->rd_hd = static_cast<uint8_t*>(hd);
                S->rd_hkey = S->rd_h;
            }
        }
        if (s) {
            drop_all();
            return s;
        }
    }
    bool launched = false;          // the last pass enqueued the check
    std::vector<uint64_t> tiles(n);
    // behind a pass's write kernel, ctx->mu held (the hidden cells are fitted by the pass)
    auto tail = [&]() -> int {
        launched = false;
        if (!all_current()) return LASPJ_OK;      // (a reset inside the call: FALLBACK below)
        auto* hd = reinterpret_cast<laspj::ReadDesc*>(S->rd_h);
        auto* hc = reinterpret_cast<laspj::ReadCur*>(static_cast<uint8_t*>(S->rd_h) + o_cs);
        auto words = [](const laspj_var* c) {
            return c->cells ? (uint32_t)laspj::wpr_of(c->kind, c->E, c->tw) : 0u;
        };
        uint32_t c0 = 0;
        for (uint32_t i = 0; i < n; ++i) {
            laspj_var* v = rq[i].var;
            const KindState& K = *v->ns;
            const uint32_t tw = laspj::ktw(K);
            // the value over the namespace's element slots (new(): zeroed cells); a lazy
            // threshold's cells are re-laid only when the pairs per element changed (the
            // namespace went wide since): the slots it does not cover are absent
            if (K.E)
                if (int s = laspj::fit_var(ctx, v, K.E, tw)) return s;
            const laspj_var* t = (*hidden)[i];
            laspj::ReadDesc& d = hd[i];
            d.cells = t->cells;
            d.words = words(t);
            const uint32_t mode = v->kind == LASPJ_KIND_GSET ? laspj::kReadGset
                                  : tw > 1                   ? laspj::kReadWide
                                                             : laspj::kReadNarrow;
            d.mode_strict = mode << 1 | (rq[i].strict ? 1u : 0u);
            d.c0 = c0;
            uint64_t maxw = d.words;
            hc[c0] = laspj::ReadCur{v->cells, words(v), i};
            maxw = std::max<uint64_t>(maxw, hc[c0].words);
            uint32_t nc = 1;
            if (rq[i].walk)
                for (laspj::Waiter& z : v->lazy) {
                    laspj_var* c = z.cells;
                    if (c->cells && v->kind == LASPJ_KIND_ORSET && c->tw != tw)
                        if (int s = laspj::fit_var(ctx, c, K.E, tw)) return s;
                    hc[c0 + nc] = laspj::ReadCur{c->cells, words(c), i};
                    maxw = std::max<uint64_t>(maxw, hc[c0 + nc].words);
                    ++nc;
                }
            d.nc = nc;
            c0 += nc;
            tiles[i] = laspj::read_tiles(maxw);
        }
        const uint64_t items = laspj::read_lay_items(hd, n, tiles.data());
        LJ_HIP(ctx, laspj::launch_read_check(
                        ctx, reinterpret_cast<const laspj::ReadDesc*>(S->rd_hd), n,
                        reinterpret_cast<const laspj::ReadCur*>(S->rd_hd + o_cs), ncs, items,
                        static_cast<uint32_t*>(S->rd_d), S->rd_hd + o_met));
        launched = true;
        return LASPJ_OK;
    };
    // one run per kind named, each kind's payloads grouped by namespace
    std::vector<uint32_t> ord[2];
    for (uint32_t i = 0; i < n; ++i) ord[rq[i].var->kind == LASPJ_KIND_GSET ? 1 : 0].push_back(i);
    const int last = ord[1].empty() ? 0 : 1;
    for (int k = 0; k < 2; ++k) {
        std::vector<uint32_t>& o = ord[k];
        if (o.empty()) continue;
        std::stable_sort(o.begin(), o.end(), [&](uint32_t x, uint32_t y) {
            return std::less<const KindState*>()(rq[x].var->ns.get(), rq[y].var->ns.get());
        });
        laspj::Call c;
        c.op = laspj::Op::WRITE;
        c.kind = k ? LASPJ_KIND_GSET : LASPJ_KIND_ORSET;
        c.n = c.m = (uint32_t)o.size();
        for (uint32_t a = 0; a < o.size(); ++a) {
            const ReadReq& r = rq[o[a]];
            c.p.push_back(r.p);
            c.len.push_back(r.len);
            c.vars.push_back((*hidden)[o[a]]);
            if (a == 0 || rq[o[a - 1]].var->ns != r.var->ns)
                c.groups.push_back(laspj::Group{r.var->ns.get(), a, a + 1});
            else
                c.groups.back().p1 = a + 1;
        }
        if (k == last) c.tail = tail;
        std::vector<int32_t> vd;
        if (int s = laspj::run(ctx, S, c, &vd)) {
            drop_all();
            return s;
        }
        for (int32_t x : vd)
            if (x != LASPJ_NIF_OK) {
                drop_all();                       // (run counted the FALLBACKs)
                return LASPJ_OK;
            }
    }
    if (!launched || !all_current()) return fallback();
    const uint8_t* met = static_cast<const uint8_t*>(S->rd_h) + o_met;
    uint32_t c0 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t nc = 1 + (rq[i].walk ? (uint32_t)rq[i].var->lazy.size() : 0);
        (*ans)[i].assign(met + c0, met + c0 + nc);
        c0 += nc;
        (*hidden)[i]->image.clear();              // (a reset inside the call wrote cells out)
    }
    *verdict = LASPJ_NIF_OK;
    return LASPJ_OK;
}

// read_any/3's fold (lasp_core.erl:372-414) over set variables of this context, S->mu held
// (laspj_var_read is the fold over one pair)
int read_any_locked(laspj_ctx* ctx, laspj::NifState* S, uint32_t n, laspj_var* const* vars,
                    const uint8_t* const* thresholds, const uint64_t* lens, const int32_t* strict,
                    uint64_t id, int32_t* found, uint64_t* lazy_ids, uint32_t cap,
                    uint32_t* nlazy, int32_t* verdict) {
    *found = -1;
    for (uint32_t i = 0; i < n; ++i) nlazy[i] = 0;
    std::vector<ReadReq> rq(n);
    // the variables named, densely numbered (one may be named again)
    std::vector<laspj_var*> uniq;
    std::vector<uint32_t> var_of(n);
    for (uint32_t i = 0; i < n; ++i) {
        rq[i] = ReadReq{vars[i], thresholds[i], lens[i], strict[i] ? 1 : 0, true};
        const auto it = std::find(uniq.begin(), uniq.end(), vars[i]);
        var_of[i] = (uint32_t)(it - uniq.begin());
        if (it == uniq.end()) uniq.push_back(vars[i]);
    }
    std::vector<laspj_var*> hidden;
    std::vector<std::vector<uint8_t>> ans;
    if (int s = read_pass(ctx, S, n, rq.data(), &hidden, &ans, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    auto drop_hidden = [&] {
        for (laspj_var*& h : hidden) {
            waiter_cells_drop(S, h);
            h = nullptr;
        }
    };
    const int s = laspj::nomem_guard(ctx, "var_read", [&] {
        std::vector<uint32_t> nl(uniq.size());
        for (size_t v = 0; v < uniq.size(); ++v) nl[v] = (uint32_t)uniq[v]->lazy.size();
        std::vector<const uint8_t*> ap(n);
        for (uint32_t i = 0; i < n; ++i) ap[i] = ans[i].data();
        laspj::ReadFold f;
        laspj::read_fold(n, var_of.data(), (uint32_t)uniq.size(), nl.data(), ap.data(), &f);
        *found = f.found;
        for (uint32_t i = 0; i < n; ++i) nlazy[i] = (uint32_t)f.fired[i].size();
        if (f.total > cap || (f.total && !lazy_ids)) {
            drop_hidden();                        // nothing is changed or registered
            return LASPJ_OK;
        }
        // the waiters built before anything is touched (an allocation may fail)
        std::vector<laspj::Waiter> ws(n);
        for (uint32_t i = 0; i < n; ++i) {
            if (!f.blocked[i]) continue;
            ws[i].id = id;
            ws[i].strict = rq[i].strict;
            ws[i].image.assign(rq[i].p, rq[i].p + rq[i].len);
            vars[i]->waiters.reserve(vars[i]->waiters.size() + n);
        }
        uint64_t at = 0;
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j : f.fired[i]) lazy_ids[at++] = vars[i]->lazy[j].id;
        for (uint32_t i = 0; i < n; ++i) {
            if (!f.blocked[i]) continue;
            ws[i].cells = hidden[i];
            hidden[i] = nullptr;
            vars[i]->waiters.push_back(std::move(ws[i]));
        }
        drop_hidden();                            // the met read's, and those after it
        for (size_t v = 0; v < uniq.size(); ++v) {
            std::vector<laspj::Waiter>& lz = uniq[v]->lazy;
            if (f.still[v].size() == lz.size()) continue;
            size_t keep = 0, k = 0;
            for (size_t j = 0; j < lz.size(); ++j) {
                if (k < f.still[v].size() && f.still[v][k] == j) {
                    if (keep != j) lz[keep] = std::move(lz[j]);
                    ++keep;
                    ++k;
                } else {
                    waiter_cells_drop(S, lz[j].cells);
                }
            }
            lz.resize(keep);
        }
        return LASPJ_OK;
    });
    if (s) drop_hidden();
    return s;
}

// A variable's waiting or lazy threads: the calls that differ only in the list they name.
using Threads = std::vector<laspj::Waiter> laspj_var::*;

// an entry appended to a list (an allocation may throw: nothing is appended then)
int thread_append(std::vector<laspj::Waiter>* list, uint64_t id, int strict, const uint8_t* p,
                  uint64_t n, laspj_var* cells) {
    laspj::Waiter w;
    w.id = id;
    w.strict = strict ? 1 : 0;
    w.image.assign(p, p + n);
    w.cells = cells;
    list->push_back(std::move(w));
    return LASPJ_OK;
}

// laspj_var_wait_cancel / _lazy_cancel: the entry `id` names, its hidden cells dropped, erased
int thread_cancel(laspj_var* var, Threads list, const char* name, uint64_t id, int32_t* found) {
    const laspj::Entry e = laspj::enter_var(var, name, found != nullptr);
    if (e.rc) return e.rc;
    *found = 0;
    std::vector<laspj::Waiter>& ts = var->*list;
    for (size_t k = 0; k < ts.size(); ++k)
        if (ts[k].id == id) {
            waiter_cells_drop(e.S, ts[k].cells);
            ts.erase(ts.begin() + (ptrdiff_t)k);
            *found = 1;
            break;
        }
    return LASPJ_OK;
}

// laspj_var_waiter_count / _lazy_count (no membership test, no error text)
int thread_count(const laspj_var* var, Threads list, uint32_t* n) {
    laspj::NifState* S = var_state(const_cast<laspj_var*>(var));
    if (!S || !n) return LASPJ_E_INVAL;
    std::lock_guard<std::mutex> lk(S->mu);
    *n = (uint32_t)(var->*list).size();
    return LASPJ_OK;
}

// laspj_var_waiter_at / _lazy_at (no membership test): entry k of the list; strict may be null
int thread_at(laspj_var* var, Threads list, const char* name, const char* what, uint32_t k,
              bool args_ok, uint64_t* id, int32_t* strict, const uint8_t** threshold, uint64_t* n) {
    const laspj::Entry e = laspj::enter(var_state(var), var ? var->ctx : nullptr, name, args_ok);
    if (e.rc) return e.rc;
    const std::vector<laspj::Waiter>& ts = var->*list;
    if (k >= ts.size()) return fail(e.ctx, LASPJ_E_RANGE, "%s: no %s %u", name, what, k);
    *id = ts[k].id;
    if (strict) *strict = ts[k].strict;
    *threshold = ts[k].image.data();
    *n = ts[k].image.size();
    return LASPJ_OK;
}

}  // namespace

extern "C" {

int laspj_var_wait(laspj_var* var, const uint8_t* threshold, uint64_t n, int strict, uint64_t id,
                   int32_t* met, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_wait(var->gc, threshold, n, strict, id, met, verdict);
    const laspj::Entry e = laspj::enter_var(var, "var_wait", (threshold || !n) && met && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    bool ok = false;
    if (int s = laspj::hydrate(ctx, S, var, &ok)) return s;
    *met = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    if (!ok) return laspj::fallback(S);
    // threshold_met(Type, Value, Threshold) (lasp_lattice.erl:62-75) as
    // laspj_var_etf_threshold answers it; the pass registers the threshold's terms
    {
        laspj::Call c = laspj::var_call(laspj::Op::THRESHOLD, var, threshold, n, strict ? 1 : 0);
        std::vector<int32_t> vd;
        if (int s = laspj::run(ctx, S, c, &vd)) return s;
        if (vd[0] != LASPJ_NIF_OK) return LASPJ_OK;
        if (c.res[0]) {
            *met = 1;
            *verdict = LASPJ_NIF_OK;
            return LASPJ_OK;
        }
    }
    // unmet (lasp_core.erl:355-364): appended to waiting_threads, its threshold decoded
    // into a hidden variable of this namespace (its terms are known now: one more pass)
    laspj_var* cells = nullptr;
    if (int s = var_new(ctx, S, var->kind, var->ns, &cells)) return s;
    int32_t wv = LASPJ_NIF_FALLBACK;
    int s = var_write_locked(ctx, S, cells, threshold, n, &wv);
    if (s == LASPJ_OK && wv == LASPJ_NIF_OK) {
        s = laspj::nomem_guard(ctx, "var_wait", [&] {
            return thread_append(&var->waiters, id, strict, threshold, n, cells);
        });
        if (s == LASPJ_OK) {
            *verdict = LASPJ_NIF_OK;
            return LASPJ_OK;
        }
    }
    waiter_cells_drop(S, cells);
    return s;
}

int laspj_var_recheck(laspj_var* var, uint64_t* ids, uint32_t cap, uint32_t* nmet,
                      uint32_t* nwaiting, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_recheck(var->gc, ids, cap, nmet, nwaiting, verdict);
    const laspj::Entry e =
        laspj::enter_var(var, "var_recheck", (ids || !cap) && nmet && nwaiting && verdict);
    if (e.rc) return e.rc;
    *nmet = 0;
    const int s = recheck_locked(e.ctx, e.S, 1, &var, ids, cap, nmet, verdict);
    *nwaiting = (uint32_t)var->waiters.size();
    return s;
}

int laspj_var_recheck_many(laspj_ctx* ctx, uint32_t n, laspj_var* const* vars, uint64_t* ids,
                           uint32_t cap, uint32_t* nmet, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!n) return LASPJ_OK;
    if (!vars || (!ids && cap) || !nmet || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_recheck: null array");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    if (kinds_of(n, vars) & 2) return recheck_mixed(ctx, S, n, vars, ids, cap, nmet, verdict);
    std::unordered_set<laspj_var*> seen;
    for (uint32_t i = 0; i < n; ++i) {
        if (!vars[i] || vars[i]->ctx != ctx || !S->vars.count(vars[i]))
            return fail(ctx, LASPJ_E_INVAL, "var_recheck: variable %u is not this context's", i);
        if (!seen.insert(vars[i]).second)
            return fail(ctx, LASPJ_E_INVAL, "var_recheck: variable %u named twice", i);
    }
    return recheck_locked(ctx, S, n, vars, ids, cap, nmet, verdict);
}

int laspj_var_wait_cancel(laspj_var* var, uint64_t id, int32_t* found) {
    if (var && var->gc) return laspj::gc_wait_cancel(var->gc, id, found);
    return thread_cancel(var, &laspj_var::waiters, "var_wait_cancel", id, found);
}

int laspj_var_waiter_count(const laspj_var* var, uint32_t* n) {
    if (var && var->gc) return laspj::gc_waiter_count(var->gc, n);
    return thread_count(var, &laspj_var::waiters, n);
}

int laspj_var_waiter_at(laspj_var* var, uint32_t k, uint64_t* id, int32_t* strict,
                        const uint8_t** threshold, uint64_t* n) {
    if (var && var->gc) return laspj::gc_waiter_at(var->gc, k, id, strict, threshold, n);
    return thread_at(var, &laspj_var::waiters, "var_waiter_at", "waiter", k,
                     id && strict && threshold && n, id, strict, threshold, n);
}

int laspj_var_wait_needed(laspj_var* var, const uint8_t* threshold, uint64_t n, int strict,
                          uint64_t id, int32_t* needed, int32_t* verdict) {
    if (var && var->gc) {
        // the entry's threshold is a number, which reply_to_all hands to
        // riak_dt_gcounter:value/1 as a value (lasp_core.erl:798) and crashes there
        if (!needed || !verdict) return LASPJ_E_INVAL;
        *needed = 0;
        return laspj::gc_refuse(var->gc, verdict);
    }
    const laspj::Entry e =
        laspj::enter_var(var, "var_wait_needed", (threshold || !n) && needed && verdict);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    laspj_ctx* ctx = e.ctx;
    *needed = 0;
    const ReadReq rq{var, threshold, n, strict ? 1 : 0, false};
    std::vector<laspj_var*> hidden;
    std::vector<std::vector<uint8_t>> ans;
    if (int s = read_pass(ctx, S, 1, &rq, &hidden, &ans, verdict)) return s;
    if (*verdict != LASPJ_NIF_OK) return LASPJ_OK;
    if (ans[0][0] || !var->waiters.empty()) {
        // met, or somebody is already reading (lasp_core.erl:736-741): ReplyFun(Threshold)
        waiter_cells_drop(S, hidden[0]);
        *needed = 1;
        return LASPJ_OK;
    }
    int s = LASPJ_OK;
    if (strict) {
        // the entry would hold {strict, T}, which reply_to_all hands to is_inflation as a
        // value (:798): the reference's clause, and its crash, on the NIF side
        *verdict = LASPJ_NIF_FALLBACK;
        laspj::fallback(S);
    } else {
        s = laspj::nomem_guard(ctx, "var_wait_needed", [&] {
            return thread_append(&var->lazy, id, 0, threshold, n, hidden[0]);
        });
        if (s == LASPJ_OK) return LASPJ_OK;
    }
    waiter_cells_drop(S, hidden[0]);
    return s;
}

int laspj_var_read(laspj_var* var, const uint8_t* threshold, uint64_t n, int strict, uint64_t id,
                   int32_t* met, uint64_t* lazy_ids, uint32_t cap, uint32_t* nlazy,
                   uint32_t* nstill_lazy, int32_t* verdict) {
    if (var && var->gc) {
        // laspj_var_wait remains the counter's read
        if (!met || !nlazy || !nstill_lazy || !verdict) return LASPJ_E_INVAL;
        *met = 0;
        *nlazy = *nstill_lazy = 0;
        return laspj::gc_refuse(var->gc, verdict);
    }
    const laspj::Entry e = laspj::enter_var(
        var, "var_read",
        (threshold || !n) && met && (lazy_ids || !cap) && nlazy && nstill_lazy && verdict);
    if (e.rc) return e.rc;
    const int32_t st = strict ? 1 : 0;
    int32_t found = -1;
    const int s = read_any_locked(e.ctx, e.S, 1, &var, &threshold, &n, &st, id, &found, lazy_ids,
                                  cap, nlazy, verdict);
    *met = found == 0 ? 1 : 0;
    *nstill_lazy = (uint32_t)var->lazy.size();
    return s;
}

int laspj_var_read_any(laspj_ctx* ctx, uint32_t n, laspj_var* const* vars,
                       const uint8_t* const* thresholds, const uint64_t* lens,
                       const int32_t* strict, uint64_t id, int32_t* found, uint64_t* lazy_ids,
                       uint32_t cap, uint32_t* nlazy, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!found || !verdict) return fail(ctx, LASPJ_E_INVAL, "var_read_any: null argument");
    *found = -1;
    *verdict = LASPJ_NIF_OK;
    if (!n) return LASPJ_OK;                      // lists:foldl over []: not_available_yet
    if (!vars || !thresholds || !lens || !strict || (!lazy_ids && cap) || !nlazy)
        return fail(ctx, LASPJ_E_INVAL, "var_read_any: null array");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    bool counter = false;
    for (uint32_t i = 0; i < n; ++i) {
        nlazy[i] = 0;
        if (vars[i] && vars[i]->gc) {
            if (laspj::gc_var_ctx(vars[i]->gc) != ctx)
                return fail(ctx, LASPJ_E_INVAL, "var_read_any: variable %u is not this context's", i);
            counter = true;
            continue;
        }
        if (!vars[i] || vars[i]->ctx != ctx || !S->vars.count(vars[i]))
            return fail(ctx, LASPJ_E_INVAL, "var_read_any: variable %u is not this context's", i);
        if (!thresholds[i] && lens[i])
            return fail(ctx, LASPJ_E_INVAL, "var_read_any: null threshold");
    }
    if (counter) {
        *verdict = LASPJ_NIF_FALLBACK;
        return laspj::fallback(S);
    }
    return read_any_locked(ctx, S, n, vars, thresholds, lens, strict, id, found, lazy_ids, cap,
                           nlazy, verdict);
}

int laspj_var_lazy_count(const laspj_var* var, uint32_t* n) {
    if (var && var->gc) {
        if (!n) return LASPJ_E_INVAL;
        *n = 0;
        return LASPJ_OK;
    }
    return thread_count(var, &laspj_var::lazy, n);
}

int laspj_var_lazy_at(laspj_var* var, uint32_t k, uint64_t* id, const uint8_t** threshold,
                      uint64_t* n) {
    if (var && var->gc) return LASPJ_E_RANGE;     // a counter keeps none
    return thread_at(var, &laspj_var::lazy, "var_lazy_at", "lazy thread", k, id && threshold && n,
                     id, nullptr, threshold, n);
}

int laspj_var_lazy_cancel(laspj_var* var, uint64_t id, int32_t* found) {
    if (var && var->gc) {
        if (!found) return LASPJ_E_INVAL;
        *found = 0;
        return LASPJ_OK;
    }
    return thread_cancel(var, &laspj_var::lazy, "var_lazy_cancel", id, found);
}

}  // extern "C"
