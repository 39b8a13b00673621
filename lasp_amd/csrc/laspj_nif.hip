// NIF-level entry points (include/laspj.h "NIF entry points", "device-resident variables"):
// what a `laspj_nif` NIF function does between `enif_term_to_binary` and
// `enif_binary_to_term`, inside liblaspj so that it is compiled, tested and timed here
// rather than living as a listing.
//
// The reference's drop-in point is `Type:merge/2` and friends (lasp_orset.erl:32-36,
// 67-73, 128-138; lasp_gset.erl:39-43, 74-76, 99-105), called from lasp_core:bind/3
// (lasp_core.erl:291-312) on many BEAM schedulers at once (lasp_vnode.erl:213-237).
//
// Image calls (laspj_{orset,gset}_etf_*) take the operands as `term_to_binary/1` images and
//   1. stage them into the context's pinned memory; kernels on the context's stream pull
//      them to the device in pieces while the host stages the next (offsets and the
//      decoder's segment table ride along),
//   2. decode them on the device against the context's dictionary of that kind
//      (laspj_orset_etf_read's / laspj_gset_etf_read's kernels), join / test the cells,
//      encode the answer on the device straight into pinned memory — all enqueued on the
//      context's stream with ONE host synchronisation,
//   3. answer from pinned memory: the merged / value term's image (what the NIF hands to
//      enif_binary_to_term) or the boolean.
// Variable calls (laspj_var_*) keep `#dv.value` (include/lasp.hrl:60-63) on the device
// between calls: bind/3 ships only the incoming `Value`, decodes it, and one kernel decides
// `Value0 =:= Value`, joins it into the resident cells and answers the status; the value
// is encoded only when it is read.
//
// A token the dictionary has not seen (another node's unique/1) on a known element is
// taken by the decoder in the same pass when it is a binary of the namespace's token
// length (NewTok: the element's next free slot, registered after the pass; a merge's
// answer is then written by a second, write-only launch once the images know it).  Any
// other unseen term makes the decoder answer UNKNOWN_TERM: the call registers the
// operands' terms in the host dictionary (only the elements of the decoder segments that
// failed, when it decoded in segments; else the whole operands, laspj_dict_add), patches
// or rebuilds the device images and decodes again (only the failed segments, when it can).
// An element past 64 tokens widens its namespace (cells of k {p, r} pairs, the wide codec)
// — image calls start a fresh dictionary first.  An operand the columnar form does not
// take — not an orddict of {Elem, [{Token, Bool}]} (an ordset for G-Sets) in term order,
// an element with no tokens, a term `==` to a registered one under another image, a term
// kind no dictionary holds — gets verdict LASPJ_NIF_FALLBACK: the NIF then runs the
// reference's own Erlang clause, so the caller always gets the reference's answer (or its
// crash).  Scratch, dictionaries and staging are per context: one context per scheduler
// (or per vnode), or one per GPU with the binds of many schedulers committed in groups;
// no process globals.
//
// This file holds the passes (the planner, the phases of device_pass, run and its
// registration loop), the image calls and the context's state.  The calls on handles are in
// laspj_nif_vars.hip (resident variables: lifecycle, bind queue, write, read, union, update),
// laspj_nif_waiters.hip (waiting and lazy threads, the one-pass reads), laspj_nif_process.hip
// (filter processes, the G-Set intersection) and laspj_nif_lvars.hip (list-valued
// variables); what they share is in laspj_nif_internal.h.

#include "laspj_nif_internal.h"

namespace laspj {

namespace {

// The in region pulled from pinned host memory by a kernel on the context's stream: the
// decoder then starts right behind it instead of waiting for a copy engine's completion
// signal.  16-byte lanes, grid-stride.
typedef uint32_t pull16 __attribute__((ext_vector_type(4)));
__global__ void __launch_bounds__(256) k_nif_pull(const pull16* __restrict__ src,
                                                  pull16* __restrict__ dst, uint64_t n16) {
    // a wave moves 4 KiB per step: four 1 KiB loads in flight per instruction group
    const uint64_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nw = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave; c * 256 < n16; c += nw) {
        pull16 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = c * 256 + k * 64 + lane;
            if (i < n16) v[k] = __builtin_nontemporal_load(src + i);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint64_t i = c * 256 + k * 64 + lane;
            if (i < n16) dst[i] = v[k];
        }
    }
}

// Payloads gathered into the in region at their (byte) offsets from pinned blocks: those
// group-commit waiters staged themselves, and the leader's own (copied into the staging
// at its offset).  8-byte lanes, four loads in flight per lane (2 KiB per wave step), a
// dst word composed of two source words (the neighbour lane's) when source and
// destination differ in alignment, partial words at a payload's ends written byte by
// byte (a neighbouring payload owns their other bytes).  blockIdx.y: the payload.
struct GatherDesc {
    const uint8_t* src;             // any alignment; readable 16 bytes past len
    uint64_t dst, len;              // offset in the region, bytes
};
constexpr uint32_t kGatherMax = 16;
constexpr uint32_t kGatherU = 4;
struct GatherArgs {
    GatherDesc d[kGatherMax];
};
__global__ void __launch_bounds__(256) k_nif_gather(GatherArgs g, uint8_t* __restrict__ dst) {
    const GatherDesc ds = g.d[blockIdx.y];
    const uint64_t d0 = ds.dst, d1 = ds.dst + ds.len;
    if (d1 == d0) return;
    const uint64_t w0 = d0 & ~7ull;
    const uint32_t sh = (uint32_t)(d0 - w0);
    const uint64_t nw = (d1 - w0 + 7) / 8;             // dst words touched
    const uint64_t sa = reinterpret_cast<uint64_t>(ds.src);
    const uint64_t* src = reinterpret_cast<const uint64_t*>(sa & ~7ull);
    // dst byte w0 + 8j + b is source word j's byte b + delta (of the aligned source)
    const int32_t delta = (int32_t)(sa & 7ull) - (int32_t)sh;
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwv = ((uint64_t)gridDim.x * blockDim.x) >> 6;
    for (uint64_t c = wave * 64 * kGatherU; c < nw; c += nwv * 64 * kGatherU) {
        uint64_t cur[kGatherU], edge[kGatherU];
#pragma unroll
        for (uint32_t u = 0; u < kGatherU; ++u) {
            const uint64_t j = c + 64 * u + lane;
            cur[u] = j < nw ? __builtin_nontemporal_load(src + j) : 0ull;
            // the one neighbour word no lane of this group loads
            edge[u] = 0;
            if (j < nw && delta < 0 && lane == 0 && j > 0) edge[u] = __builtin_nontemporal_load(src + j - 1);
            if (j < nw && delta > 0 && (lane == 63 || j + 1 == nw))
                edge[u] = __builtin_nontemporal_load(src + j + 1);
        }
#pragma unroll
        for (uint32_t u = 0; u < kGatherU; ++u) {
            const uint64_t up = __shfl_up(cur[u], 1, 64), dn = __shfl_down(cur[u], 1, 64);
            const uint64_t j = c + 64 * u + lane;
            if (j >= nw) continue;
            const uint64_t w = w0 + 8 * j;
            if (w >= d0 && w + 8 <= d1) {
                uint64_t v = cur[u];
                if (delta < 0) {
                    const uint64_t pv = lane ? up : edge[u];
                    v = (pv >> (8 * (8 + delta))) | (cur[u] << (8 * -delta));
                } else if (delta > 0) {
                    const uint64_t nx = (lane == 63 || j + 1 == nw) ? edge[u] : dn;
                    v = (cur[u] >> (8 * delta)) | (nx << (8 * (8 - delta)));
                }
                *reinterpret_cast<uint64_t*>(dst + w) = v;
            } else {
                for (uint32_t b = 0; b < 8; ++b)
                    if (w + b >= d0 && w + b < d1) dst[w + b] = ds.src[w + b - d0];
            }
        }
    }
}

constexpr uint32_t kMaxDictElements = 1u << 20;   // a larger dictionary is reset
// a wide namespace (an element past 64 tokens): token slots per element, and the token
// image length its fixed-width templates hold
constexpr uint32_t kWideTokens = 1024, kWideTokenLen = 46;
// new tokens a single bind's decoder may take (NewTok entries; more: the two-pass path)
constexpr uint32_t kNewTokCap = 512;
// device passes per call: registration, a grown answer area and a serial re-decode each
// take one; a call still unresolved after this many answers FALLBACK (run's post-condition)
constexpr int kMaxPasses = 6;
// the in region is pulled by kernels in pieces of this many bytes: each piece's pull runs
// while the host stages the next (one copy-engine copy per call measured slower, and
// 512 KiB copy pieces hit a slow runtime path: profiles/r04i_nif_ab.log,
// r04pull_block_size_ab.log)
constexpr uint64_t kPullPiece = 512ull << 10;

// the group payload i belongs to
size_t group_of(const Call& c, uint32_t i) {
    size_t g = 0;
    while (g + 1 < c.groups.size() && i >= c.groups[g].p1) ++g;
    return g;
}

KindState& kstate(NifState* S, int32_t kind) {
    return S->ks[kind == LASPJ_KIND_GSET ? 1 : 0];
}

void free_etf(KindState& K) {
    if (K.etf) laspj_etf_dict_destroy(K.etf);
    K.etf = nullptr;
    if (K.wd) wide_dict_destroy(K.wd);
    K.wd = nullptr;
    K.E = 0;
}

// the device images of the dictionary (called without ctx->mu: etf_dict_create takes it)
// a wide namespace's tables (called as rebuild_etf): every element exactly (no headroom:
// any registration rebuilds — the wide path is the rare one), pairs per cell grown to hold
// the widest element; LASPJ_E_UNSUPPORTED: token images of several lengths
int rebuild_wide(laspj_ctx* ctx, NifState* S, KindState& K) {
    const uint64_t t0 = now_ns();
    WideExport x;
    if (int s = dict_export_wide(K.dict, &x)) return fail(ctx, s, "nif: wide export");
    const uint32_t n = (uint32_t)x.eorder.size();
    if (!n) return LASPJ_E_UNSUPPORTED;
    const uint32_t tw = std::max(K.tw, std::max(2u, (x.max_cnt + 63u) / 64u));
    WideDict* wd = nullptr;
    if (int s = wide_dict_create(ctx, x, tw, &wd)) return s;
    laspj_etf_dict* g = nullptr;
    if (int s = laspj_etf_dict_create(ctx, n, x.eblob.data(), x.eoff.data(), x.eorder.data(),
                                      nullptr, nullptr, nullptr, &g)) {
        wide_dict_destroy(wd);
        return s;
    }
    free_etf(K);
    K.wd = wd;
    K.etf = g;
    K.E = n;
    K.tw = tw;
    K.stale = false;
    K.built_K = n;
    {
        std::vector<uint32_t> gone;
        dict_take_dirty(K.dict, &gone);
    }
    ++S->stats[ST_REBUILDS];
    S->stats[ST_NS_IMAGES] += now_ns() - t0;
    return LASPJ_OK;
}

}  // namespace

int grow_dev(laspj_ctx* ctx, void** p, uint64_t* have, uint64_t need) {
    if (*have >= need) return LASPJ_OK;
    const uint64_t want = std::max<uint64_t>(need, *have + *have / 2);
    if (*p) {
        hipStreamSynchronize(ctx->stream);
        hipFree(*p);
        *p = nullptr;
        *have = 0;
    }
    if (dev_malloc(ctx, p, want) != hipSuccess) {
        hipGetLastError();
        *p = nullptr;
        return fail(ctx, LASPJ_E_NOMEM, "nif: device allocation of %llu bytes",
                    (unsigned long long)want);
    }
    *have = want;
    return LASPJ_OK;
}

int grow_host(laspj_ctx* ctx, void** p, uint64_t* have, uint64_t need) {
    if (*have >= need) return LASPJ_OK;
    const uint64_t want = std::max<uint64_t>(need, *have + *have / 2);
    if (*p) {
        hipStreamSynchronize(ctx->stream);
        hipHostFree(*p);
        *p = nullptr;
        *have = 0;
    }
    // coherent: kernels read the staging and write the answers themselves, and a device
    // L2 line of last call's operands must not outlive the host's rewrite
    if (hipHostMalloc(p, want, hipHostMallocCoherent) != hipSuccess) {
        hipGetLastError();
        *p = nullptr;
        return fail(ctx, LASPJ_E_NOMEM, "nif: pinned allocation of %llu bytes",
                    (unsigned long long)want);
    }
    *have = want;
    return LASPJ_OK;
}

// the namespace takes elements of more than 64 tokens from now on (its cells widen on
// their next use; slots are unchanged, so nothing is written out)
// (false: the namespace stays narrow — its token images are not of one length, which the
// wide templates need)
bool go_wide(NifState* S, KindState& K) {
    if (K.wide) return true;
    if (K.kind != LASPJ_KIND_ORSET || !K.dict) return false;
    // token ids 64 e + k name 64 slots per element: the namespace's list variables are
    // written out to their images first and stay host-held while it is wide
    if (spill_lvars(S, K) != LASPJ_OK) return false;
    if (!dict_set_tok_cap(K.dict, kWideTokens, kWideTokenLen)) return false;
    K.wide = true;
    K.stale = true;
    ++S->stats[ST_WIDENED];
    return true;
}

int rebuild_etf(laspj_ctx* ctx, NifState* S, KindState& K) {
    if (K.wide && dict_elements(K.dict) == 0) {
        // (every registration that widened it was refused: narrow again)
        dict_set_tok_cap(K.dict, 64, 0);
        K.wide = false;
        K.tw = 1;
    }
    if (K.wide) return rebuild_wide(ctx, S, K);
    const uint64_t t0 = now_ns();
    uint32_t n = 0;
    uint64_t eb = 0, tb = 0;
    if (laspj_dict_info(K.dict, &n, &eb, &tb) != LASPJ_OK)
        return fail(ctx, LASPJ_E_INVAL, "nif: dictionary info");
    // head-room: registrations are append-only, so a larger E holds the next terms
    uint32_t E = K.E;
    if (!K.etf || n > E) E = n + n / 4 + 64;
    const bool toks = K.kind == LASPJ_KIND_ORSET;
    // (the context's arrays, grown only: the export writes every entry it hands on)
    auto fit = [](auto& v, uint64_t n) {
        if (v.size() < n) v.resize(n + n / 4);
        return v.data();
    };
    uint8_t* ebl = fit(S->x_ebl, eb + 1);
    uint8_t* tbl = fit(S->x_tbl, toks ? tb + 1 : 1);
    uint8_t* tord = fit(S->x_tord, toks ? 64ull * E : 1);
    uint32_t* eoff = fit(S->x_eoff, E + 1ull);
    uint32_t* eord = fit(S->x_eord, E);
    uint32_t* toff = fit(S->x_toff, toks ? 64ull * E + 1 : 1);
    if (laspj_dict_export(K.dict, E, ebl, eoff, eord, toks ? tbl : nullptr,
                          toks ? toff : nullptr, toks ? tord : nullptr) != LASPJ_OK)
        return fail(ctx, LASPJ_E_INVAL, "nif: dictionary export");
    free_etf(K);
    laspj_etf_dict* d = nullptr;
    // OR-Sets: two tokens of headroom per element, so a call that only adds tokens to
    // known elements patches the images (patch_etf) instead of coming back here
    if (int s = toks ? etf_dict_create_ex(ctx, E, ebl, eoff, eord, tbl, toff, tord, 2, &d)
                     : laspj_etf_dict_create(ctx, E, ebl, eoff, eord, nullptr, nullptr,
                                             nullptr, &d))
        return s;
    K.etf = d;
    K.E = E;
    K.stale = false;
    K.built_K = n;
    {
        std::vector<uint32_t> gone;
        dict_take_dirty(K.dict, &gone);             // (the rebuild holds every token)
    }
    K.built_cnt.resize(n);
    K.built_toks = 0;
    for (uint32_t e = 0; e < n; ++e)
        K.built_toks += K.built_cnt[e] = toks ? dict_token_count(K.dict, e) : 0;
    K.rank_full = true;                             // (the order tables follow the images)
    K.rank_dirty.clear();
    for (laspj_map* m : K.maps) m->tok_all = true;  // (any element may have gained tokens)
    for (laspj_fold* f : K.folds) f->tok_all = true;
    ++S->stats[ST_REBUILDS];
    S->stats[ST_NS_IMAGES] += now_ns() - t0;
    return LASPJ_OK;
}

// Registrations that only added tokens to elements the images already hold: their rows
// patched in place.  False: rebuild (new elements, an element past its headroom, ...).
bool patch_etf(laspj_ctx* ctx, NifState* S, KindState& K) {
    if (!K.etf || K.kind != LASPJ_KIND_ORSET || K.wide) return false;
    const uint64_t t0 = now_ns();
    const uint32_t n = dict_elements(K.dict);
    if (n != K.built_K || n > K.E) return false;
    // the slots the dictionary saw gain tokens (no scan over every element)
    std::vector<uint32_t> seen, dirty;
    dict_take_dirty(K.dict, &seen);
    std::sort(seen.begin(), seen.end());
    seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
    for (uint32_t e : seen)
        if (e < n && dict_token_count(K.dict, e) != K.built_cnt[e]) dirty.push_back(e);
    if (!dirty.empty() &&
        etf_dict_patch(ctx, K.etf, K.dict, dirty.data(), (uint32_t)dirty.size()) != LASPJ_OK)
        return false;
    for (uint32_t e : dirty) {
        const uint32_t cnt = dict_token_count(K.dict, e);
        K.built_toks += cnt - K.built_cnt[e];
        K.built_cnt[e] = cnt;
    }
    if (!K.lvars.empty() && !K.rank_full)
        K.rank_dirty.insert(K.rank_dirty.end(), dirty.begin(), dirty.end());
    for (laspj_map* m : K.maps)
        if (!m->tok_all) m->tok_dirty.insert(m->tok_dirty.end(), dirty.begin(), dirty.end());
    for (laspj_fold* f : K.folds)
        if (!f->tok_all) f->tok_dirty.insert(f->tok_dirty.end(), dirty.begin(), dirty.end());
    K.stale = false;
    ++S->stats[ST_PATCHES];
    S->stats[ST_NS_IMAGES] += now_ns() - t0;
    return true;
}

void release_cells(laspj_ctx* ctx, laspj_var* v) {
    if (v->cells) dev_release(ctx, v->cells, v->cell_bytes);
    v->cells = nullptr;
    v->cell_bytes = 0;
    v->E = 0;
    v->tw = 1;
}

// a variable's cells widened to the dictionary's E (slots are append-only: the old cells
// stay where they are, the new slots start absent); call with ctx->mu held
int fit_var(laspj_ctx* ctx, laspj_var* v, uint32_t E, uint32_t tw) {
    if (v->cells && v->E == E && v->tw == tw) return LASPJ_OK;
    const uint64_t wnew = wpr_of(v->kind, E, tw), wold = v->cells ? wpr_of(v->kind, v->E, v->tw) : 0;
    const uint64_t bytes = std::max<uint64_t>(8ull * wnew, 256);
    void* p = nullptr;
    if (dev_alloc(ctx, bytes, &p) != hipSuccess) {
        hipGetLastError();
        return fail(ctx, LASPJ_E_NOMEM, "nif: variable cells (%llu bytes)",
                    (unsigned long long)bytes);
    }
    uint64_t* c = static_cast<uint64_t*>(p);
    if (v->kind == LASPJ_KIND_ORSET && (tw != 1 || (v->cells && v->tw != 1))) {
        // pairs per element change (a namespace gone wide): re-laid, slot for slot
        LJ_HIP(ctx, launch_relay(ctx, c, v->cells, v->cells ? v->E : 0, v->cells ? v->tw : 1, E, tw));
    } else {
        const uint64_t keep = std::min(wold, wnew);
        if (keep) LJ_HIP(ctx, hipMemcpyAsync(c, v->cells, 8ull * keep, hipMemcpyDeviceToDevice,
                                             ctx->stream));
        if (wnew > keep)
            LJ_HIP(ctx, hipMemsetAsync(c + keep, 0, 8ull * (wnew - keep), ctx->stream));
    }
    release_cells(ctx, v);
    v->cells = c;
    v->cell_bytes = bytes;
    v->E = E;
    v->tw = tw;
    return LASPJ_OK;
}

// The pinned staging grown to the two regions, and its device addresses (looked up once per
// allocation: the runtime's lookup costs host microseconds).  Call with ctx->mu held.
int fit_staging(laspj_ctx* ctx, NifState* S, uint64_t in_bytes, uint64_t out_bytes) {
    if (int s = grow_host(ctx, &S->hin, &S->hin_bytes, in_bytes)) return s;
    if (int s = grow_host(ctx, &S->hout, &S->hout_bytes, out_bytes)) return s;
    void* hd = nullptr;
    if (S->hin_dkey != S->hin) {
        LJ_HIP(ctx, hipHostGetDevicePointer(&hd, S->hin, 0));
        S->hin_d = static_cast<uint8_t*>(hd);
        S->hin_dkey = S->hin;
    }
    if (S->hout_dkey != S->hout) {
        LJ_HIP(ctx, hipHostGetDevicePointer(&hd, S->hout, 0));
        S->hout_d = static_cast<uint8_t*>(hd);
        S->hout_dkey = S->hout;
    }
    return LASPJ_OK;
}

namespace {

// device_pass's answer when the writer found the answer area short: nothing was written, the
// area has been grown (S->ocap) and run() takes the pass again
constexpr int kPassAgain = -1000;

// What one device pass does: decided once, from the call and its dictionaries' state.
struct PassPlan {
    bool orset = false;
    bool wide = false;              // (single-group ops: answers by the wide codec)
    bool dec = false;               // the device decodes the operands (else the host encodes cells)
    bool var_op = false;            // BIND / WRITE: a kernel joins into resident cells
    bool var_in = false;            // the call reads resident cells
    bool any_wide = false;
    bool multi = false;             // several namespaces' payloads in one decode launch
    bool has_payload_out = false;   // the answer is an image (MERGE / VALUE / READ / VVALUE)
    bool defer = false;             // the chain check rides on the answer's launch (ChainJob)
    bool nt_merge = false, nt_on = false;   // the decoder takes unseen tokens (NewTok)
    bool gathered = false;          // payloads staged by group-commit waiters: k_nif_gather
    std::vector<unsigned long long> hoffs;  // m + 1: the payloads laid end to end
    uint64_t pay = 0;                       // their bytes
    std::vector<EtfGroup> eg;               // per group (cells: PassMem's copy)
    std::vector<EtfReadPlan> plans;         // one over every payload (multi), else per group
};

PassPlan plan_pass(const laspj_ctx* ctx, const Call& c) {
    PassPlan P;
    const uint32_t m = c.m, n = c.n;
    const size_t G = c.groups.size();
    // single-group ops (every op but BIND / WRITE) answer over group 0's dictionary
    const KindState& K = *c.groups[0].K;
    const uint32_t E = K.E;
    P.orset = c.kind == LASPJ_KIND_ORSET;
    P.wide = P.orset && K.wide;
    P.dec = m != 0;
    // (a wide namespace's operands are encoded by the host dictionary: dict_encode_cells)
    for (const Group& g : c.groups)
        if (P.orset && g.p1 > g.p0 && (g.K->wide || !etf_dict_decodable(g.K->etf))) P.dec = false;
    P.var_op = c.op == Op::BIND || c.op == Op::WRITE;
    P.var_in = P.var_op || c.op == Op::THRESHOLD || c.op == Op::READ || c.op == Op::VVALUE;
    P.hoffs.assign(m + 1ull, 0);
    for (uint32_t i = 0; i < m; ++i) P.hoffs[i + 1] = P.hoffs[i] + c.len[i];
    P.pay = P.hoffs[m];
    P.eg.resize(G);
    for (size_t g = 0; g < G; ++g) {
        const Group& gr = c.groups[g];
        P.eg[g] = EtfGroup{gr.K->etf, gr.p0, gr.p1, nullptr, gr.K->E};
        P.any_wide |= P.orset && gr.K->wide;
    }
    // several namespaces' OR-Set payloads: one decode launch over all of them (a table of
    // the dictionaries rides in the in region) with one plan, else group by group, each
    // with its own plan and segment table
    P.multi = G > 1 && P.dec && P.orset && !P.any_wide &&
              etf_multi_fill(ctx, P.eg.data(), (uint32_t)G, m, nullptr);
    P.plans.resize(P.multi ? 1 : G);
    for (size_t g = 0; g < P.plans.size(); ++g) {
        const Group& gr = c.groups[g];
        const uint32_t p0 = P.multi ? 0 : gr.p0, R = P.multi ? m : gr.p1 - gr.p0;
        if (P.dec && P.orset && R && !gr.K->wide)
            etf_read_plan(ctx, gr.K->etf, R, P.hoffs.data() + p0, &P.plans[g]);
    }
    P.has_payload_out = c.op == Op::MERGE || c.op == Op::VALUE || c.op == Op::READ ||
                        c.op == Op::VVALUE;
    // MERGE: the segment decoder's chain check rides on the join's launch (ChainJob), its
    // per-segment results in a device area of their own after the in region
    // (one plan only: the join / bind launch carries one chain check)
    P.defer = (G == 1 || P.multi) && P.dec && P.orset && P.plans[0].nseg && !c.no_defer &&
              !c.write_only &&
              ((c.op == Op::MERGE && etf_merge_fused(ctx, n, E)) || P.var_op ||
               (c.op == Op::VALUE && etf_value_direct(ctx, n, E)));
    // one operand over binary tokens (a bind, write/4, a threshold, value/1 — no answer
    // carries token images): tokens the namespace has not seen are taken by the decoder
    // (NewTok entries into the answer area, registered by run())
    P.nt_merge = c.op == Op::MERGE && n == 1 && m == 2 && etf_merge_write_one(ctx, K.etf, n, E);
    P.nt_on = (((P.var_op || c.op == Op::THRESHOLD || c.op == Op::VALUE) && m == 1) ||
               P.nt_merge) &&
              G == 1 && P.orset && !K.wide && P.dec && !c.redo.n && !c.write_only &&
              !c.no_newtok && etf_dict_bin_tokens(K.etf);
    // a group commit's waiters staged their payloads into pinned blocks of their own while
    // they waited: gathered to their offsets by the device (k_nif_gather), launched before
    // the host builds the rest of the pass
    P.gathered = P.dec && !c.redo.n && !c.write_only &&
                 std::any_of(c.pre.begin(), c.pre.end(),
                             [](const uint8_t* x) { return x != nullptr; });
    return P;
}

// Where everything of a pass lies: byte offsets into the four blocks of NifState.
//
//   in region — staged in S->hin (pinned), pulled to the head of S->dblk:
//     i_offs   m + 1 payload offsets (u64)
//     i_seg    the decoders' segment tables, plan g's at gseg[g]
//     i_zero   z_bytes of words the kernels expect zero (and leave zero or do not reuse):
//                z_ticket  the size pass's / one-launch merge's ticket
//                z_redo    segment mode's redo lists: group g's R + 1 words at word p0 + g
//                z_lb      the one-launch merge's look-back words, one u64 per 256 elements
//                z_var     the variable kernel's n difference words, then its ticket
//                z_nt      the decoders' new-token counter
//     i_vptr   (BIND / WRITE) n pointers to the variables' cells, n to their decoded
//              operands' cells, n widths in words
//     i_mtab   (multi) the decode table of several dictionaries
//     i_pay    the payloads end to end (+ 64 bytes the decoders may read past), or the
//              host-encoded operand cells
//   the device block's tail, after the in region (device only):
//     d_seg    a deferred decode's segment results (kSegResBytes each)
//     d_vst    (BIND / WRITE) the decode statuses their kernel reads
//   out region — S->hout (pinned), written by the kernels in place:
//     o_st     m decode statuses          o_res   n answer bytes
//     o_ooff   n + 1 answer offsets       o_seg   a failed payload's segment results
//     o_nt     kNewTokCap NewTok entries  o_pay   ocap bytes of answer payloads
//   cells — S->dcells: group g's operand cells at word gcell[g] (its payloads' replicas at
//   its own width), then at byte c_out the answer's cells (MERGE) or value words
struct PassLayout {
    uint64_t i_offs = 0, i_seg = 0, i_zero = 0, i_vptr = 0, i_mtab = 0, i_pay = 0, in_bytes = 0;
    std::vector<uint64_t> gseg;
    uint64_t z_ticket = 0, z_redo = 4, z_lb = 0, z_var = 0, z_nt = 0, z_bytes = 0;
    uint64_t d_seg = 0, seg_bytes = 0, d_vst = 0, dblk_bytes = 0;
    uint64_t o_st = 0, o_res = 0, o_ooff = 0, o_seg = 0, o_nt = 0, o_pay = 0, ocap = 0,
             out_bytes = 0;
    std::vector<uint64_t> gcell;
    uint64_t W = 0;                 // words per replica (single-group ops)
    uint64_t in_words = 0, cells_in = 0, c_out = 0, dcells_bytes = 0;
};

// (grows S->ocap to the call's bound: the one thing it decides beyond offsets)
PassLayout layout_pass(NifState* S, const Call& c, const PassPlan& P) {
    PassLayout L;
    const uint32_t m = c.m, n = c.n;
    const size_t G = c.groups.size();
    const KindState& K = *c.groups[0].K;
    const uint32_t E = K.E;
    uint64_t seg_area = 0;
    L.gseg.assign(G, 0);
    L.gcell.assign(G, 0);
    for (size_t g = 0; g < G; ++g) {
        const Group& gr = c.groups[g];
        L.gcell[g] = L.in_words;
        L.in_words += (uint64_t)(gr.p1 - gr.p0) * wpr_of(c.kind, gr.K->E, ktw(*gr.K));
    }
    for (size_t g = 0; g < P.plans.size(); ++g) {
        const uint32_t R = P.multi ? m : c.groups[g].p1 - c.groups[g].p0;
        L.gseg[g] = seg_area;
        if (P.plans[g].nseg) seg_area += al(4ull * (R + 1), 16);
    }
    L.W = wpr_of(c.kind, E, ktw(K));
    L.cells_in = L.in_words * 8ull;
    L.i_seg = al(8ull * (m + 1), 256);
    L.i_zero = L.i_seg + al(seg_area, 256);
    L.z_lb = al(4ull * (m + G + 2), 16);
    L.z_var = L.z_lb + 8ull * ((E + 255) / 256);
    L.z_nt = L.z_var + 4ull * (n + 1);
    L.z_bytes = L.z_nt + 4;
    L.i_vptr = L.i_zero + al(L.z_bytes, 256);
    L.i_mtab = L.i_vptr + (P.var_op ? al(24ull * n, 256) : 0);
    L.i_pay = L.i_mtab + (P.multi ? al(etf_multi_bytes((uint32_t)G, m), 256) : 0);
    L.in_bytes = L.i_pay + (P.dec ? al(P.pay + 64, 256) : al(L.cells_in, 256));
    L.d_seg = al(L.in_bytes, 256);
    L.seg_bytes = P.defer ? al(P.plans[0].nseg * kSegResBytes, 256) : 0;
    L.d_vst = L.d_seg + L.seg_bytes;
    L.dblk_bytes = L.d_vst + (P.var_op ? al(4ull * m, 256) : 0);
    // answer payload bound: a merge's image is at most both operands' (flags may be
    // re-encoded one byte longer than a SMALL_ATOM_UTF8 input: the slack, and a second
    // pass when even that is short); value/1's at most its operand's; a variable's image
    // is bounded by nothing the call knows (a second pass when the area is short)
    uint64_t bound = 64ull * n + 64;
    for (uint32_t i = 0; i < m; ++i) bound += c.len[i];
    if (P.has_payload_out && S->ocap < bound + bound / 8)
        S->ocap = al(bound + bound / 8, 1 << 16);
    L.ocap = P.has_payload_out ? S->ocap : 0;
    L.o_res = al(4ull * m, 16);
    L.o_ooff = L.o_res + al(n, 16);
    L.o_seg = L.o_ooff + al(8ull * (n + 1), 16);
    // (a failed payload's results, written by its chain check)
    L.o_nt = L.o_seg + L.seg_bytes;
    L.o_pay = L.o_nt + (P.nt_on ? al(sizeof(NewTok) * kNewTokCap, 256) : 0);
    L.out_bytes = L.o_pay + L.ocap;
    // cells: in batch m x W words; MERGE: answers n x W; VALUE / VVALUE: value words
    const uint64_t VW = (E + 63ull) / 64ull;
    const uint64_t cells_out = c.op == Op::MERGE ? (uint64_t)n * L.W * 8ull
                               : (c.op == Op::VALUE || c.op == Op::VVALUE) ? (uint64_t)n * VW * 8ull
                                                                            : 0;
    L.c_out = al(L.cells_in, 256);
    L.dcells_bytes = L.c_out + cells_out + 256;
    return L;
}

// the four blocks' addresses once they are fitted to a layout
struct PassMem {
    uint8_t* hin = nullptr;             // in region: pinned host address,
    const uint8_t* hin_d = nullptr;     //   the same bytes as the device sees them,
    uint8_t* din = nullptr;             //   and their device copy (S->dblk)
    const uint8_t* hout = nullptr;      // out region: as the host reads it,
    uint8_t* rout = nullptr;            //   as the kernels write it
    uint64_t *cin = nullptr, *cout = nullptr;   // operand cells, answer cells
    std::vector<EtfGroup> eg;           // the plan's groups, their cells' addresses filled in
};

int fit_pass(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
             PassMem* M) {
    Guard g(ctx);
    if (int s = grow_dev(ctx, &S->dblk, &S->dblk_bytes, L.dblk_bytes)) return s;
    const uint64_t had = S->dcells_bytes;
    if (int s = grow_dev(ctx, &S->dcells, &S->dcells_bytes, L.dcells_bytes)) return s;
    if (S->dcells_bytes != had) S->clean_words = 0;
    if (int s = fit_staging(ctx, S, L.in_bytes, L.out_bytes)) return s;
    if (P.var_in)
        for (laspj_var* v : c.vars)
            if (int s = fit_var(ctx, v, v->ns->E, v->ns->wide ? v->ns->tw : 1)) return s;
    M->hin = static_cast<uint8_t*>(S->hin);
    M->hin_d = S->hin_d;
    M->din = static_cast<uint8_t*>(S->dblk);
    M->hout = static_cast<const uint8_t*>(S->hout);
    M->rout = S->hout_d;
    M->cin = static_cast<uint64_t*>(S->dcells);
    M->cout = reinterpret_cast<uint64_t*>(static_cast<uint8_t*>(S->dcells) + L.c_out);
    M->eg = P.eg;
    for (size_t k = 0; k < M->eg.size(); ++k) M->eg[k].cells = M->cin + L.gcell[k];
    return LASPJ_OK;
}

// payloads for k_nif_gather, launched kGatherMax at a time (call with ctx->mu held)
struct Gatherer {
    laspj_ctx* ctx;
    uint8_t* dst;                   // the payload area on the device
    GatherArgs ga{};
    uint32_t ng = 0;
    uint64_t most = 0;
    int flush() {
        if (!ng) return LASPJ_OK;
        // (one wave step of 2 KiB per wave, 8 KiB per block)
        const uint64_t blocks = std::min<uint64_t>((most + 8191) / 8192, (uint64_t)ctx->cus);
        hipLaunchKernelGGL(k_nif_gather, dim3((unsigned)std::max<uint64_t>(blocks, 1), ng),
                           dim3(256), 0, ctx->stream, ga, dst);
        LJ_LAUNCHED(ctx);
        ng = 0;
        most = 0;
        return LASPJ_OK;
    }
    int add(const uint8_t* src, uint64_t at, uint64_t len) {
        ga.d[ng++] = GatherDesc{src, at, len};
        most = std::max(most, len);
        return ng == kGatherMax ? flush() : LASPJ_OK;
    }
};

// The host's half of staging, outside ctx->mu (group-commit waiters keep queueing behind a
// pass that builds its head): the payloads the waiters staged themselves set off first,
// then the head written into the pinned in region and, when the device cannot decode the
// operands, their cells encoded by the host dictionaries (*hst: their statuses).
int stage_operands(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                   const PassMem& M, std::vector<int32_t>* hst) {
    const uint32_t m = c.m, n = c.n;
    const size_t G = c.groups.size();
    if (P.gathered) {
        Guard g(ctx);
        Gatherer ga{ctx, M.din + L.i_pay};
        for (uint32_t i = 0; i < m; ++i)
            if (c.len[i] && c.pre[i])
                if (int s = ga.add(c.pre[i], P.hoffs[i], c.len[i])) return s;
        if (int s = ga.flush()) return s;
    }
    std::memcpy(M.hin + L.i_offs, P.hoffs.data(), 8ull * (m + 1));
    for (size_t g = 0; g < P.plans.size(); ++g)
        if (P.plans[g].nseg)
            std::memcpy(M.hin + L.i_seg + L.gseg[g], P.plans[g].segbase.data(),
                        4ull * P.plans[g].segbase.size());
    if (P.multi) etf_multi_fill(ctx, M.eg.data(), (uint32_t)G, m, M.hin + L.i_mtab);
    std::memset(M.hin + L.i_zero, 0, L.z_bytes);
    if (P.var_op) {
        // per variable: its cells, its decoded operand's cells, their width
        for (size_t g = 0; g < G; ++g) {
            const Group& gr = c.groups[g];
            const uint64_t w = wpr_of(c.kind, gr.K->E, ktw(*gr.K));
            for (uint32_t i = gr.p0; i < gr.p1; ++i) {
                const uint64_t cur = reinterpret_cast<uint64_t>(c.vars[i]->cells);
                const uint64_t in = reinterpret_cast<uint64_t>(
                    M.cin + L.gcell[g] + (uint64_t)(i - gr.p0) * w);
                std::memcpy(M.hin + L.i_vptr + 8ull * i, &cur, 8);
                std::memcpy(M.hin + L.i_vptr + 8ull * (n + i), &in, 8);
                std::memcpy(M.hin + L.i_vptr + 8ull * (2ull * n + i), &w, 8);
            }
        }
    }
    if (m && !P.dec) {
        // token images of several lengths (or no tokens yet): the host dictionaries encode
        // the cells (laspj_dict_encode), the device does the rest
        std::vector<uint8_t> blob(P.pay);
        for (uint32_t i = 0; i < m; ++i)
            if (c.len[i]) std::memcpy(blob.data() + P.hoffs[i], c.p[i], c.len[i]);
        hst->assign(m, 0);
        for (size_t g = 0; g < G; ++g) {
            const Group& gr = c.groups[g];
            if (gr.p1 == gr.p0) continue;
            if (int s = dict_encode_cells(gr.K->dict, c.kind, blob.data(),
                                          reinterpret_cast<const uint64_t*>(P.hoffs.data()) + gr.p0,
                                          gr.p1 - gr.p0, -1, gr.K->E, ktw(*gr.K),
                                          reinterpret_cast<uint64_t*>(M.hin + L.i_pay) + L.gcell[g],
                                          hst->data() + gr.p0))
                return fail(ctx, s, "nif: host encode failed (%d)", s);
        }
        ++S->stats[ST_HOST_ENCODED];
    }
    return LASPJ_OK;
}

// The device's half (ctx->mu held): the head, then the payloads (or host-encoded cells) a
// piece at a time — each piece's pull runs while the host stages the next.  *t_copy: the
// host nanoseconds spent copying operands into pinned memory.
int pull_operands(laspj_ctx* ctx, Call& c, const PassPlan& P, const PassLayout& L,
                  const PassMem& M, uint64_t* t_copy) {
    const uint32_t m = c.m;
    uint64_t sent = 0;                   // region bytes already pulled
    auto send = [&](uint64_t upto) -> int {
        // 16-byte lanes: sent is a multiple of 16 (the head is 256-aligned, pieces
        // 4096-multiples), upto is rounded up inside the staged region
        const uint64_t n16 = (al(upto, 16) - sent) / 16;
        if (!n16) return LASPJ_OK;
        const uint64_t blocks = std::min<uint64_t>((n16 + 255) / 256, (uint64_t)ctx->cus * 4);
        hipLaunchKernelGGL(k_nif_pull, dim3((unsigned)std::max<uint64_t>(blocks, 1)), dim3(256), 0,
                           ctx->stream, reinterpret_cast<const pull16*>(M.hin_d + sent),
                           reinterpret_cast<pull16*>(M.din + sent), n16);
        LJ_LAUNCHED(ctx);
        sent = al(upto, 16);
        return LASPJ_OK;
    };
    if (P.dec && (c.redo.n || c.write_only)) {
        // (a redo or write-only pass: the head and payloads the last pass pulled are
        // still there)
    } else if (P.gathered) {
        // the head, then the payloads not staged by their callers (the leader's own)
        // copied into the staging and gathered to their offsets (the staged ones are
        // on their way since the region was allocated)
        if (int s = send(L.i_pay)) return s;
        Gatherer ga{ctx, M.din + L.i_pay};
        for (uint32_t i = 0; i < m; ++i) {
            if (!c.len[i] || c.pre[i]) continue;
            const uint64_t tc = now_ns();
            std::memcpy(M.hin + L.i_pay + P.hoffs[i], c.p[i], c.len[i]);
            *t_copy += now_ns() - tc;
            if (int s = ga.add(M.hin_d + L.i_pay + P.hoffs[i], P.hoffs[i], c.len[i])) return s;
        }
        if (int s = ga.flush()) return s;
    } else if (P.dec) {
        uint64_t at = 0;
        uint32_t i = 0;
        uint64_t io = 0;                     // offset inside payload i
        while (i < m && c.len[i] == 0) ++i;
        while (at < P.pay) {
            const uint64_t piece = std::min(kPullPiece, P.pay - at);
            uint64_t done = 0;
            const uint64_t tc = now_ns();
            while (done < piece) {
                const uint64_t take = std::min(piece - done, c.len[i] - io);
                std::memcpy(M.hin + L.i_pay + at + done, c.p[i] + io, take);
                done += take;
                io += take;
                if (io == c.len[i]) {
                    ++i;
                    io = 0;
                    while (i < m && c.len[i] == 0) ++i;
                }
            }
            *t_copy += now_ns() - tc;
            at += piece;
            if (int s = send(L.i_pay + at)) return s;
        }
        if (P.pay == 0)
            if (int s = send(L.i_pay)) return s;
    } else {
        // the head and (when there are operands) the host-encoded cells
        if (int s = send(L.i_pay)) return s;
        if (m) LJ_HIP(ctx, hipMemcpyAsync(M.cin, M.hin + L.i_pay, L.cells_in,
                                          hipMemcpyHostToDevice, ctx->stream));
    }
    return LASPJ_OK;
}

// where the decoders (or the host) leave the m decode statuses: straight in the pinned
// answer, or (variable calls) device memory their kernel reads and publishes
int32_t* status_area(const PassPlan& P, const PassLayout& L, const PassMem& M) {
    return reinterpret_cast<int32_t*>(P.var_op ? M.din + L.d_vst : M.rout + L.o_st);
}

// The operands' cells: decoded by the device — every namespace's payloads in one launch, or
// group by group — or, host-encoded, only their statuses uploaded for the variable kernel.
// *cjob: armed when the chain check is left to the answer's launch.
int enqueue_decode(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                   const PassMem& M, const std::vector<int32_t>& hst, ChainJob* cjob) {
    const uint32_t m = c.m;
    const size_t G = c.groups.size();
    const bool clean = S->clean_words >= L.in_words;
    int32_t* dst = status_area(P, L, M);
    const auto* doffs_all = reinterpret_cast<const unsigned long long*>(M.din + L.i_offs);
    if (P.defer) {
        cjob->res = M.din + L.d_seg;
        cjob->hres = M.rout + L.o_seg;
    }
    if (c.write_only) {
        // (the operands' cells the last pass decoded are still there)
    } else if (P.dec && P.multi) {
        // every namespace's payloads in one launch (the cells zeroed first when the last
        // call left them dirty: the decoders only set what they decode)
        const EtfReadPlan& plan = P.plans[0];
        if (!clean && !c.redo.n) LJ_HIP(ctx, hipMemsetAsync(M.cin, 0, L.cells_in, ctx->stream));
        if (int s = etf_read_multi_enqueue(
                ctx, M.eg.data(), (uint32_t)G, M.din + L.i_mtab, m, M.din + L.i_pay, P.pay,
                doffs_all, plan,
                plan.nseg ? reinterpret_cast<const uint32_t*>(M.din + L.i_seg) : nullptr, dst,
                P.defer ? cjob : nullptr, c.redo.n ? &c.redo : nullptr))
            return s;
    } else if (P.dec) {
        // each group's payloads against its own dictionary (offsets are absolute in the
        // payload area, so a group reads its slice of them in place)
        for (size_t g = 0; g < G; ++g) {
            const Group& gr = c.groups[g];
            const uint32_t R = gr.p1 - gr.p0;
            if (!R) continue;
            laspj_batch gb = view(ctx, c.kind, R, gr.K->E, M.cin + L.gcell[g]);
            const auto* doffs = doffs_all + gr.p0;
            NewTokArgs nta;
            if (P.nt_on) {
                if (!++S->nt_seq) ++S->nt_seq;           // (0 never tags an entry)
                nta = NewTokArgs{reinterpret_cast<uint32_t*>(M.din + L.i_zero + L.z_nt),
                                 reinterpret_cast<NewTok*>(M.rout + L.o_nt), kNewTokCap,
                                 S->nt_seq};
            }
            if (P.orset) {
                const EtfReadPlan& plan = P.plans[g];
                if (int s = etf_read_enqueue(
                        ctx, &gb, gr.K->etf, -1, 1, M.din + L.i_pay, P.pay, doffs, plan,
                        plan.nseg ? reinterpret_cast<const uint32_t*>(M.din + L.i_seg + L.gseg[g])
                                  : nullptr,
                        dst + gr.p0, !clean && !c.redo.n,
                        reinterpret_cast<uint32_t*>(M.din + L.i_zero + L.z_redo) + gr.p0 + g,
                        P.defer ? cjob : nullptr, c.redo.n ? &c.redo : nullptr,
                        P.nt_on ? &nta : nullptr))
                    return s;
            } else if (int s = gset_read_enqueue(ctx, &gb, gr.K->etf, -1, 1, M.din + L.i_pay,
                                                 doffs, dst + gr.p0, !clean,
                                                 P.hoffs.data() + gr.p0)) {
                return s;
            }
        }
    } else if (m && P.var_op) {
        LJ_HIP(ctx, hipMemcpyAsync(dst, hst.data(), 4ull * m, hipMemcpyHostToDevice, ctx->stream));
    }
    return LASPJ_OK;
}

// what every answer's enqueue works on: the single-group call's dictionary and the views of
// its operand cells, the answer's offsets and payload area in the pinned out region
struct AnswerArgs {
    KindState& K;
    uint32_t E, TW;
    laspj_batch lhs, rhs;           // operands [0, n) and [n, 2n)
    unsigned long long* dooff;
    uint8_t* dopay;
    uint8_t* dres;                  // n answer bytes
};

// an answer's images from its cells: the size pass, then the writer over its offsets
int size_and_write(laspj_ctx* ctx, const laspj_batch* b, int32_t kind, const AnswerArgs& a,
                   uint64_t ocap) {
    const unsigned long long* chunks = nullptr;
    if (int s = etf_size_enqueue(ctx, b, a.K.etf, kind, -1, a.dooff, ctx->flag, &chunks)) return s;
    return etf_write_enqueue(ctx, b, a.K.etf, kind, -1, 1, a.dooff, a.dopay, ocap, chunks);
}

// the same over a wide namespace's cells
int wide_size_and_write(laspj_ctx* ctx, uint64_t* cells, uint32_t n, const AnswerArgs& a,
                        uint64_t ocap) {
    if (int s = wide_size_enqueue(ctx, a.K.wd, cells, n, -1, a.dooff, ctx->flag)) return s;
    return wide_write_enqueue(ctx, a.K.wd, cells, n, -1, 1, a.dooff, a.dopay, ocap);
}

// lasp_orset:merge/2 (lasp_orset.erl:128-134): the nested orddict:merge of two canonical
// orddicts is the slot-wise OR of their cells; lasp_gset:merge/2 (lasp_gset.erl:99-101):
// ordsets:union of two ordsets, the OR of their bits
int answer_merge(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                 const PassMem& M, const AnswerArgs& a, const ChainJob* cjob) {
    const uint32_t n = c.n;
    laspj_batch ob = view(ctx, c.kind, n, a.E, M.cout, a.TW);
    uint8_t* dzero = M.din + L.i_zero;
    uint32_t* dticket = reinterpret_cast<uint32_t*>(dzero + L.z_ticket);
    if (P.wide) {
        // elements past 64 tokens: the OR, then the wide size pass and writer
        LJ_HIP(ctx, launch_or(ctx, M.cout, a.lhs.dev, a.rhs.dev, (uint64_t)n * L.W));
        if (int s = wide_size_and_write(ctx, M.cout, n, a, L.ocap)) return s;
        S->clean_words = 0;
        return LASPJ_OK;
    }
    if (P.orset && etf_merge_write_one(ctx, a.K.etf, n, a.E)) {
        // one answer: join, size pass and writer in one launch (look-back), the
        // operands cleared behind it, the chain checks riding along
        if (int s = etf_merge_write_enqueue(
                ctx, a.lhs.dev, a.rhs.dev, a.E, a.K.etf, -1, 1, a.dooff, a.dopay, L.ocap,
                reinterpret_cast<unsigned long long*>(dzero + L.z_lb), dticket, cjob,
                P.nt_on ? reinterpret_cast<const uint32_t*>(dzero + L.z_nt) : nullptr))
            return s;
        S->clean_words = L.in_words;
        return LASPJ_OK;
    }
    if (!P.orset && etf_value_direct(ctx, n, a.E)) {
        // few long G-Set answers: written from both operands' bits
        if (int s = etf_gset_merge_write_enqueue(ctx, &a.lhs, &a.rhs, a.K.etf, -1, 1, a.dooff,
                                                 ctx->flag, a.dopay, L.ocap))
            return s;
        S->clean_words = 0;
        return LASPJ_OK;
    }
    if (P.orset && etf_merge_fused(ctx, n, a.E)) {
        // the OR fused with the answer's size pass, the operands cleared behind it
        const unsigned long long* chunks = nullptr;
        if (int s = etf_merge_size_enqueue(ctx, a.lhs.dev, a.rhs.dev, &ob, a.K.etf, -1, a.dooff,
                                           ctx->flag, dticket, &chunks, cjob))
            return s;
        S->clean_words = L.in_words;
        return etf_write_enqueue(ctx, &ob, a.K.etf, c.kind, -1, 1, a.dooff, a.dopay, L.ocap,
                                 chunks);
    }
    LJ_HIP(ctx, launch_or(ctx, M.cout, a.lhs.dev, a.rhs.dev, (uint64_t)n * L.W));
    S->clean_words = 0;
    return size_and_write(ctx, &ob, c.kind, a, L.ocap);
}

// value/1 (lasp_orset.erl:67-73): the elements with a {_, false} token, as the ordset image
// the G-Set writer gives a bit row (term_to_binary of the keys)
// (VVALUE has no operand cells: its value bits land where they would start)
int answer_value(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                 const PassMem& M, const AnswerArgs& a, const ChainJob* cjob) {
    const uint32_t n = c.n;
    laspj_batch src = c.op == Op::VALUE ? view(ctx, c.kind, c.m, a.E, M.cin, a.TW)
                                        : view(ctx, c.kind, 1, a.E, c.vars[0]->cells, a.TW);
    if (!P.wide && P.orset && etf_value_direct(ctx, n, a.E)) {
        // few long answers: written from the cells (no value bits in between), a
        // decoded operand's cells cleared behind the reads
        if (int s = etf_value_write_enqueue(ctx, &src, a.K.etf, -1, 1, a.dooff, ctx->flag, a.dopay,
                                            L.ocap, c.op == Op::VALUE, cjob))
            return s;
        S->clean_words = c.op == Op::VALUE ? L.in_words : S->clean_words;
        return LASPJ_OK;
    }
    // the value bits of the (wide) cells, then the G-Set writer over the element images
    S->clean_words = 0;
    LJ_HIP(ctx, P.wide ? launch_wide_value(ctx, &src, M.cout, false)
                       : launch_orset_value(ctx, &src, M.cout, false));
    laspj_batch vb = view(ctx, LASPJ_KIND_GSET, n, a.E, M.cout);
    return size_and_write(ctx, &vb, LASPJ_KIND_GSET, a, L.ocap);
}

// the variable's value as its term_to_binary image (#dv.value read back)
int answer_read(laspj_ctx* ctx, Call& c, const PassPlan& P, const PassLayout& L, const AnswerArgs& a) {
    laspj_batch vb = view(ctx, c.kind, 1, a.E, c.vars[0]->cells, a.TW);
    if (P.wide) return wide_size_and_write(ctx, vb.dev, 1, a, L.ocap);
    return size_and_write(ctx, &vb, c.kind, a, L.ocap);
}

// is_inflation / is_strict_inflation (lasp_lattice.erl:137-161, 212-253) of prev -> cur
hipError_t launch_inflation(laspj_ctx* ctx, const PassPlan& P, const laspj_batch* prev,
                            const laspj_batch* cur, bool strict, uint8_t* out) {
    return P.wide    ? launch_wide_inflation(ctx, prev, cur, strict, out)
           : P.orset ? launch_orset_inflation(ctx, prev, cur, strict, out)
                     : launch_gset_inflation(ctx, prev, cur, strict, out);
}

int answer_compare(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const AnswerArgs& a) {
    S->clean_words = 0;
    if (c.op == Op::EQUAL) {
        // equal/2 (lasp_orset.erl:136-138, lasp_gset.erl:103-105): A == B
        LJ_HIP(ctx, launch_equal(ctx, &a.lhs, &a.rhs, a.dres));
    } else if (c.op == Op::INFLATION) {
        LJ_HIP(ctx, launch_inflation(ctx, P, &a.lhs, &a.rhs, c.strict != 0, a.dres));
    } else {
        // threshold_met(Type, Value, Threshold) (lasp_lattice.erl:62-75): is_(strict_)
        // inflation(Threshold, Value) with Value the resident cells
        laspj_batch cur = view(ctx, c.kind, 1, a.E, c.vars[0]->cells, a.TW);
        LJ_HIP(ctx, launch_inflation(ctx, P, &a.lhs, &cur, c.strict != 0, a.dres));
    }
    return LASPJ_OK;
}

// bind/3 (lasp_core.erl:291-312) / write/4 (:839-844) into the resident cells (the segment
// decoder's chain check rides on this launch when deferred)
int answer_bind(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                const PassMem& M, const AnswerArgs& a, const ChainJob* cjob) {
    const uint32_t n = c.n;
    uint64_t maxw = 0;                                // widest variable (the bind's chunks)
    for (const Group& gr : c.groups) maxw = std::max(maxw, wpr_of(c.kind, gr.K->E, ktw(*gr.K)));
    uint32_t* dvdiff = reinterpret_cast<uint32_t*>(M.din + L.i_zero + L.z_var);
    if (int s = var_bind_enqueue(ctx, reinterpret_cast<uint64_t* const*>(M.din + L.i_vptr),
                                 reinterpret_cast<uint64_t* const*>(M.din + L.i_vptr + 8ull * n),
                                 reinterpret_cast<const uint64_t*>(M.din + L.i_vptr + 16ull * n),
                                 maxw, n, status_area(P, L, M), dvdiff, dvdiff + n, a.dres,
                                 reinterpret_cast<int32_t*>(M.rout + L.o_st), c.op == Op::WRITE,
                                 cjob))
        return s;
    S->clean_words = L.in_words;
    return LASPJ_OK;
}

// The op's answer over the decoded cells, written by the kernels into the pinned out region.
int enqueue_answer(laspj_ctx* ctx, NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                   const PassMem& M, const ChainJob* cjob) {
    KindState& K = *c.groups[0].K;
    const uint32_t E = K.E, TW = ktw(K);
    AnswerArgs a{K, E, TW, view(ctx, c.kind, c.n, E, M.cin, TW),
                 view(ctx, c.kind, c.n, E, M.cin + (uint64_t)c.n * L.W, TW),
                 reinterpret_cast<unsigned long long*>(M.rout + L.o_ooff), M.rout + L.o_pay,
                 M.rout + L.o_res};
    switch (c.op) {
    case Op::MERGE: return answer_merge(ctx, S, c, P, L, M, a, cjob);
    case Op::VALUE:
    case Op::VVALUE: return answer_value(ctx, S, c, P, L, M, a, cjob);
    case Op::READ: return answer_read(ctx, c, P, L, a);
    case Op::EQUAL:
    case Op::INFLATION:
    case Op::THRESHOLD: return answer_compare(ctx, S, c, P, a);
    case Op::BIND:
    case Op::WRITE: return answer_bind(ctx, S, c, P, L, M, a, cjob);
    }
    return LASPJ_OK;
}

// After the synchronise: statuses, new tokens, a deferred pass's segment results and the
// answers read from the pinned out region into the call.  kPassAgain: the answer area was
// short (it has been grown).
int collect_answers(NifState* S, Call& c, const PassPlan& P, const PassLayout& L,
                    const PassMem& M, const std::vector<int32_t>& hst, const ChainJob& cjob) {
    const uint32_t m = c.m, n = c.n;
    const uint8_t* hout = M.hout;
    c.st.assign(m, 0);
    if (P.dec || P.var_op) std::memcpy(c.st.data(), hout + L.o_st, 4ull * m);
    else c.st = hst;
    c.newtoks.clear();
    c.nt_met = false;
    if (P.nt_on) {
        // the decoder's new tokens: the entries tagged with this pass, in the order the
        // device numbered them
        const NewTok* ents = reinterpret_cast<const NewTok*>(hout + L.o_nt);
        uint32_t k = 0;
        while (k < kNewTokCap && ents[k].seq == S->nt_seq) ++k;
        c.nt_met = k != 0;
        bool ok = true;
        for (uint32_t i = 0; i < m; ++i) ok &= c.st[i] == LASPJ_DEC_OK;
        if (k && ok) c.newtoks.assign(ents, ents + k);
        // (a merge's writer then wrote nothing and left the operands' cells)
        if (k && c.op == Op::MERGE) S->clean_words = 0;
    }
    if (P.var_op)
        for (int32_t x : c.st)
            if (x != LASPJ_DEC_OK) S->clean_words = 0;   // (its cells were kept)
    c.has_seg = false;
    if (P.defer && cjob.armed &&
        std::find(c.st.begin(), c.st.end(), (int32_t)LASPJ_DEC_UNKNOWN_TERM) != c.st.end()) {
        // (the chain checks copied the failed payloads' results into the answer area;
        // those of payloads that decoded are not read)
        const EtfReadPlan& plan = P.plans[0];
        c.segres.resize(8ull * plan.nseg);
        std::memcpy(c.segres.data(), hout + L.o_seg, kSegResBytes * plan.nseg);
        c.segbase = plan.segbase;
        c.segS = plan.S;
        c.has_seg = true;
    }
    c.res.assign(hout + L.o_res, hout + L.o_res + n);
    if (P.has_payload_out) {
        c.ooff.resize(n + 1ull);
        std::memcpy(c.ooff.data(), hout + L.o_ooff, 8ull * (n + 1));
        const uint64_t total = c.ooff[n];
        if (total > L.ocap) {
            // the writer wrote nothing: a larger answer area, the encode again
            S->ocap = al(total + total / 4, 1 << 16);
            return kPassAgain;
        }
        c.obase = hout + L.o_pay;
    }
    return LASPJ_OK;
}

// One device pass: plan, layout, fit, stage, pull, decode (or upload host-encoded cells),
// answer, one synchronisation, collect.  Fills c.st / c.res / c.ooff / c.obase.
//
// What the phases must keep as it is:
//   - for any call the same HIP operations reach ctx->stream in the same order (memsets,
//     pulls, gathers, copies, kernels), and a pass synchronises exactly once (a call's
//     `tail`, which only the read side sets, adds its launches last, ahead of that
//     synchronisation);
//   - ctx->mu (Guard) is held over fit_pass, over the waiters' payloads' gather inside
//     stage_operands, and from pull_operands to the end — not over the rest of
//     stage_operands (the offsets, the segment tables' copy into pinned memory, the host
//     encoder): group-commit waiters queue their binds meanwhile;
//   - S->clean_words says how many operand cells the enqueued kernels leave zero, set by
//     the answer that decides it (and reset by collect_answers when a status says the
//     cells were kept);
//   - the nif_stats counters move where they did: ST_HOST_ENCODED per host-encoded pass,
//     ST_PASSES and the timers ST_NS_ENQUEUE / _WAIT / _COPY at the synchronise,
//     ST_NS_ANSWERS behind a pass that answered.
int device_pass(laspj_ctx* ctx, NifState* S, Call& c) {
    const uint64_t t0 = now_ns();
    const PassPlan P = plan_pass(ctx, c);
    const PassLayout L = layout_pass(S, c, P);
    PassMem M;
    if (int s = fit_pass(ctx, S, c, P, L, &M)) return s;
    std::vector<int32_t> hst;       // the host encoder's statuses (no device decode)
    if (int s = stage_operands(ctx, S, c, P, L, M, &hst)) return s;
    Guard g(ctx);
    uint64_t t_copy = 0;
    ChainJob cjob;
    if (int s = pull_operands(ctx, c, P, L, M, &t_copy)) return s;
    if (int s = enqueue_decode(ctx, S, c, P, L, M, hst, &cjob)) return s;
    if (int s = enqueue_answer(ctx, S, c, P, L, M, &cjob)) return s;
    if (c.tail)
        if (int s = c.tail()) return s;
    const uint64_t t1 = now_ns();
    LJ_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t t2 = now_ns();
    ++S->stats[ST_PASSES];
    S->stats[ST_NS_ENQUEUE] += t1 - t0;
    S->stats[ST_NS_WAIT] += t2 - t1;
    S->stats[ST_NS_COPY] += t_copy;
    const int s = collect_answers(S, c, P, L, M, hst, cjob);
    if (s == LASPJ_OK) S->stats[ST_NS_ANSWERS] += now_ns() - t2;
    return s;
}

int register_payloads(laspj_ctx* ctx, NifState* S, KindState& K,
                      const std::vector<const uint8_t*>& p, const std::vector<uint64_t>& len,
                      std::vector<int32_t>* st) {
    const uint64_t t0 = now_ns();
    const uint64_t k = p.size();
    std::vector<uint64_t> offs(k + 1, 0);
    for (uint64_t i = 0; i < k; ++i) offs[i + 1] = offs[i] + len[i];
    std::vector<uint8_t> blob(offs[k] + 1);
    for (uint64_t i = 0; i < k; ++i)
        if (len[i]) std::memcpy(blob.data() + offs[i], p[i], len[i]);
    st->assign(k, 0);
    if (int s = laspj_dict_add(K.dict, K.kind, blob.data(), offs.data(), k, -1, st->data()))
        return fail(ctx, s, "nif: dictionary registration failed (%d)", s);
    ++S->stats[ST_REGISTRATIONS];
    S->stats[ST_NS_REGISTER] += now_ns() - t0;
    K.stale = true;
    return LASPJ_OK;
}

// A deferred pass's unknown terms: each failing segment of those operands (a status and a
// start: its first element, where the chain check found it) registers the elements that
// start in it — what the segment's decoder could not take; the segments that decoded hold
// known terms.  False: a range did not register (nothing is kept), the caller registers
// whole operands.
bool register_segments(NifState* S, const Call& c, const std::vector<uint32_t>& ops) {
    const uint64_t t0 = now_ns();
    struct Range {
        uint32_t i;
        uint64_t from, to;
    };
    std::vector<Range> rs;
    for (uint32_t i : ops) {
        if (i + 1 >= c.segbase.size()) return false;
        for (uint32_t g = c.segbase[i]; g < c.segbase[i + 1]; ++g) {
            const int32_t st = (int32_t)c.segres[8ull * g];
            const uint32_t start = c.segres[8ull * g + 1];
            if (st == LASPJ_DEC_OK) continue;
            if (start == 0xFFFFFFFFu) return false;
            const uint64_t s = g - c.segbase[i];
            rs.push_back({i, start, std::min<uint64_t>((s + 1) * c.segS, c.len[i])});
        }
    }
    if (rs.empty()) return false;
    for (const Range& r : rs) {
        // (the payload's group: its namespace's dictionary)
        KindState& K = *c.groups[group_of(c, r.i)].K;
        if (dict_add_elems(K.dict, c.p[r.i], c.len[r.i], r.from, r.to) != LASPJ_DEC_OK)
            return false;       // (ranges already added stay: they hold well-formed terms)
        K.stale = true;
    }
    ++S->stats[ST_REGISTRATIONS];
    S->stats[ST_NS_REGISTER] += now_ns() - t0;
    return true;
}

// The tokens a pass's decoder took (NewTok): registered in the host dictionary at the
// slots the device gave them — each element's next free slots in payload order, which is
// the order the dictionary numbers them in; the device images learn them on the next call
// (patch_etf).  A slot the dictionary would number otherwise cannot happen by
// construction; it fails the call loudly (the cells already hold the device's slots).
int register_new_tokens(laspj_ctx* ctx, NifState* S, KindState& K, const Call& c,
                        bool* conflict) {
    const uint64_t t0 = now_ns();
    *conflict = false;
    std::vector<NewTok> ts = c.newtoks;
    std::sort(ts.begin(), ts.end(), [](const NewTok& a, const NewTok& b) {
        return a.e != b.e ? a.e < b.e : a.slot < b.slot;
    });
    const uint32_t TL = etf_dict_tok_len(K.etf);
    // an entry's image: offsets are into the call's payloads laid end to end
    auto image = [&](const NewTok& t) -> const uint8_t* {
        uint64_t at = 0;
        for (uint32_t i = 0; i < c.m; ++i) {
            if (t.off >= at && (uint64_t)t.off + TL <= at + c.len[i]) return c.p[i] + (t.off - at);
            at += c.len[i];
        }
        return nullptr;
    };
    // two operands of a merge may each take a token for one element: the same slot is
    // the same token (kept once) or a conflict (the caller decodes the usual way)
    std::vector<NewTok> uniq;
    for (size_t i = 0; i < ts.size(); ++i) {
        if (!uniq.empty() && uniq.back().e == ts[i].e && uniq.back().slot == ts[i].slot) {
            const uint8_t *x = image(uniq.back()), *y = image(ts[i]);
            if (!x || !y || std::memcmp(x, y, TL) != 0) {
                *conflict = true;
                return LASPJ_OK;
            }
            continue;
        }
        uniq.push_back(ts[i]);
    }
    dict_begin(K.dict);
    for (const NewTok& t : uniq) {
        uint32_t slot = 0;
        const uint8_t* img = image(t);
        const int st = img ? dict_reg_tok(K.dict, t.e, img, TL, &slot) : LASPJ_DEC_MALFORMED;
        if (st != LASPJ_DEC_OK || slot != t.slot) {
            dict_rollback(K.dict);
            return fail(ctx, LASPJ_E_DEVICE,
                        "nif: new token of element %u at slot %u registered as %u (%d)", t.e,
                        t.slot, slot, st);
        }
    }
    dict_begin(K.dict);                           // (the journal kept nothing)
    K.stale = true;                               // (patched on the next call)
    ++S->stats[ST_REGISTRATIONS];
    S->stats[ST_NEW_TOKENS] += uniq.size();
    S->stats[ST_NS_REGISTER] += now_ns() - t0;
    return LASPJ_OK;
}

// the image of a resident variable (a READ pass; the caller holds S->mu)
int read_var(laspj_ctx* ctx, NifState* S, laspj_var* v, std::vector<uint8_t>* img) {
    Call c;
    c.op = Op::READ;
    c.kind = v->kind;
    c.n = 1;
    c.m = 0;
    c.vars.push_back(v);
    one_group(c, v->ns.get());
    std::vector<int32_t> vd;
    if (int s = run(ctx, S, c, &vd)) return s;
    if (vd[0] != LASPJ_NIF_OK) return fail(ctx, LASPJ_E_DEVICE, "nif: variable encode failed");
    img->assign(c.obase + c.ooff[0], c.obase + c.ooff[1]);
    return LASPJ_OK;
}

// Before a dictionary of this kind is dropped: every resident variable over it is written
// out to its image (encoded on the device with the dictionary its cells refer to) and its
// cells released; the next call that uses it decodes the image again (hydrate)
int spill_vars(laspj_ctx* ctx, NifState* S, KindState& K) {
    for (laspj_var* v : K.vars) {
        if (!v->resident || v->epoch != K.epoch) continue;
        if (!v->cells) {
            v->image.assign({131, 106});              // new() = []
        } else if (int s = read_var(ctx, S, v, &v->image)) {
            return s;
        }
        {
            Guard g(ctx);
            release_cells(ctx, v);
        }
        v->resident = false;
        ++S->stats[ST_SPILLED];
    }
    return LASPJ_OK;
}

}  // namespace

// the call's payloads decoded against one dictionary
void one_group(Call& c, KindState* K) { c.groups.assign(1, Group{K, 0, c.m}); }

int reset_dict(laspj_ctx* ctx, NifState* S, KindState& K) {
    const bool had = K.dict != nullptr;       // (creating a namespace's first is no reset)
    if (had) {
        if (int s = spill_vars(ctx, S, K)) return s;
        if (int s = spill_lvars(S, K)) return s;
    }
    free_etf(K);
    if (K.dict) laspj_dict_destroy(K.dict);
    K.dict = nullptr;
    if (laspj_dict_create(&K.dict) != LASPJ_OK)
        return fail(ctx, LASPJ_E_NOMEM, "nif: dictionary allocation");
    K.stale = false;
    K.wide = false;                           // (a fresh dictionary starts narrow)
    K.tw = 1;
    K.pair_scanned = 0;
    K.has_pair = false;
    K.rank_full = true;
    K.rank_dirty.clear();
    K.built_toks = 0;
    ++K.epoch;
    if (had) ++S->stats[ST_RESETS];
    return LASPJ_OK;
}

namespace {

// an operand met an element's 64 token slots all taken: the namespace goes wide (true: the
// caller registers the operands again)
bool widen(NifState* S, KindState& K, const std::vector<int32_t>& st) {
    if (K.wide || K.kind != LASPJ_KIND_ORSET) return false;
    for (int32_t x : st)
        if (x == LASPJ_DEC_UNREPRESENTABLE) return go_wide(S, K);
    return false;
}

// what run() keeps between a call's passes: the groups whose operands were registered, the
// answers already given to the reference's clause
struct RunState {
    std::vector<uint8_t> registered;    // per group
    std::vector<uint8_t> fallback;      // per answer (payload i belongs to answer i % n)
};

// a group's whole operands registered (again with a wide namespace when an element's 64
// token slots ran out); the operands that did not register answer FALLBACK
int register_group(laspj_ctx* ctx, NifState* S, const Call& c, size_t g, RunState* rs) {
    KindState& K = *c.groups[g].K;
    const uint32_t p0 = c.groups[g].p0, p1 = c.groups[g].p1;
    const std::vector<const uint8_t*> rp(c.p.begin() + p0, c.p.begin() + p1);
    const std::vector<uint64_t> rl(c.len.begin() + p0, c.len.begin() + p1);
    std::vector<int32_t> rst;
    if (int s = register_payloads(ctx, S, K, rp, rl, &rst)) return s;
    if (widen(S, K, rst))
        if (int s = register_payloads(ctx, S, K, rp, rl, &rst)) return s;
    for (uint32_t i = p0; i < p1; ++i)
        if (rst[i - p0] != LASPJ_DEC_OK) rs->fallback[i % c.n] = 1;
    return LASPJ_OK;
}

// Ahead of a pass: every group's device images brought up to its dictionary (a group with
// none yet registers its operands first), patched in place when only tokens were added.
int refresh_images(laspj_ctx* ctx, NifState* S, Call& c, RunState* rs) {
    for (size_t g = 0; g < c.groups.size(); ++g) {
        KindState& K = *c.groups[g].K;
        if (K.etf && !K.stale) continue;
        if (!K.etf && c.groups[g].p1 > c.groups[g].p0) {
            // nothing registered yet: register this group's operands first
            if (int s = register_group(ctx, S, c, g, rs)) return s;
            rs->registered[g] = 1;
        }
        // a wide namespace's operands are host-encoded: its device images serve the
        // answers' writers only, so a call that writes none keeps the stale ones
        // (while the cells' element slots and pairs still hold every term)
        if (K.wide && K.etf && dict_elements(K.dict) <= K.E &&
            dict_max_tokens(K.dict) <= 64u * K.tw && c.op != Op::MERGE &&
            c.op != Op::VALUE && c.op != Op::VVALUE && c.op != Op::READ)
            continue;
        if (!patch_etf(ctx, S, K)) {
            if (int s = rebuild_etf(ctx, S, K)) return s;
            c.redo.n = 0;         // (element ranks moved: the last pass's results stale)
        }
    }
    return LASPJ_OK;
}

// Terms a dictionary has not seen (or operands that are not orddicts, which the next pass
// tells apart): each group registers its operands that met them (an operand that decoded
// holds only registered terms).
int register_unknown(laspj_ctx* ctx, NifState* S, Call& c, const std::vector<uint32_t>& unknown,
                     RunState* rs) {
    // a variable call's operands are its own (payload i belongs to variable i): an element
    // past its 64 token slots widens the namespace's cells (k {p, r} pairs); only image
    // calls start a fresh dictionary for it, and only write/4 resets a dictionary grown past
    // its bound (bind / threshold answer FALLBACK there and the NIF runs the reference's
    // clause over the variable's read image)
    const bool may_reset = !(c.op == Op::BIND || c.op == Op::THRESHOLD);
    for (size_t g = 0; g < c.groups.size(); ++g) {
        KindState& K = *c.groups[g].K;
        const uint32_t p0 = c.groups[g].p0, p1 = c.groups[g].p1;
        std::vector<uint32_t> ri;
        std::vector<const uint8_t*> rp;
        std::vector<uint64_t> rl;
        std::vector<int32_t> rst;
        for (uint32_t i : unknown)
            if (i >= p0 && i < p1) {
                rp.push_back(c.p[i]);
                rl.push_back(c.len[i]);
                ri.push_back(i);
            }
        if (ri.empty()) continue;
        uint32_t nd = 0;
        uint64_t eb, tb;
        if (int s = register_payloads(ctx, S, K, rp, rl, &rst)) return s;
        bool full = false;
        for (int32_t x : rst) full |= x == LASPJ_DEC_UNREPRESENTABLE;
        laspj_dict_info(K.dict, &nd, &eb, &tb);
        // image calls own their namespace's terms for the call only: a wide one starts
        // over narrow when it meets new terms (the narrow codec is the fast one)
        const bool image_call = c.vars.empty();
        if (may_reset && ((image_call && ((full && nd) || K.wide)) || nd > kMaxDictElements)) {
            // an element's 64 token slots used up by earlier calls (or a dictionary grown
            // past its bound): start a fresh dictionary holding this group's terms only —
            // image calls are self-contained (images in, images out); the namespace's
            // resident variables are written out to their images first and decoded again
            // when next used
            // (an operand of more than 64 tokens on an element even so: wide)
            if (int s = reset_dict(ctx, S, K)) return s;
            if (int s = register_group(ctx, S, c, g, rs)) return s;
            for (uint32_t i = p0; i < p1 && i < c.vars.size(); ++i) {
                c.vars[i]->epoch = K.epoch;           // write/4's own variable: new cells
                c.vars[i]->resident = true;
            }
        } else {
            // a variable's namespace (its replicas' cells hold its slots) goes wide
            // rather than start over
            if (widen(S, K, rst))
                if (int s = register_payloads(ctx, S, K, rp, rl, &rst)) return s;
            for (size_t k = 0; k < ri.size(); ++k)
                if (rst[k] != LASPJ_DEC_OK) rs->fallback[ri[k] % c.n] = 1;
        }
        rs->registered[g] = 1;
    }
    return LASPJ_OK;
}

}  // namespace

// The call: device pass; operands with unknown terms registered and a second pass; every
// other undecodable operand -> FALLBACK.  verdict[j] per answer.
int run(laspj_ctx* ctx, NifState* S, Call& c, std::vector<int32_t>* verdict) {
    ++S->stats[ST_CALLS];
    const size_t G = c.groups.size();
    for (const Group& g : c.groups)
        if (!g.K->dict && reset_dict(ctx, S, *g.K)) return LASPJ_E_NOMEM;
    const uint32_t n = c.n, m = c.m;
    RunState rs{std::vector<uint8_t>(G, 0), std::vector<uint8_t>(n, 0)};
    bool partial = false;           // the last registration took the failing segments only
    bool resolved = false;          // the last pass's answers stand (statuses all final)
    const int passes = ctx->tune_nif_passes ? (int)ctx->tune_nif_passes : kMaxPasses;
    std::vector<uint8_t> written;
    for (int pass = 0; pass < passes && !resolved; ++pass) {
        if (int s = refresh_images(ctx, S, c, &rs)) return s;
        int s = device_pass(ctx, S, c);
        c.redo.n = 0;                 // (a redo pass is taken once)
        if (s == kPassAgain) {
            // answer area grown: once more (a write-only pass's writer may have cleared
            // the operands: decode them again)
            if (c.write_only) {
                c.write_only = false;
                S->clean_words = 0;
            }
            continue;
        }
        if (s) return s;
        c.write_only = false;
        if (!c.newtoks.empty()) {
            KindState& K = *c.groups[0].K;
            bool conflict = false;
            if (int s2 = register_new_tokens(ctx, S, K, c, &conflict)) return s2;
            if (conflict) {
                // two operands gave one slot to different tokens: decode again the usual
                // way (registration, then a pass over the known terms)
                c.no_newtok = true;
                S->clean_words = 0;
                continue;
            }
            if (c.op == Op::MERGE) {
                // the answer needs the tokens' images: patch them in, then join and write
                // the cells the decoders left (a rebuild moves element slots: decode again)
                if (patch_etf(ctx, S, K)) {
                    c.write_only = true;
                } else {
                    if (int s2 = rebuild_etf(ctx, S, K)) return s2;
                    S->clean_words = 0;
                }
                continue;
            }
        }
        // a bind that decoded in this pass was merged in it: WRITTEN if this pass (or an
        // earlier one, for an operand whose call needed another pass) changed its value
        if (c.op == Op::BIND) {
            written.resize(n, 0);
            for (uint32_t i = 0; i < m; ++i)
                if (c.st[i] == LASPJ_DEC_OK) written[i] |= c.res[i];
        }
        bool redo = false;
        for (uint32_t i = 0; i < m; ++i) redo |= c.st[i] == kDecRedo;
        if (redo) {
            // a segment chain that only a serial decode can judge: once more, decoding
            // serially (the join's answer of this pass is not used)
            c.no_defer = true;
            ++S->stats[ST_CHAIN_REDOS];
            continue;
        }
        std::vector<uint32_t> unknown;
        for (uint32_t i = 0; i < m; ++i) {
            if (rs.fallback[i % n]) continue;
            // (an element past a narrow namespace's 64 token slots: its registration widens
            // the namespace)
            const KindState& Ki = *c.groups[group_of(c, i)].K;
            const bool grow = c.st[i] == LASPJ_DEC_UNREPRESENTABLE &&
                              Ki.kind == LASPJ_KIND_ORSET && !Ki.wide;
            if ((c.st[i] == LASPJ_DEC_UNKNOWN_TERM || grow) &&
                (!rs.registered[group_of(c, i)] || partial))
                unknown.push_back(i);
            else if (c.st[i] != LASPJ_DEC_OK)
                rs.fallback[i % n] = 1;
        }
        if (unknown.empty()) {
            resolved = true;
            break;
        }
        bool fresh = true;            // no group of an unknown operand registered yet
        for (uint32_t i : unknown) fresh &= !rs.registered[group_of(c, i)];
        if (fresh && c.has_seg && register_segments(S, c, unknown)) {
            // the failing segments' elements registered; if the next pass still meets an
            // unknown term, the whole operands are registered after all
            partial = true;
            for (uint32_t i : unknown) rs.registered[group_of(c, i)] = 1;
            // a single bind: the next pass decodes only those segments again, over the
            // payload and cells this pass left (when the images are patched, not rebuilt)
            if (c.op == Op::BIND && n == 1 && !c.no_defer && !c.nt_met) {
                SegList sl;
                for (uint32_t i : unknown)
                    for (uint32_t g = c.segbase[i]; g < c.segbase[i + 1] && sl.n <= 31; ++g)
                        if ((int32_t)c.segres[8ull * g] != LASPJ_DEC_OK) {
                            if (sl.n < 31) sl.g[sl.n] = g;
                            ++sl.n;
                        }
                if (sl.n <= 31) c.redo = sl;
            }
            continue;
        }
        partial = false;
        if (int s2 = register_unknown(ctx, S, c, unknown, &rs)) return s2;
    }
    // post-condition: an answer is OK only from a pass whose statuses were all final; a
    // call whose passes ran out (the answer area grown, a segment chain only a serial
    // decode judges, terms registered — each on the last pass) hands every operand to the
    // reference's clause rather than answer from a superseded pass
    if (c.op == Op::BIND && written.size() == n) c.res = written;
    verdict->assign(n, LASPJ_NIF_OK);
    for (uint32_t j = 0; j < n; ++j)
        if (rs.fallback[j] || !resolved) {
            (*verdict)[j] = LASPJ_NIF_FALLBACK;
            ++S->stats[ST_FALLBACKS];
        }
    return LASPJ_OK;
}

NifState* state(laspj_ctx* ctx) {
    // (without ctx->mu once it exists: a device phase holds that lock, and binds arriving
    // meanwhile must reach the group-commit queue, not wait behind it)
    if (NifState* s = __atomic_load_n(&ctx->nif, __ATOMIC_ACQUIRE)) return s;
    std::lock_guard<std::mutex> lk(ctx->mu);
    if (!ctx->nif) {
        NifState* s = new (std::nothrow) NifState;
        if (s) s->ks[1].kind = LASPJ_KIND_GSET;
        __atomic_store_n(&ctx->nif, s, __ATOMIC_RELEASE);
    }
    return ctx->nif;
}

bool nif_gc_hooks(laspj_ctx* ctx, GcHooks* h) {
    NifState* S = state(ctx);
    if (!S) return false;
    h->mu = &S->mu;
    h->stats = S->stats;
    h->slot = &S->gc;
    return true;
}

// a namespace's dictionary and device images dropped (the context still alive)
void free_ns(KindState& K) {
    free_etf(K);
    if (K.krank) hipFree(K.krank);
    if (K.grank) hipFree(K.grank);
    K.krank = K.grank = nullptr;
    K.krank_bytes = K.grank_bytes = 0;
    K.rank_E = 0;
    K.rank_full = true;
    if (K.dict) laspj_dict_destroy(K.dict);
    K.dict = nullptr;
}

void nif_destroy(laspj_ctx* ctx) {
    NifState* S = ctx->nif;
    if (!S) return;
    {
        std::lock_guard<std::mutex> lk(S->mu);
        {
            Guard g(ctx);
            for (laspj_var* v : S->vars) {
                // the variables' cells go with the context (the cache it frees next)
                release_cells(ctx, v);
                v->ctx = nullptr;
                v->resident = false;
            }
            // the filters' tables too; a filter outliving its context is dead
            for (laspj_filter* f : S->filters) {
                if (f->dev) dev_release(ctx, f->dev, f->dev_bytes);
                f->dev = nullptr;
                f->ctx = nullptr;
                f->in = f->out = nullptr;
                f->ns.reset();
            }
            S->filters.clear();
            maps_ctx_gone(ctx, S);
            folds_ctx_gone(ctx, S);
        }
        // the list-valued variables' lists go with the context; one outliving it is dead
        for (laspj_lvar* lv : S->lvars) {
            for (laspj_batch** b : {&lv->list, &lv->val, &lv->dst, &lv->tmp}) {
                if (*b) laspj_batch_destroy(*b);
                *b = nullptr;
            }
            for (LWaiter& w : lv->waiters) lwaiter_release(w);
            free_ns(*lv->ns);
            lv->ns->lvars.clear();
            lv->ctx = nullptr;
            lv->resident = false;
        }
        S->lvars.clear();
        // their namespaces' device images too (a variable outliving its context keeps only
        // the host side, which its destroy frees)
        for (laspj_var* v : S->vars) {
            free_ns(*v->ns);
            v->ns->vars.clear();
        }
        S->vars.clear();
        gc_ctx_destroy(ctx, S->gc);
        S->gc = nullptr;
    }
    for (KindState& K : S->ks) free_ns(K);
    hipSetDevice(ctx->device);
    hipStreamSynchronize(ctx->stream);
    if (S->dblk) hipFree(S->dblk);
    if (S->dcells) hipFree(S->dcells);
    if (S->hin) hipHostFree(S->hin);
    if (S->hout) hipHostFree(S->hout);
    if (S->rd_d) hipFree(S->rd_d);
    if (S->rd_h) hipHostFree(S->rd_h);
    if (S->lv_tiles) hipFree(S->lv_tiles);
    if (S->lp_side) hipFree(S->lp_side);
    if (S->lv_ans) hipHostFree(S->lv_ans);
    for (const PinSlot& p : S->pins) hipHostFree(p.h);
    delete S;
    ctx->nif = nullptr;
}

}  // namespace laspj

using laspj::fail;

namespace {

int pair_call(laspj_ctx* ctx, laspj::NifState* S, int32_t kind, laspj::Op op, int strict,
              uint32_t n, const uint8_t* const* a, const uint64_t* na, const uint8_t* const* b,
              const uint64_t* nb, laspj::Call* c, std::vector<int32_t>* verdict) {
    if (!n || !a || !na || (op != laspj::Op::VALUE && (!b || !nb)))
        return fail(ctx, LASPJ_E_INVAL, "nif: null operand array");
    const uint32_t per = op == laspj::Op::VALUE ? 1u : 2u;
    if ((uint64_t)n * per > (1ull << 31))
        return fail(ctx, LASPJ_E_RANGE, "nif: too many operands");
    c->op = op;
    c->kind = kind;
    c->strict = strict;
    c->n = n;
    c->m = n * per;
    c->p.resize(c->m);
    c->len.resize(c->m);
    for (uint32_t i = 0; i < n; ++i) {
        if ((!a[i] && na[i]) || (per == 2 && !b[i] && nb[i]))
            return fail(ctx, LASPJ_E_INVAL, "nif: null payload");
        c->p[i] = a[i];
        c->len[i] = na[i];
        if (per == 2) {
            c->p[n + i] = b[i];
            c->len[n + i] = nb[i];
        }
    }
    laspj::one_group(*c, &laspj::kstate(S, kind));
    return laspj::run(ctx, S, *c, verdict);
}

int merge_many(int32_t kind, laspj_ctx* ctx, uint32_t n, const uint8_t* const* a,
               const uint64_t* na, const uint8_t* const* b, const uint64_t* nb,
               const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!out || !out_len || !verdict) return fail(ctx, LASPJ_E_INVAL, "nif: null output array");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::Call c;
    std::vector<int32_t> v;
    if (int s = pair_call(ctx, e.S, kind, laspj::Op::MERGE, 0, n, a, na, b, nb, &c, &v)) return s;
    for (uint32_t i = 0; i < n; ++i) {
        verdict[i] = v[i];
        out[i] = v[i] == LASPJ_NIF_OK ? c.obase + c.ooff[i] : nullptr;
        out_len[i] = v[i] == LASPJ_NIF_OK ? c.ooff[i + 1] - c.ooff[i] : 0;
    }
    return LASPJ_OK;
}

int bool_call(int32_t kind, laspj_ctx* ctx, laspj::Op op, int strict, const uint8_t* a,
              uint64_t na, const uint8_t* b, uint64_t nb, int32_t* result, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!result || !verdict) return fail(ctx, LASPJ_E_INVAL, "nif: null output");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::Call c;
    std::vector<int32_t> v;
    if (int s = pair_call(ctx, e.S, kind, op, strict, 1, &a, &na, &b, &nb, &c, &v)) return s;
    *verdict = v[0];
    *result = v[0] == LASPJ_NIF_OK ? (int32_t)(c.res[0] != 0) : 0;
    return LASPJ_OK;
}

}  // namespace

extern "C" {

int laspj_orset_etf_merge_many(laspj_ctx* ctx, uint32_t n, const uint8_t* const* a,
                               const uint64_t* na, const uint8_t* const* b, const uint64_t* nb,
                               const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    return merge_many(LASPJ_KIND_ORSET, ctx, n, a, na, b, nb, out, out_len, verdict);
}

int laspj_orset_etf_merge(laspj_ctx* ctx, const uint8_t* a, uint64_t na, const uint8_t* b,
                          uint64_t nb, const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    return laspj_orset_etf_merge_many(ctx, 1, &a, &na, &b, &nb, out, out_len, verdict);
}

int laspj_orset_etf_value(laspj_ctx* ctx, const uint8_t* s, uint64_t ns, const uint8_t** out,
                          uint64_t* out_len, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!out || !out_len || !verdict) return fail(ctx, LASPJ_E_INVAL, "nif: null output");
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::Call c;
    std::vector<int32_t> v;
    if (int st = pair_call(ctx, e.S, LASPJ_KIND_ORSET, laspj::Op::VALUE, 0, 1, &s, &ns, nullptr,
                           nullptr, &c, &v))
        return st;
    *verdict = v[0];
    *out = v[0] == LASPJ_NIF_OK ? c.obase + c.ooff[0] : nullptr;
    *out_len = v[0] == LASPJ_NIF_OK ? c.ooff[1] - c.ooff[0] : 0;
    return LASPJ_OK;
}

int laspj_orset_etf_equal(laspj_ctx* ctx, const uint8_t* a, uint64_t na, const uint8_t* b,
                          uint64_t nb, int32_t* result, int32_t* verdict) {
    return bool_call(LASPJ_KIND_ORSET, ctx, laspj::Op::EQUAL, 0, a, na, b, nb, result, verdict);
}

int laspj_orset_etf_inflation(laspj_ctx* ctx, const uint8_t* prev, uint64_t np,
                              const uint8_t* cur, uint64_t nc, int strict, int32_t* result,
                              int32_t* verdict) {
    return bool_call(LASPJ_KIND_ORSET, ctx, laspj::Op::INFLATION, strict ? 1 : 0, prev, np, cur,
                     nc, result, verdict);
}

// ---------------------------------------------------------------- lasp_gset

int laspj_gset_etf_merge_many(laspj_ctx* ctx, uint32_t n, const uint8_t* const* a,
                              const uint64_t* na, const uint8_t* const* b, const uint64_t* nb,
                              const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    return merge_many(LASPJ_KIND_GSET, ctx, n, a, na, b, nb, out, out_len, verdict);
}

int laspj_gset_etf_merge(laspj_ctx* ctx, const uint8_t* a, uint64_t na, const uint8_t* b,
                         uint64_t nb, const uint8_t** out, uint64_t* out_len, int32_t* verdict) {
    return laspj_gset_etf_merge_many(ctx, 1, &a, &na, &b, &nb, out, out_len, verdict);
}

int laspj_gset_etf_value(laspj_ctx* ctx, const uint8_t* s, uint64_t ns, const uint8_t** out,
                         uint64_t* out_len, int32_t* verdict) {
    // value/1 = ordsets:to_list/1 (lasp_gset.erl:74-76), the identity on any term: the
    // answer is the operand's own image (no device work)
    if (!ctx) return LASPJ_E_INVAL;
    if (!out || !out_len || !verdict || (!s && ns))
        return fail(ctx, LASPJ_E_INVAL, "nif: null argument");
    *out = s;
    *out_len = ns;
    *verdict = LASPJ_NIF_OK;
    return LASPJ_OK;
}

int laspj_gset_etf_equal(laspj_ctx* ctx, const uint8_t* a, uint64_t na, const uint8_t* b,
                         uint64_t nb, int32_t* result, int32_t* verdict) {
    return bool_call(LASPJ_KIND_GSET, ctx, laspj::Op::EQUAL, 0, a, na, b, nb, result, verdict);
}

int laspj_gset_etf_inflation(laspj_ctx* ctx, const uint8_t* prev, uint64_t np,
                             const uint8_t* cur, uint64_t nc, int strict, int32_t* result,
                             int32_t* verdict) {
    return bool_call(LASPJ_KIND_GSET, ctx, laspj::Op::INFLATION, strict ? 1 : 0, prev, np, cur,
                     nc, result, verdict);
}

// ---------------------------------------------------------------- counters

int laspj_nif_stats(laspj_ctx* ctx, uint64_t* out, uint32_t n) {
    if (!ctx || (n && !out)) return LASPJ_E_INVAL;
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    for (uint32_t i = 0; i < n && i < LASPJ_NIF_STATS; ++i) out[i] = S->stats[i];
    if (n > 7) {
        // [7] is the dictionaries' size, not a counter: the image calls' and every
        // namespace's
        uint64_t tot = 0;
        std::unordered_set<const laspj::KindState*> seen;
        auto add = [&](const laspj::KindState* K) {
            uint32_t e = 0;
            uint64_t eb, tb;
            if (K->dict && seen.insert(K).second) {
                laspj_dict_info(K->dict, &e, &eb, &tb);
                tot += e;
            }
        };
        for (const laspj::KindState& K : S->ks) add(&K);
        for (const laspj_var* v : S->vars) add(v->ns.get());
        for (const laspj_lvar* lv : S->lvars) add(lv->ns.get());
        out[7] = tot + laspj::gc_dict_elements(S->gc);
    }
    return LASPJ_OK;
}

int laspj_nif_reset(laspj_ctx* ctx) {
    if (!ctx) return LASPJ_E_INVAL;
    const laspj::Entry e = laspj::enter_ctx(ctx);
    if (e.rc) return e.rc;
    laspj::NifState* S = e.S;
    for (laspj::KindState& K : S->ks)
        if (int s = laspj::reset_dict(ctx, S, K)) return s;
    std::unordered_set<laspj::KindState*> seen;
    std::vector<std::shared_ptr<laspj::KindState>> nss;
    for (laspj_var* v : S->vars)
        if (seen.insert(v->ns.get()).second) nss.push_back(v->ns);
    for (laspj_lvar* lv : S->lvars)
        if (seen.insert(lv->ns.get()).second) nss.push_back(lv->ns);
    for (auto& ns : nss)
        if (int s = laspj::reset_dict(ctx, S, *ns)) return s;
    return laspj::gc_ctx_reset(ctx, S->gc);
}

}  // extern "C"
