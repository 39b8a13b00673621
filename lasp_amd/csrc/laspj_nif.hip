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

#include <sys/random.h>

#include <algorithm>
#include <atomic>
#include <cerrno>
#include <chrono>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <memory>
#include <new>
#include <unordered_set>
#include <vector>

#include "laspj_internal.h"

namespace laspj {

// One dictionary of one kind (OR-Set or G-Set) and its device images.  The image calls of a
// context share one per kind; every resident variable has one of its own — its token
// namespace — shared only with the replicas created beside it (laspj_var_create_replica),
// so a variable's dictionary holds the terms of its own value (and its replicas') and
// variables never compete for an element's token slots (include/lasp.hrl:60-63: each
// #dv.value is independent).
struct KindState {
    int32_t kind = LASPJ_KIND_ORSET;
    laspj_dict* dict = nullptr;     // term images -> slots (host, append-only)
    laspj_etf_dict* etf = nullptr;  // the device images of `dict` (rebuilt when it grows)
    uint32_t E = 0;                 // element slots of `etf` and of the batches
    bool stale = false;             // `dict` registered terms since `etf` was built
    uint64_t epoch = 1;             // bumped by every reset (variables' cells refer to one)
    // what `etf` was built (or last patched) from: host dictionary elements and each
    // one's token count, so registrations that only add tokens to known elements are
    // patched into the device images (etf_dict_patch) instead of rebuilding them
    uint32_t built_K = 0;
    std::vector<uint32_t> built_cnt;
    // the variables whose cells refer to this dictionary (none for the image calls')
    std::unordered_set<laspj_var*> vars;
    // a wide namespace: an element holds more than 64 tokens (add_elem never collects one,
    // lasp_orset.erl:222-241): cells of tw {p, r} pairs per element, the wide tables in wd
    // (etf then holds the element images only, for value/1's G-Set answer)
    bool wide = false;
    uint32_t tw = 1;
    WideDict* wd = nullptr;
    // whether `dict` has registered a 2-tuple element (laspj_var_intersection: the bodies'
    // `{X, Causality}` branch takes those), kept incrementally: slots below pair_scanned
    // have been looked at
    uint32_t pair_scanned = 0;
    bool has_pair = false;
    // the list-valued variables over this dictionary (laspj_lvar) and the order tables their
    // list kernels compare by, derived on the device from `etf`'s images (laspj_lvars.hip):
    // krank (rank_E words) and grank (64 rank_E words).  rank_full: the images were rebuilt
    // since the tables were written; rank_dirty: the element slots patch_etf rewrote since.
    // Kept only while the namespace has list variables.
    std::unordered_set<laspj_lvar*> lvars;
    void* krank = nullptr;
    uint64_t krank_bytes = 0;
    void* grank = nullptr;
    uint64_t grank_bytes = 0;
    uint32_t rank_E = 0;
    bool rank_full = true;
    std::vector<uint32_t> rank_dirty;
    uint64_t built_toks = 0;        // the tokens `etf` holds over all elements (sum of built_cnt)
};

// One entry of `#dv.waiting_threads` ({threshold, read, From, Type, Threshold},
// lasp_core.erl:331-364): the threshold decoded once into `cells`, a hidden variable of the
// waiting variable's namespace (registered where variables are, so widening, growth and a
// dictionary reset carry it along), and its image as registered.
struct Waiter {
    uint64_t id = 0;
    int32_t strict = 0;
    std::vector<uint8_t> image;
    laspj_var* cells = nullptr;
};

// One entry of `#dv.lazy_threads` ({threshold, wait, From, Type, Threshold},
// lasp_core.erl:730-758), kept as a Waiter's threshold is: decoded once into a hidden
// variable of the namespace.  (The bare-pid entry of :744-746 cannot be reached for the set
// types: threshold_met(Type, Value, undefined) ahead of it raises.)
struct Lazy {
    uint64_t id = 0;
    std::vector<uint8_t> image;
    laspj_var* cells = nullptr;
};

}  // namespace laspj

// A device-resident variable's value (the `#dv.value` of lasp_core's store): cells over its
// namespace's dictionary, or — when its value is not representable, or between a dictionary
// reset and its next use — the value's image held on the host.
struct laspj_var {
    laspj_ctx* ctx = nullptr;        // null once the context is gone
    int32_t kind = LASPJ_KIND_ORSET;
    std::shared_ptr<laspj::KindState> ns;   // the token namespace (dictionary) of the cells
    uint64_t* cells = nullptr;       // one replica over `E` element slots (null: new())
    uint64_t cell_bytes = 0;         // the block's size (dev_alloc)
    uint32_t E = 0;
    uint32_t tw = 1;                 // {p, r} pairs per element slot (a wide namespace's)
    uint64_t epoch = 0;              // the dictionary generation the cells refer to
    bool resident = true;            // cells hold the value (else `image` does)
    bool held = false;               // `image` is a value write/4 could not represent
    std::vector<uint8_t> image;      // host-held value (term_to_binary image)
    std::vector<laspj::Waiter> waiters;   // `#dv.waiting_threads`, in list order
    std::vector<laspj::Lazy> lazy;        // `#dv.lazy_threads`, in list order
    // LASPJ_KIND_GCOUNTER: the variable lives in laspj_counters.hip and nothing above is
    // used (ctx stays null, so a set path reached by mistake answers LASPJ_E_INVAL)
    laspj::GcVar* gc = nullptr;
};

// One lasp_process running filter/6 (lasp_core.erl:681-712) from `in` into `out`, and the
// fun's results for the elements it has seen: two bitmaps over the namespace's element
// slots on the device (dev: [evaluated | keep | pmask], `words` each; pmask is the last
// check pass's pending slots) with the first two mirrored on the host, where
// laspj_filter_results edits them.
struct laspj_filter {
    laspj_ctx* ctx = nullptr;        // null once the context is gone
    laspj_var* in = nullptr;         // null once either variable is destroyed: the filter
    laspj_var* out = nullptr;        // is dead and its calls answer LASPJ_E_INVAL
    std::shared_ptr<laspj::KindState> ns;
    uint64_t epoch = 0;              // the dictionary generation the bitmaps refer to
    uint32_t words = 0;
    uint64_t* dev = nullptr;
    uint64_t dev_bytes = 0;
    std::vector<uint64_t> h_eval, h_keep;
    bool pmask_valid = false;        // pmask is a check pass's of this generation and size
    // laspj_filter_args' list: the slots in the order listed, its image; dropped: a
    // dictionary reset took the list away (the next laspj_filter_results answers OK)
    std::vector<uint32_t> listed;
    bool outstanding = false, dropped = false;
    std::string image;
};

// A list-valued lasp_orset variable (include/laspj.h "list-valued resident variables"): any
// list of {Key, [{Token, Bool}]} over the slots of `ns`, held as a one-replica LIST batch, or
// — between a dictionary reset or a widening and its next use, or when a write's image could
// not be walked — as its image on the host.  val and dst are the bind's other two lists: the
// incoming value (the producer's output, or a walked image) and the merge, which becomes
// `list` by a swap of the blocks when the bind writes.
struct laspj_lvar {
    laspj_ctx* ctx = nullptr;        // null once the context is gone
    std::shared_ptr<laspj::KindState> ns;
    uint64_t epoch = 0;              // the dictionary generation the items refer to
    bool resident = true;            // `list` holds the value (else `image` does)
    bool held = false;               // `image` is a value the walk refused (until the next write)
    laspj_batch* list = nullptr;
    laspj_batch* val = nullptr;
    laspj_batch* dst = nullptr;
    laspj_batch* tmp = nullptr;      // l's list form (the two-step composition, A/B only)
    std::vector<uint8_t> image;
};

namespace laspj {

// a pinned host block a group-commit waiter stages its payload into while it waits
struct PinSlot {
    uint8_t* h = nullptr;           // host address
    const uint8_t* d = nullptr;     // its device address
    uint64_t cap = 0;
};

// a single bind waiting for a group-commit pass (laspj_var_etf_bind)
struct BindReq {
    laspj_var* var;
    const uint8_t* p;
    uint64_t n;
    // the payload's pinned copy (device address), valid once `staged` is set: made by the
    // waiter itself, so the leader's pass gathers it on the device instead of copying it
    const uint8_t* pre = nullptr;
    std::atomic<bool> staged{false};
    int32_t status = 0, verdict = LASPJ_NIF_FALLBACK;
    int rc = LASPJ_OK;
    // its own wake-up (no herd of waiters on one condition and one lock): done — answered;
    // lead — handed the leadership, its request still to serve
    std::mutex m;
    std::condition_variable cv;
    bool done = false, lead = false;
};

// the counters of laspj_nif_stats, by the indices include/laspj.h documents
enum NifStat : uint32_t {
    ST_CALLS,           // [0] calls
    ST_PASSES,          // [1] device passes
    ST_REGISTRATIONS,   // [2] dictionary registrations
    ST_RESETS,          // [3] dictionary resets
    ST_REBUILDS,        // [4] device image rebuilds
    ST_HOST_ENCODED,    // [5] host-encoded passes
    ST_FALLBACKS,       // [6] FALLBACK verdicts
    ST_DICT_ELEMENTS,   // [7] dictionary elements (computed when read, never counted)
    ST_NS_ENQUEUE,      // [8] host ns staging + enqueueing
    ST_NS_WAIT,         // [9] host ns waiting for the device
    ST_NS_ANSWERS,      // [10] host ns reading the answers
    ST_NS_COPY,         // [11] the part of [8] copying operands into pinned memory
    ST_NS_REGISTER,     // [12] host ns registering operands' terms
    ST_NS_IMAGES,       // [13] host ns rebuilding or patching the device images
    ST_PATCHES,         // [14] device image patches
    ST_CHAIN_REDOS,     // [15] passes run again for a chain only a serial decode judges
    ST_SPILLED,         // [16] variables written out by a dictionary reset
    ST_HYDRATED,        // [17] variables decoded back onto the device
    ST_NEW_TOKENS,      // [18] tokens taken by a decoder, registered after the pass
    ST_WIDENED,         // [19] namespaces widened
    ST_COUNT
};
static_assert(ST_COUNT == LASPJ_NIF_STATS, "NifStat names every laspj_nif_stats entry");

struct NifState {
    std::mutex mu;                  // one call at a time (ctx->mu is held per device phase)
    // single binds queued for the next group-commit pass, and whether a caller leads one
    std::mutex qmu;
    std::vector<BindReq*> queue;
    bool leading = false;
    // rebuild_etf's export arrays, kept between rebuilds (S->mu): fresh multi-MB blocks
    // would be paged in again by every rebuild
    std::vector<uint8_t> x_ebl, x_tbl, x_tord;
    std::vector<uint32_t> x_eoff, x_eord, x_toff;
    std::vector<PinSlot> pins;      // free waiters' staging blocks (qmu)
    uint32_t pins_live = 0;         // blocks allocated (qmu)
    KindState ks[2];                // the image calls' dictionaries: [0] OR-Set, [1] G-Set
    // the device block and the cell area of a pass, laid out by PassLayout (the waiter
    // re-check keeps its records at the head of dblk: recheck_pass)
    void* dblk = nullptr;
    uint64_t dblk_bytes = 0;
    void* dcells = nullptr;
    uint64_t dcells_bytes = 0;
    // pinned host staging, coherent (kernels pull the operands from one and write the
    // answers into the other: PassLayout's in and out regions), and the device addresses
    // of both (fit_staging)
    void* hin = nullptr;
    uint64_t hin_bytes = 0;
    void* hout = nullptr;
    uint64_t hout_bytes = 0;
    uint8_t* hin_d = nullptr;
    uint8_t* hout_d = nullptr;
    const void* hin_dkey = nullptr;
    const void* hout_dkey = nullptr;
    // the read check's own blocks (read_pass: its launches ride behind a pass that is using
    // the four above): pinned [ReadDesc | ReadCur | met bytes] and the device records
    void* rd_h = nullptr;
    uint64_t rd_h_bytes = 0;
    uint8_t* rd_hd = nullptr;
    const void* rd_hkey = nullptr;
    void* rd_d = nullptr;
    uint64_t rd_d_bytes = 0;
    uint64_t ocap = 1 << 20;        // bytes reserved for answer payloads
    // the operand cells known to be zero (the fused merge and the variable kernel clear
    // them behind them), so the next call's decoders need no memset
    uint64_t clean_words = 0;
    uint64_t stats[LASPJ_NIF_STATS] = {};
    uint32_t nt_seq = 0;            // device passes that took new tokens (their entries' tag)
    std::unordered_set<laspj_var*> vars;
    // laspj_var_etf_update's answers (valid until the context's next call): the tokens it
    // minted, the image of the element a failed precondition names
    std::vector<uint8_t> minted;
    std::string err_elem;
    GcState* gc = nullptr;          // the counter variables' state (laspj_counters.hip)
    std::unordered_set<laspj_filter*> filters;   // the live filter processes
    // the list-valued variables, their last answer image (valid until the context's next
    // call), the producer's tile sums (device) and its totals {entries, tokens, overflow}
    // (pinned, coherent: the producer's last tile writes them there)
    std::unordered_set<laspj_lvar*> lvars;
    std::string lv_out;
    void* lv_tiles = nullptr;
    uint64_t lv_tiles_bytes = 0;
    uint32_t* lv_ans = nullptr;
    uint32_t* lv_ans_d = nullptr;
};

namespace {

enum class Op { MERGE, VALUE, EQUAL, INFLATION, BIND, WRITE, THRESHOLD, READ, VVALUE };

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

// lasp_orset:update/3 / lasp_gset:update/3 (lasp_orset.erl:99-117, 222-259;
// lasp_gset.erl:84-88) of one call on a resident variable's cells: the ops in order, all or
// nothing.  A REMOVE whose element is absent — not in the cells and not added earlier in the
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
    for (uint32_t k = 0; k < nops; ++k) {
        if (bad < nops) {
            if (status) status[k] = k == bad ? LASPJ_OPST_NOT_PRESENT : LASPJ_OPST_ROLLED_BACK;
            continue;
        }
        const laspj_op o = op(k);
        if (kind == LASPJ_KIND_ORSET) {
            uint64_t* c = cells + 2ull * (uint64_t)o.element * tw;
            if (o.kind == LASPJ_OP_ADD) {
                // orddict:store(Token, false, Tokens): present, flag false
                const uint32_t t = op_slot(o);
                c[2 * (t >> 6)] |= 1ull << (t & 63u);
                c[2 * (t >> 6) + 1] &= ~(1ull << (t & 63u));
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

// the same for a call of ADDs only (add_all over many elements): commutative, one op per lane
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
        atomicAnd(c + 1, ~(1ull << (t & 63u)));
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

struct Guard {
    std::lock_guard<std::mutex> lk;
    explicit Guard(laspj_ctx* c) : lk(c->mu) { hipSetDevice(c->device); }
};

constexpr uint32_t kMaxDictElements = 1u << 20;   // a larger dictionary is reset
// a wide namespace (an element past 64 tokens): token slots per element, and the token
// image length its fixed-width templates hold
constexpr uint32_t kWideTokens = 1024, kWideTokenLen = 46;
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

uint64_t al(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

uint64_t wpr_of(int32_t kind, uint32_t E, uint32_t tw = 1) {
    return kind == LASPJ_KIND_ORSET ? 2ull * E * tw : (E + 63ull) / 64ull;
}

// pairs per element slot of a namespace's cells
uint32_t ktw(const KindState& K) { return K.wide ? K.tw : 1u; }

// the payloads [p0, p1) of a call decoded against one dictionary (an image call: the
// context's; a variable call: one per namespace of its variables)
struct Group {
    KindState* K = nullptr;
    uint32_t p0 = 0, p1 = 0;
};

// one NIF-level call over m operand payloads giving n answers
struct Call {
    Op op = Op::MERGE;
    int32_t kind = LASPJ_KIND_ORSET;
    int strict = 0;
    uint32_t n = 0, m = 0;
    std::vector<Group> groups;      // >= 1; single-group ops (all but BIND / WRITE) use [0]
    std::vector<const uint8_t*> p;  // m payloads: MERGE / EQUAL / INFLATION: lhs[0..n) then rhs
    std::vector<uint64_t> len;
    std::vector<const uint8_t*> pre;   // (binds) a payload's pinned copy on the device, or null
    std::vector<laspj_var*> vars;   // variable calls: n variables (payload i -> variable i)
    std::vector<int32_t> st;        // m decode statuses
    std::vector<uint8_t> res;       // n answer bytes (EQUAL / INFLATION / BIND / THRESHOLD)
    std::vector<uint64_t> ooff;     // n + 1 answer payload offsets (MERGE / VALUE / READ)
    const uint8_t* obase = nullptr; // pinned answer payloads
    bool no_defer = false;          // a deferred chain check came back kDecRedo: decode serially
    // a redo pass: the last pass's payloads and cells stay on the device and only these
    // segments are decoded again (their terms registered since, patched into the images)
    SegList redo;
    // a deferred pass that met unknown terms: its segment results (SegRes records, 32 bytes
    // each: status, start, ...) and table, so only the failing segments are registered
    bool has_seg = false;
    std::vector<uint32_t> segres;   // 8 words per segment
    std::vector<uint32_t> segbase;
    uint64_t segS = 0;
    // a single bind / write whose decoder took tokens its namespace had not seen (NewTok):
    // the entries of a pass that decoded, registered by run(); `nt_met`: the pass met some
    // (its cells then hold slots nobody registered unless it decoded)
    std::vector<NewTok> newtoks;
    bool nt_met = false;
    bool no_newtok = false;         // (two payloads gave one slot to different tokens)
    // a merge whose decoders took new tokens: its operands' cells stay on the device and
    // the next pass only joins and writes (the images patched with the tokens first)
    bool write_only = false;
    // launches that ride behind the answer's, ahead of the pass's one synchronisation (every
    // pass of the call runs it again; ctx->mu is held): the read check behind its
    // thresholds' decode (read_pass)
    std::function<int()> tail;
};

// the group payload i belongs to
size_t group_of(const Call& c, uint32_t i) {
    size_t g = 0;
    while (g + 1 < c.groups.size() && i >= c.groups[g].p1) ++g;
    return g;
}

KindState& kstate(NifState* S, int32_t kind) {
    return S->ks[kind == LASPJ_KIND_GSET ? 1 : 0];
}

laspj_batch view(laspj_ctx* ctx, int32_t kind, uint64_t R, uint32_t E, uint64_t* dev,
                 uint32_t tw = 1) {
    laspj_batch b;
    b.ctx = ctx;
    b.kind = kind == LASPJ_KIND_ORSET && tw > 1 ? LASPJ_KIND_ORSET_WIDE : kind;
    b.elements = E;
    b.replicas = R;
    b.words_per_replica = wpr_of(kind, E, tw);
    b.cells = E;
    b.tok_words = kind == LASPJ_KIND_ORSET ? tw : 1;
    b.dev = dev;
    b.owns = false;
    return b;
}

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

void free_etf(KindState& K) {
    if (K.etf) laspj_etf_dict_destroy(K.etf);
    K.etf = nullptr;
    if (K.wd) wide_dict_destroy(K.wd);
    K.wd = nullptr;
    K.E = 0;
}

uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
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

// the namespace takes elements of more than 64 tokens from now on (its cells widen on
// their next use; slots are unchanged, so nothing is written out)
// (false: the namespace stays narrow — its token images are not of one length, which the
// wide templates need)
int spill_lvars(NifState* S, KindState& K);

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
int fit_var(laspj_ctx* ctx, laspj_var* v, uint32_t E, uint32_t tw = 1) {
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

int run(laspj_ctx* ctx, NifState* S, Call& c, std::vector<int32_t>* verdict);

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

// the call's payloads decoded against one dictionary
void one_group(Call& c, KindState* K) { c.groups.assign(1, Group{K, 0, c.m}); }

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

}  // namespace

bool nif_gc_hooks(laspj_ctx* ctx, GcHooks* h) {
    NifState* S = state(ctx);
    if (!S) return false;
    h->mu = &S->mu;
    h->stats = S->stats;
    h->slot = &S->gc;
    return true;
}

namespace {

// A variable whose value sits in its host image (written out by a dictionary reset) gets
// cells again: write/4 of that image.  *ok: the variable is resident over the current
// dictionary (false: it stays host-held; its calls answer FALLBACK)
int hydrate(laspj_ctx* ctx, NifState* S, laspj_var* v, bool* ok) {
    KindState& K = *v->ns;
    *ok = v->resident && v->epoch == K.epoch;
    // (a value write/4 could not represent stays an image until the next write)
    if (*ok || v->image.empty() || v->held) return LASPJ_OK;
    const std::vector<uint8_t> img = v->image;
    Call c;
    c.op = Op::WRITE;
    c.kind = v->kind;
    c.n = c.m = 1;
    c.p.push_back(img.data());
    c.len.push_back(img.size());
    c.vars.push_back(v);
    one_group(c, &K);
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
    auto current = [](const laspj_var* v) { return v->resident && v->epoch == v->ns->epoch; };
    for (uint32_t i = 0; i < n; ++i) {
        // (a decode above may have started a namespace's dictionary afresh and written the
        // cells decoded before it out again: such a variable answers FALLBACK this once)
        laspj_var* v = vars[i];
        bool ok = verdict[i] == LASPJ_NIF_OK && current(v);
        for (const Waiter& w : v->waiters) ok = ok && current(w.cells);
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

}  // namespace

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
        }
        // the list-valued variables' lists go with the context; one outliving it is dead
        for (laspj_lvar* lv : S->lvars) {
            for (laspj_batch** b : {&lv->list, &lv->val, &lv->dst, &lv->tmp}) {
                if (*b) laspj_batch_destroy(*b);
                *b = nullptr;
            }
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
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
    laspj::Call c;
    std::vector<int32_t> v;
    if (int s = pair_call(ctx, S, kind, laspj::Op::MERGE, 0, n, a, na, b, nb, &c, &v)) return s;
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
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
    laspj::Call c;
    std::vector<int32_t> v;
    if (int s = pair_call(ctx, S, kind, op, strict, 1, &a, &na, &b, &nb, &c, &v)) return s;
    *verdict = v[0];
    *result = v[0] == LASPJ_NIF_OK ? (int32_t)(c.res[0] != 0) : 0;
    return LASPJ_OK;
}

// the variable's context state (its S->mu is taken by the caller)
laspj::NifState* var_state(laspj_var* v) {
    if (!v || !v->ctx) return nullptr;
    return laspj::state(v->ctx);
}

int var_image_call(laspj_var* var, bool value, const uint8_t** out, uint64_t* out_len,
                   int32_t* verdict) {
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!out || !out_len || !verdict) return fail(ctx, LASPJ_E_INVAL, "var: null output");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var: unknown variable");
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
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
    laspj::Call c;
    std::vector<int32_t> v;
    if (int st = pair_call(ctx, S, LASPJ_KIND_ORSET, laspj::Op::VALUE, 0, 1, &s, &ns, nullptr,
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

// ---------------------------------------------------------------- resident variables

}  // extern "C"

namespace {

// a variable in namespace `ns` (a fresh one when null); call with S->mu held
int var_new(laspj_ctx* ctx, laspj::NifState* S, int32_t kind,
            std::shared_ptr<laspj::KindState> ns, laspj_var** out) {
    auto* v = new (std::nothrow) laspj_var;
    if (!v) return fail(ctx, LASPJ_E_NOMEM, "var_create: host allocation");
    v->ctx = ctx;
    v->kind = kind;
    try {
        if (!ns) {
            ns = std::make_shared<laspj::KindState>();
            ns->kind = kind;
        }
        v->ns = ns;
        if (!ns->dict && laspj::reset_dict(ctx, S, *ns)) {
            delete v;
            return LASPJ_E_NOMEM;
        }
        v->epoch = ns->epoch;         // new(): no cells until the first call sizes them
        S->vars.insert(v);
        try {
            ns->vars.insert(v);
        } catch (const std::bad_alloc&) {
            S->vars.erase(v);
            throw;
        }
    } catch (const std::bad_alloc&) {
        delete v;
        return fail(ctx, LASPJ_E_NOMEM, "var_create: registry");
    }
    *out = v;
    return LASPJ_OK;
}

// write/4 builds a fresh #dv (lasp_core.erl:842-843): the variable's lazy threads go, their
// hidden cells with them (S->mu held; locked: ctx->mu is held too)
void lazy_clear(laspj::NifState* S, laspj_var* v, bool locked = false) {
    if (v->lazy.empty()) return;
    for (laspj::Lazy& z : v->lazy) {
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

namespace {

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

// the kinds named in a list of variables: bit 0 sets, bit 1 counters
int kinds_of(uint32_t n, laspj_var* const* vars) {
    int k = 0;
    for (uint32_t i = 0; i < n; ++i)
        if (vars[i]) k |= vars[i]->gc ? 2 : 1;
    return k;
}

}  // namespace

extern "C" {

int laspj_var_create(laspj_ctx* ctx, int32_t kind, laspj_var** out) {
    if (!ctx || !out) return LASPJ_E_INVAL;
    *out = nullptr;
    if (kind == LASPJ_KIND_GCOUNTER) return counter_new(ctx, nullptr, out);
    if (kind != LASPJ_KIND_ORSET && kind != LASPJ_KIND_GSET)
        return fail(ctx, LASPJ_E_KIND, "var_create: OR-Set, G-Set or G-Counter variables");
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
    return var_new(ctx, S, kind, nullptr, out);
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
    if (!S->vars.count(peer)) return fail(ctx, LASPJ_E_INVAL, "var_create_replica: unknown variable");
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
        auto drop = [S](laspj_var* c) {
            if (c && c->ctx && S) {
                S->vars.erase(c);
                c->ns->vars.erase(c);
                std::lock_guard<std::mutex> lk2(c->ctx->mu);
                hipSetDevice(c->ctx->device);
                laspj::release_cells(c->ctx, c);
            }
            delete c;
        };
        for (laspj::Waiter& w : v->waiters) drop(w.cells);
        for (laspj::Lazy& z : v->lazy) drop(z.cells);
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
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
    return bind_many_locked(ctx, S, n, vars, values, lens, status, verdict);
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

}  // extern "C"

namespace {

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
    laspj::Call c;
    c.op = laspj::Op::WRITE;
    c.kind = var->kind;
    c.n = c.m = 1;
    c.p.push_back(value);
    c.len.push_back(n);
    c.vars.push_back(var);
    laspj::one_group(c, &K);
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
    try {
        var->image.assign(value, value + n);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "var_write: host image");
    }
    var->resident = false;
    var->held = true;
    drop_cells();
    return LASPJ_OK;
}

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
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
    };
    auto current = [](const laspj_var* v) { return v->resident && v->epoch == v->ns->epoch; };
    // every block of cells the check reads is of its namespace's current dictionary
    auto all_current = [&] {
        for (uint32_t i = 0; i < n; ++i) {
            if (!current(rq[i].var)) return false;
            if ((*hidden)[i] && !current((*hidden)[i])) return false;
            if (rq[i].walk)
                for (const laspj::Lazy& z : rq[i].var->lazy)
                    if (!current(z.cells)) return false;
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
                for (laspj::Lazy& z : v->lazy) {
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
    try {
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
            std::vector<laspj::Lazy>& lz = uniq[v]->lazy;
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
    } catch (const std::bad_alloc&) {
        drop_hidden();
        return fail(ctx, LASPJ_E_NOMEM, "var_read: host allocation");
    }
    return LASPJ_OK;
}

}  // namespace

extern "C" {

int laspj_var_etf_write(laspj_var* var, const uint8_t* value, uint64_t n, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_write(var->gc, value, n, verdict);
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!value && n) || !verdict) return fail(ctx, LASPJ_E_INVAL, "var_write: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_write: unknown variable");
    const int s = var_write_locked(ctx, S, var, value, n, verdict);
    if (s == LASPJ_OK) lazy_clear(S, var);
    return s;
}

int laspj_var_wait(laspj_var* var, const uint8_t* threshold, uint64_t n, int strict, uint64_t id,
                   int32_t* met, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_wait(var->gc, threshold, n, strict, id, met, verdict);
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!threshold && n) || !met || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_wait: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_wait: unknown variable");
    bool ok = false;
    if (int s = laspj::hydrate(ctx, S, var, &ok)) return s;
    *met = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    if (!ok) {
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
    }
    // threshold_met(Type, Value, Threshold) (lasp_lattice.erl:62-75) as
    // laspj_var_etf_threshold answers it; the pass registers the threshold's terms
    {
        laspj::Call c;
        c.op = laspj::Op::THRESHOLD;
        c.kind = var->kind;
        c.strict = strict ? 1 : 0;
        c.n = c.m = 1;
        c.p.push_back(threshold);
        c.len.push_back(n);
        c.vars.push_back(var);
        laspj::one_group(c, var->ns.get());
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
        try {
            laspj::Waiter w;
            w.id = id;
            w.strict = strict ? 1 : 0;
            w.image.assign(threshold, threshold + n);
            w.cells = cells;
            var->waiters.push_back(std::move(w));
            *verdict = LASPJ_NIF_OK;
            return LASPJ_OK;
        } catch (const std::bad_alloc&) {
            s = fail(ctx, LASPJ_E_NOMEM, "var_wait: host allocation");
        }
    }
    waiter_cells_drop(S, cells);
    return s;
}

int laspj_var_recheck(laspj_var* var, uint64_t* ids, uint32_t cap, uint32_t* nmet,
                      uint32_t* nwaiting, int32_t* verdict) {
    if (var && var->gc) return laspj::gc_recheck(var->gc, ids, cap, nmet, nwaiting, verdict);
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!ids && cap) || !nmet || !nwaiting || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_recheck: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_recheck: unknown variable");
    *nmet = 0;
    const int s = recheck_locked(ctx, S, 1, &var, ids, cap, nmet, verdict);
    *nwaiting = (uint32_t)var->waiters.size();
    return s;
}

int laspj_var_recheck_many(laspj_ctx* ctx, uint32_t n, laspj_var* const* vars, uint64_t* ids,
                           uint32_t cap, uint32_t* nmet, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!n) return LASPJ_OK;
    if (!vars || (!ids && cap) || !nmet || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_recheck: null array");
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
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
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!found) return fail(ctx, LASPJ_E_INVAL, "var_wait_cancel: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_wait_cancel: unknown variable");
    *found = 0;
    for (size_t k = 0; k < var->waiters.size(); ++k)
        if (var->waiters[k].id == id) {
            waiter_cells_drop(S, var->waiters[k].cells);
            var->waiters.erase(var->waiters.begin() + (ptrdiff_t)k);
            *found = 1;
            break;
        }
    return LASPJ_OK;
}

int laspj_var_waiter_count(const laspj_var* var, uint32_t* n) {
    if (var && var->gc) return laspj::gc_waiter_count(var->gc, n);
    laspj::NifState* S = var_state(const_cast<laspj_var*>(var));
    if (!S || !n) return LASPJ_E_INVAL;
    std::lock_guard<std::mutex> lk(S->mu);
    *n = (uint32_t)var->waiters.size();
    return LASPJ_OK;
}

int laspj_var_waiter_at(laspj_var* var, uint32_t k, uint64_t* id, int32_t* strict,
                        const uint8_t** threshold, uint64_t* n) {
    if (var && var->gc) return laspj::gc_waiter_at(var->gc, k, id, strict, threshold, n);
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!id || !strict || !threshold || !n)
        return fail(ctx, LASPJ_E_INVAL, "var_waiter_at: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (k >= var->waiters.size()) return fail(ctx, LASPJ_E_RANGE, "var_waiter_at: no waiter %u", k);
    const laspj::Waiter& w = var->waiters[k];
    *id = w.id;
    *strict = w.strict;
    *threshold = w.image.data();
    *n = w.image.size();
    return LASPJ_OK;
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
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!threshold && n) || !needed || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_wait_needed: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_wait_needed: unknown variable");
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
        ++S->stats[laspj::ST_FALLBACKS];
    } else {
        try {
            laspj::Lazy z;
            z.id = id;
            z.image.assign(threshold, threshold + n);
            z.cells = hidden[0];
            var->lazy.push_back(std::move(z));
            return LASPJ_OK;
        } catch (const std::bad_alloc&) {
            s = fail(ctx, LASPJ_E_NOMEM, "var_wait_needed: host allocation");
        }
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
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!threshold && n) || !met || (!lazy_ids && cap) || !nlazy || !nstill_lazy || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_read: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_read: unknown variable");
    const int32_t st = strict ? 1 : 0;
    int32_t found = -1;
    const int s = read_any_locked(ctx, S, 1, &var, &threshold, &n, &st, id, &found, lazy_ids, cap,
                                  nlazy, verdict);
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
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
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
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
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
    laspj::NifState* S = var_state(const_cast<laspj_var*>(var));
    if (!S || !n) return LASPJ_E_INVAL;
    std::lock_guard<std::mutex> lk(S->mu);
    *n = (uint32_t)var->lazy.size();
    return LASPJ_OK;
}

int laspj_var_lazy_at(laspj_var* var, uint32_t k, uint64_t* id, const uint8_t** threshold,
                      uint64_t* n) {
    if (var && var->gc) return LASPJ_E_RANGE;     // a counter keeps none
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!id || !threshold || !n) return fail(ctx, LASPJ_E_INVAL, "var_lazy_at: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (k >= var->lazy.size()) return fail(ctx, LASPJ_E_RANGE, "var_lazy_at: no lazy thread %u", k);
    const laspj::Lazy& z = var->lazy[k];
    *id = z.id;
    *threshold = z.image.data();
    *n = z.image.size();
    return LASPJ_OK;
}

int laspj_var_lazy_cancel(laspj_var* var, uint64_t id, int32_t* found) {
    if (var && var->gc) {
        if (!found) return LASPJ_E_INVAL;
        *found = 0;
        return LASPJ_OK;
    }
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!found) return fail(ctx, LASPJ_E_INVAL, "var_lazy_cancel: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_lazy_cancel: unknown variable");
    *found = 0;
    for (size_t k = 0; k < var->lazy.size(); ++k)
        if (var->lazy[k].id == id) {
            waiter_cells_drop(S, var->lazy[k].cells);
            var->lazy.erase(var->lazy.begin() + (ptrdiff_t)k);
            *found = 1;
            break;
        }
    return LASPJ_OK;
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
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if ((!threshold && n) || !result || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_threshold: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_threshold: unknown variable");
    bool ok = false;
    if (int s = laspj::hydrate(ctx, S, var, &ok)) return s;
    *result = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    if (!ok) return LASPJ_OK;
    laspj::Call c;
    c.op = laspj::Op::THRESHOLD;
    c.kind = var->kind;
    c.strict = strict ? 1 : 0;
    c.n = c.m = 1;
    c.p.push_back(threshold);
    c.len.push_back(n);
    c.vars.push_back(var);
    laspj::one_group(c, var->ns.get());
    std::vector<int32_t> vd;
    if (int s = laspj::run(ctx, S, c, &vd)) return s;
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
        return fail(ctx, LASPJ_E_INVAL, "var_union: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    // OR-Sets of one namespace only: a G-Set's body is `LValue ++ RValue` (a list value),
    // and cells of two namespaces name different terms by one slot
    if (out->kind != LASPJ_KIND_ORSET || l->kind != LASPJ_KIND_ORSET ||
        r->kind != LASPJ_KIND_ORSET || l->ns != out->ns || r->ns != out->ns) {
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
    }
    for (laspj_var* v : {out, l, r}) {
        bool ok = false;
        if (int s = laspj::hydrate(ctx, S, v, &ok)) return s;
        if (!ok) {
            ++S->stats[laspj::ST_FALLBACKS];
            return LASPJ_OK;
        }
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
    laspj::NifState* S = var_state(var);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = var->ctx;
    if (!op || !nop || !result || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "var_update: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(var)) return fail(ctx, LASPJ_E_INVAL, "var_update: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *result = LASPJ_UPDATE_OK;
    *verdict = LASPJ_NIF_FALLBACK;
    if (err_elem) *err_elem = nullptr;
    if (err_len) *err_len = 0;
    if (minted) *minted = nullptr;
    if (nminted) *nminted = 0;
    bool ok = false;
    if (int s = laspj::hydrate(ctx, S, var, &ok)) return s;
    auto fallback = [&] {
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
    };
    if (!ok) return fallback();
    // Type:update(Op, Actor, Value0) (lasp_core.erl:283-287): the op's terms
    std::vector<laspj::UpdateOp> ops;
    const int ps = laspj::parse_update_op(var->kind, op, nop, &ops);
    if (ps == LASPJ_E_NOMEM) return fail(ctx, LASPJ_E_NOMEM, "var_update: host allocation");
    if (ps != LASPJ_DEC_OK || ops.size() > (1u << 24)) return fallback();
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
                return fallback();            // an `==`-equal key under another image
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
            return fallback();
        }
        if (st != LASPJ_DEC_OK) {
            // an `==`-equal term under another image, a token image a wide namespace cannot
            // hold: the reference's clause on the NIF side
            laspj::dict_rollback(K.dict);
            return fallback();
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

// ---------------------------------------------------------------- counters

int laspj_nif_stats(laspj_ctx* ctx, uint64_t* out, uint32_t n) {
    if (!ctx || (n && !out)) return LASPJ_E_INVAL;
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
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
    laspj::NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
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

// ---------------------------------------------------------------- resident processes
// lasp_process:process/3 re-runs (lasp_process.erl:61-95) of the bodies whose outputs stay
// canonical values of the inputs' namespace: filter/6 (lasp_core.erl:681-712) with the fun's
// results kept beside the variable, and the G-Set intersection/7 (:569-576).  The kernels
// are laspj_process.hip's.

namespace {

using laspj::KindState;
using laspj::NifState;
using laspj::ProcDesc;

bool var_current(const laspj_var* v) { return v->resident && v->epoch == v->ns->epoch; }

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

// the elements of a proper list image (131 + the list); a STRING_EXT's bytes stand as empty
// views (small integers: none is `true`)
bool image_list(const uint8_t* p, uint64_t n, std::vector<std::string_view>* out) {
    out->clear();
    if (!p || n < 2 || p[0] != 131 || laspj::list_term_len(p + 1, n - 1) != n - 1) return false;
    const uint8_t* t = p + 1;
    const size_t tn = n - 1;
    if (t[0] == 106) return true;
    if (t[0] == 107) {
        out->assign(((size_t)t[1] << 8) | t[2], std::string_view());
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

hipError_t proc_upload(laspj_ctx* ctx, void* dst, const void* src, uint64_t bytes) {
    if (!bytes) return hipSuccess;
    const void* staged = laspj::stage_small(ctx, src, bytes);
    return hipMemcpyAsync(dst, staged ? staged : src, bytes, hipMemcpyHostToDevice, ctx->stream);
}

// the filter's context state; null: the context is gone
NifState* filter_state(laspj_filter* f) {
    if (!f || !f->ctx) return nullptr;
    return laspj::state(f->ctx);
}

// (S->mu held) the handle is this context's and both its variables are alive
bool filter_alive(const NifState* S, laspj_filter* f) {
    return f && S->filters.count(f) && f->in && f->out;
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
    try {
        f->h_eval.resize(words, 0);
        f->h_keep.resize(words, 0);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "filter: host tables");
    }
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
    // the pending slots (results recorded since the pass taken off) in term order: the
    // order the body calls F in over a canonical value
    std::vector<uint32_t> slots;
    const uint32_t known = K.dict ? laspj::dict_elements(K.dict) : 0;
    for (uint32_t w = 0; w < pm.size(); ++w)
        for (uint64_t m = pm[w] & ~f->h_eval[w]; m; m &= m - 1) {
            const uint32_t e = 64u * w + (uint32_t)__builtin_ctzll(m);
            if (e < known) slots.push_back(e);
        }
    auto img = [&](uint32_t e) { return laspj::list_elem_image(K.dict, e); };
    std::sort(slots.begin(), slots.end(), [&](uint32_t a, uint32_t b) {
        const std::string_view x = img(a), y = img(b);
        int c = 0;
        laspj_term_compare(reinterpret_cast<const uint8_t*>(x.data()), x.size(),
                           reinterpret_cast<const uint8_t*>(y.data()), y.size(), &c);
        return c < 0;
    });
    // F's argument: the element; a G-Set 2-tuple element's first component
    std::vector<std::string_view> items;
    items.reserve(slots.size());
    const bool gset = f->in->kind == LASPJ_KIND_GSET;
    for (uint32_t e : slots) {
        const std::string_view x = img(e);
        const size_t l0 = gset ? first_of_pair(x) : 0;
        items.push_back(l0 ? x.substr(2, l0) : x);
    }
    image_write_list(items, &f->image);
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
        return fail(ctx, LASPJ_E_INVAL, "filter_create: unknown variable");
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
    try {
        S->filters.insert(p);
    } catch (const std::bad_alloc&) {
        delete p;
        return fail(ctx, LASPJ_E_NOMEM, "filter_create: registry");
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
    NifState* S = filter_state(f);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = f->ctx;
    if (!status || !pending || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "filter_run: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!filter_alive(S, f))
        return fail(ctx, LASPJ_E_INVAL, "filter_run: a variable of the filter was destroyed");
    try {
        return filter_run_locked(ctx, S, 1, &f, status, pending, verdict);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "filter_run: host allocation");
    }
}

int laspj_filter_run_many(laspj_ctx* ctx, uint32_t n, laspj_filter* const* fs, int32_t* status,
                          uint32_t* pending, int32_t* verdict) {
    if (!ctx) return LASPJ_E_INVAL;
    if (!n) return LASPJ_OK;
    if (!fs || !status || !pending || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "filter_run: null array");
    NifState* S = laspj::state(ctx);
    if (!S) return fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    std::lock_guard<std::mutex> lk(S->mu);
    try {
        return filter_run_many_locked(ctx, S, n, fs, status, pending, verdict);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "filter_run: host allocation");
    }
}

int laspj_filter_args(laspj_filter* f, const uint8_t** out, uint64_t* out_len, uint32_t* count,
                      int32_t* verdict) {
    NifState* S = filter_state(f);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = f->ctx;
    if (!out || !out_len || !count || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "filter_args: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!filter_alive(S, f))
        return fail(ctx, LASPJ_E_INVAL, "filter_args: a variable of the filter was destroyed");
    ++S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *count = 0;
    try {
        return filter_args_locked(ctx, S, f, out, out_len, count, verdict);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "filter_args: host allocation");
    }
}

int laspj_filter_results(laspj_filter* f, const uint8_t* results, uint64_t n) {
    NifState* S = filter_state(f);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = f->ctx;
    std::lock_guard<std::mutex> lk(S->mu);
    if (!filter_alive(S, f))
        return fail(ctx, LASPJ_E_INVAL, "filter_results: a variable of the filter was destroyed");
    ++S->stats[laspj::ST_CALLS];
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
    try {
        parsed = image_list(results, n, &res);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "filter_results: host allocation");
    }
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
        return fail(ctx, LASPJ_E_INVAL, "var_intersection: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    auto fallback = [&] {
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
    };
    // G-Sets of one namespace only: the OR-Set body's `Cx ++ Cy` is a list value, and cells
    // of two namespaces name different terms by one slot
    if (out->kind != LASPJ_KIND_GSET || l->kind != LASPJ_KIND_GSET ||
        r->kind != LASPJ_KIND_GSET || l->ns != out->ns || r->ns != out->ns)
        return fallback();
    for (laspj_var* v : {out, l, r}) {
        bool ok = false;
        if (int s = laspj::hydrate(ctx, S, v, &ok)) return s;
        if (!ok) return fallback();
    }
    for (laspj_var* v : {out, l, r})
        if (!var_current(v)) return fallback();
    KindState& K = *out->ns;
    // a 2-tuple element goes down the body's OR-Set branch (keyfind, then ++ on a causality
    // that is no list): the reference's to run, as on the image path
    if (ns_has_pair(K)) return fallback();
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

// ---------------------------------------------------------------- list-valued variables
// include/laspj.h "list-valued resident variables": a `#dv.value` that is any list of
// {Key, [{Token, Bool}]}, kept as a LIST batch over the slots of a laspj_var namespace.  The
// list kernels are laspj_lists.hip's; the order tables and the producer of intersection/7's
// OR-Set branch (lasp_core.erl:559-568, 583) are laspj_lvars.hip's.

namespace laspj {
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

int spill_lvars(NifState* S, KindState& K) {
    for (laspj_lvar* lv : K.lvars)
        if (int s = lvar_spill(S, lv)) return s;
    return LASPJ_OK;
}

// what a walk registered in the namespace: the device images are stale from here on
struct RegMark {
    uint32_t n = 0;
    uint64_t tb = 0;
};
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

// the tables as the list entry points take them (the bufs are views, never destroyed)
struct LvOrder {
    laspj_buf kb, gb;
    laspj_list_order o{};
    LvOrder(laspj_ctx* ctx, const KindState& K) {
        kb.ctx = gb.ctx = ctx;
        kb.dev = K.krank;
        kb.bytes = K.krank_bytes;
        gb.dev = K.grank;
        gb.bytes = K.grank_bytes;
        o.krank = &kb;
        o.nkeys = K.rank_E;
        o.grank = &gb;
        o.ntokens = 64u * K.rank_E;
    }
};

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

// images and tables ready for a list kernel over the namespace (S->mu held, ctx->mu not)
int lvar_prepare(laspj_ctx* ctx, NifState* S, KindState& K) {
    if (K.dict && dict_elements(K.dict) > 0)
        if (int s = lvar_images(ctx, S, K)) return s;
    Guard g(ctx);
    return lvar_ranks(ctx, S, K);
}

// bind/3 (lasp_core.erl:291-312) of lv->val into the variable: laspj_list_bind's status; the
// merge becomes the variable's list by a swap of the two batches when it is written
int lvar_bind(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, int32_t* status) {
    const LvOrder ord(ctx, *lv->ns);
    uint8_t st = 0;
    const uint64_t t0 = now_ns();
    if (int s = laspj_list_bind(ctx, lv->dst, lv->list, lv->val, &ord.o, &st)) return s;
    ++S->stats[ST_PASSES];
    S->stats[ST_NS_WAIT] += now_ns() - t0;
    if (st == 1) std::swap(lv->list, lv->dst);
    *status = st;
    return LASPJ_OK;
}

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

// laspj_lvar_intersection with S->mu held and the handles checked
int lvar_intersection_locked(laspj_ctx* ctx, NifState* S, laspj_lvar* out, laspj_var* l,
                             laspj_var* r, int32_t* status, int32_t* verdict) {
    ++S->stats[ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    auto fallback = [&] {
        ++S->stats[ST_FALLBACKS];
        return LASPJ_OK;
    };
    // OR-Sets of the list's namespace only: cells of another namespace name other terms
    if (l->kind != LASPJ_KIND_ORSET || r->kind != LASPJ_KIND_ORSET || l->ns != out->ns ||
        r->ns != out->ns)
        return fallback();
    KindState& K = *out->ns;
    if (K.wide) return fallback();
    for (laspj_var* v : {l, r}) {
        bool ok = false;
        if (int s = hydrate(ctx, S, v, &ok)) return s;
        if (!ok) return fallback();
    }
    bool ok = false;
    if (int s = lvar_ready(ctx, S, out, &ok)) return s;
    // (a decode above may have widened the namespace or started its dictionary afresh)
    if (!ok || K.wide || !var_current(l) || !var_current(r) || out->epoch != K.epoch)
        return fallback();
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
    if (int s = lvar_bind(ctx, S, out, &st)) return s;
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

}  // namespace
}  // namespace laspj

namespace {

// the variable's context state; null: the context is gone
laspj::NifState* lvar_state(laspj_lvar* lv) {
    if (!lv || !lv->ctx) return nullptr;
    return laspj::state(lv->ctx);
}

// (S->mu held) the handle is a live list variable of this context
bool lvar_alive(const laspj::NifState* S, laspj_lvar* lv) { return lv && S->lvars.count(lv); }

void lvar_free_batches(laspj_lvar* lv) {
    for (laspj_batch** b : {&lv->list, &lv->val, &lv->dst, &lv->tmp}) {
        if (*b) laspj_batch_destroy(*b);
        *b = nullptr;
    }
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
    laspj::NifState* S = var_state(peer);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = peer->ctx;
    std::lock_guard<std::mutex> lk(S->mu);
    if (!S->vars.count(peer)) return fail(ctx, LASPJ_E_INVAL, "lvar_create: unknown variable");
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
    try {
        S->lvars.insert(lv);
        try {
            lv->ns->lvars.insert(lv);
        } catch (const std::bad_alloc&) {
            S->lvars.erase(lv);
            throw;
        }
    } catch (const std::bad_alloc&) {
        lvar_free_batches(lv);
        delete lv;
        return fail(ctx, LASPJ_E_NOMEM, "lvar_create: registry");
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
    laspj::NifState* S = lvar_state(out);
    if (!S || !l || !r) return LASPJ_E_INVAL;
    laspj_ctx* ctx = out->ctx;
    if (!status || !verdict) return fail(ctx, LASPJ_E_INVAL, "lvar_intersection: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, out)) return fail(ctx, LASPJ_E_INVAL, "lvar_intersection: unknown variable");
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    if (l->gc || r->gc || l->ctx != ctx || r->ctx != ctx || !S->vars.count(l) || !S->vars.count(r)) {
        // a counter, a variable of another context: nothing this body runs over
        ++S->stats[laspj::ST_CALLS];
        ++S->stats[laspj::ST_FALLBACKS];
        return LASPJ_OK;
    }
    try {
        return laspj::lvar_intersection_locked(ctx, S, out, l, r, status, verdict);
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "lvar_intersection: host allocation");
    }
}

int laspj_lvar_etf_bind(laspj_lvar* lv, const uint8_t* value, uint64_t n, int32_t* status,
                        int32_t* verdict) {
    laspj::NifState* S = lvar_state(lv);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = lv->ctx;
    if (!value || !n || !status || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "lvar_bind: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, lv)) return fail(ctx, LASPJ_E_INVAL, "lvar_bind: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *status = LASPJ_BIND_NOOP;
    *verdict = LASPJ_NIF_FALLBACK;
    try {
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (ok)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, value, n, &ok)) return s;
        if (!ok) {
            ++S->stats[laspj::ST_FALLBACKS];
            return LASPJ_OK;
        }
        int32_t st = 0;
        if (int s = laspj::lvar_bind(ctx, S, lv, &st)) return s;
        *status = st;
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "lvar_bind: host allocation");
    }
}

int laspj_lvar_etf_write(laspj_lvar* lv, const uint8_t* value, uint64_t n, int32_t* verdict) {
    laspj::NifState* S = lvar_state(lv);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = lv->ctx;
    if (!value || !n || !verdict) return fail(ctx, LASPJ_E_INVAL, "lvar_write: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, lv)) return fail(ctx, LASPJ_E_INVAL, "lvar_write: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *verdict = LASPJ_NIF_FALLBACK;
    try {
        laspj::KindState& K = *lv->ns;
        bool ok = false;
        if (!K.wide)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, value, n, &ok)) return s;
        if (!ok) {
            // held as its image: read answers it, the other calls FALLBACK until a write
            lv->image.assign(value, value + n);
            lv->resident = false;
            lv->held = true;
            ++S->stats[laspj::ST_FALLBACKS];
            return LASPJ_OK;
        }
        std::swap(lv->list, lv->val);
        lv->resident = true;
        lv->held = false;
        lv->epoch = K.epoch;
        lv->image.clear();
        *verdict = LASPJ_NIF_OK;
        return LASPJ_OK;
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "lvar_write: host allocation");
    }
}

int laspj_lvar_etf_read(laspj_lvar* lv, const uint8_t** out, uint64_t* out_len,
                        int32_t* verdict) {
    laspj::NifState* S = lvar_state(lv);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = lv->ctx;
    if (!out || !out_len || !verdict) return fail(ctx, LASPJ_E_INVAL, "lvar_read: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, lv)) return fail(ctx, LASPJ_E_INVAL, "lvar_read: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *verdict = LASPJ_NIF_OK;
    try {
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
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "lvar_read: host allocation");
    }
}

int laspj_lvar_etf_value(laspj_lvar* lv, const uint8_t** out, uint64_t* out_len,
                         int32_t* verdict) {
    laspj::NifState* S = lvar_state(lv);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = lv->ctx;
    if (!out || !out_len || !verdict) return fail(ctx, LASPJ_E_INVAL, "lvar_value: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, lv)) return fail(ctx, LASPJ_E_INVAL, "lvar_value: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *out = nullptr;
    *out_len = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    try {
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (!ok) {
            ++S->stats[laspj::ST_FALLBACKS];
            return LASPJ_OK;
        }
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
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "lvar_value: host allocation");
    }
}

int laspj_lvar_etf_threshold(laspj_lvar* lv, const uint8_t* threshold, uint64_t n, int strict,
                             int32_t* result, int32_t* verdict) {
    laspj::NifState* S = lvar_state(lv);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = lv->ctx;
    if (!threshold || !n || !result || !verdict)
        return fail(ctx, LASPJ_E_INVAL, "lvar_threshold: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, lv)) return fail(ctx, LASPJ_E_INVAL, "lvar_threshold: unknown variable");
    ++S->stats[laspj::ST_CALLS];
    *result = 0;
    *verdict = LASPJ_NIF_FALLBACK;
    try {
        bool ok = false;
        if (int s = laspj::lvar_ready(ctx, S, lv, &ok)) return s;
        if (ok)
            if (int s = laspj::lvar_walk_val(ctx, S, lv, threshold, n, &ok)) return s;
        if (!ok) {
            ++S->stats[laspj::ST_FALLBACKS];
            return LASPJ_OK;
        }
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
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "lvar_threshold: host allocation");
    }
}

int laspj_lvar_counts(laspj_lvar* lv, uint32_t* entries, uint32_t* tokens) {
    laspj::NifState* S = lvar_state(lv);
    if (!S) return LASPJ_E_INVAL;
    laspj_ctx* ctx = lv->ctx;
    if (!entries || !tokens) return fail(ctx, LASPJ_E_INVAL, "lvar_counts: null argument");
    std::lock_guard<std::mutex> lk(S->mu);
    if (!lvar_alive(S, lv)) return fail(ctx, LASPJ_E_INVAL, "lvar_counts: unknown variable");
    if (!(lv->resident && lv->epoch == lv->ns->epoch))
        return fail(ctx, LASPJ_E_UNSUPPORTED, "lvar_counts: the value is held as its image");
    uint32_t cnt[2] = {0, 0};
    if (int s = laspj_list_counts(ctx, lv->list, cnt)) return s;
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
