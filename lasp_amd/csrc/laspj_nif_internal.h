// What the NIF-level translation units share (laspj_nif.hip and laspj_nif_{vars,waiters,
// process,lvars,maps}.hip): the per-context state, a call's description, the functions one file
// defines and another calls (each with the lock its caller holds), and the opening, the
// allocation guard and the FALLBACK ending the entry points have in common.
#pragma once

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

struct laspj_map;
struct laspj_fold;

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
    // the map processes over this dictionary (laspj_map): patch_etf hands each the slots it
    // rewrote — elements that gained tokens, which the map then names under its keys before
    // its next pass — and rebuild_etf says "all"
    std::unordered_set<laspj_map*> maps;
    // the fold processes (laspj_fold), handed the same slots
    std::unordered_set<laspj_fold*> folds;
};

// One entry of `#dv.waiting_threads` ({threshold, read, From, Type, Threshold},
// lasp_core.erl:331-364): the threshold decoded once into `cells`, a hidden variable of the
// waiting variable's namespace (registered where variables are, so widening, growth and a
// dictionary reset carry it along), and its image as registered.
// An entry of `#dv.lazy_threads` ({threshold, wait, From, Type, Threshold},
// lasp_core.erl:730-758) is kept the same way, always with strict == 0.  (The bare-pid entry
// of :744-746 cannot be reached for the set types: threshold_met(Type, Value, undefined)
// ahead of it raises.)
struct Waiter {
    uint64_t id = 0;
    int32_t strict = 0;
    std::vector<uint8_t> image;
    laspj_var* cells = nullptr;
};

// One entry of a list-valued variable's `#dv.waiting_threads`: the threshold walked once over
// the variable's namespace into a one-replica OR-Set LIST batch of its own (its items are
// slots, so the namespace growing leaves it alone), and its image as registered.  `list` is
// null while the threshold is not on the device: a dictionary reset made its items stale
// (walked back in from the image at the variable's next waiter call; `epoch` names the
// generation the items refer to) or the namespace went wide (it stays out).
struct LWaiter {
    uint64_t id = 0;
    int32_t strict = 0;
    std::vector<uint8_t> image;
    laspj_batch* list = nullptr;
    uint32_t n = 0;                  // the threshold's entries
    uint64_t epoch = 0;
};
// An entry of a list variable's `#dv.lazy_threads` ({threshold, wait, From, Type, Threshold},
// lasp_core.erl:730-758) is kept the same way, always with strict == 0, and follows the same
// rules across growth, a dictionary reset and a widening.

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
    std::vector<laspj::Waiter> lazy;      // `#dv.lazy_threads`, in list order
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
    bool pairs = false;              // pair-keyed (laspj_lvar_create_pairs): every image of it
                                     // is walked by list_walk_pairs, for its whole life
    laspj_batch* list = nullptr;
    laspj_batch* val = nullptr;
    laspj_batch* dst = nullptr;
    laspj_batch* tmp = nullptr;      // l's list form (the two-step composition, A/B only)
    std::vector<uint8_t> image;
    std::vector<laspj::LWaiter> waiters;   // `#dv.waiting_threads`, in list order
    std::vector<laspj::LWaiter> lazy;      // `#dv.lazy_threads`, in list order
};

// One lasp_process running map/6 (lasp_core.erl:641-667) from the OR-Set `in` into the list
// variable `out` (include/laspj.h "resident map processes").  Per element slot e of the
// namespace: whether F has been asked (evaluated), the element slot F(X) took (ymap) and, per
// token slot k of e, the slot the token's image holds under ymap[e] (tmap, 0xFF: not mapped).
// On the device (dev: [rec {pending, unmapped} | evaluated | pmask | ymap | tmap], over E
// slots) with all but pmask mirrored on the host, where laspj_map_results and the token
// fan-out edit them; rows that changed are uploaded ahead of the next pass.
struct laspj_map {
    laspj_ctx* ctx = nullptr;        // null once the context is gone
    laspj_var* in = nullptr;         // null once in or out is destroyed: the map is dead
    laspj_lvar* out = nullptr;       // and its calls answer LASPJ_E_INVAL
    std::shared_ptr<laspj::KindState> ns;
    uint64_t epoch = 0;              // the dictionary generation the tables refer to
    uint32_t E = 0, words = 0;       // the slots the device tables cover
    uint8_t* dev = nullptr;
    uint64_t dev_bytes = 0;
    std::vector<uint64_t> h_eval;
    std::vector<uint32_t> h_ymap;
    std::vector<uint8_t> h_tmap;     // 64 per slot
    // per slot: the token slots this map's own registrations created under it (the images
    // of some input's tokens: never tokens of that element in `in`, so not mapped onwards),
    // and how many of its tokens have been looked at
    std::vector<uint64_t> h_mine;
    std::vector<uint8_t> h_seen;
    // mirror rows the device has not got yet: the slots whose evaluated bit / ymap changed
    // (as a range) and the slots whose tmap row changed
    uint32_t up_lo = ~0u, up_hi = 0;
    std::vector<uint32_t> up_rows;
    bool pmask_valid = false;        // pmask is a pass's of this generation and size
    bool rec_dirty = true;           // rec is not known zero (a pass without its writer)
    bool refused = false;            // until the next dictionary reset: FALLBACK
    bool val_not_asc = false;        // the produced list's keys do not ascend (F's order)
    // the element slots whose tokens grew since the last look (patch_etf), or all of them
    std::vector<uint32_t> tok_dirty;
    bool tok_all = true;
    // laspj_map_args' list, as the filter's
    std::vector<uint32_t> listed;
    bool outstanding = false, dropped = false;
    std::string image;
};

// One lasp_process running fold/6 (lasp_core.erl:460-486) from the OR-Set `in` into the list
// variable `out` (include/laspj.h "resident fold processes").  F(X) is a list, so a slot owns
// a run of rows of a pool appended in the order slots are evaluated: per element slot e
// whether F has been asked (evaluated), its run (frow: first row | count << 32) and the token
// slots mapped in every row of the run (fmapped); per row the element slot V took (ykey) and,
// per token slot k of e, the slot the token's image holds under that key (tmap, 0xFF: not
// mapped).  On the device (dev: [rec {pending, unmapped} | evaluated | pmask | frow | fmapped
// | ykey | tmap], over E slots and row_cap rows) with all but pmask mirrored on the host;
// what changed is uploaded ahead of the next pass.
struct laspj_fold {
    laspj_ctx* ctx = nullptr;        // null once the context is gone
    laspj_var* in = nullptr;         // null once in or out is destroyed: the fold is dead
    laspj_lvar* out = nullptr;       // and its calls answer LASPJ_E_INVAL
    std::shared_ptr<laspj::KindState> ns;
    uint64_t epoch = 0;              // the dictionary generation the tables refer to
    uint32_t E = 0, words = 0;       // the slots the device tables cover
    uint32_t row_cap = 0;            // the rows the device pool has room for
    uint32_t rows_up = 0;            // the rows the device pool has got
    uint8_t* dev = nullptr;
    uint64_t dev_bytes = 0;
    std::vector<uint64_t> h_eval;
    std::vector<uint64_t> h_frow, h_fmapped;     // per slot
    std::vector<uint32_t> h_ykey;                // per row
    std::vector<uint8_t> h_tmap;                 // 64 per row
    // per slot, as the map's: the token slots this fold's own registrations created under it
    // and how many of its tokens have been looked at
    std::vector<uint64_t> h_mine;
    std::vector<uint8_t> h_seen;
    // sum over slots of rows x tokens looked at: the bound of a pass's tokens
    uint64_t sum_rt = 0;
    // mirror entries the device has not got yet: the slots whose evaluated bit / frow changed
    // (as a range), the slots whose fmapped word and the old rows whose tmap row changed
    uint32_t up_lo = ~0u, up_hi = 0;
    std::vector<uint32_t> up_slots, up_rows;
    bool pmask_valid = false;        // pmask is a pass's of this generation and size
    bool rec_dirty = true;           // rec is not known zero (a pass without its writer)
    bool refused = false;            // until the next dictionary reset: FALLBACK
    bool val_not_asc = false;        // the produced list's keys do not ascend (F's order)
    // the element slots whose tokens grew since the last look (patch_etf), or all of them
    std::vector<uint32_t> tok_dirty;
    bool tok_all = true;
    // laspj_fold_args' list, as the filter's
    std::vector<uint32_t> listed;
    bool outstanding = false, dropped = false;
    std::string image;
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
    // the product's side arrays (laspj_lvar_product: per side the held slots, the exclusive
    // token prefix, the runs in term order and each token's owner position)
    void* lp_side = nullptr;
    uint64_t lp_side_bytes = 0;
    std::unordered_set<laspj_map*> maps;         // the live map processes
    std::unordered_set<laspj_fold*> folds;       // the live fold processes
};

enum class Op { MERGE, VALUE, EQUAL, INFLATION, BIND, WRITE, THRESHOLD, READ, VVALUE };

struct Guard {
    std::lock_guard<std::mutex> lk;
    explicit Guard(laspj_ctx* c) : lk(c->mu) { hipSetDevice(c->device); }
};

inline uint64_t al(uint64_t x, uint64_t a) { return (x + a - 1) & ~(a - 1); }

inline uint64_t wpr_of(int32_t kind, uint32_t E, uint32_t tw = 1) {
    return kind == LASPJ_KIND_ORSET ? 2ull * E * tw : (E + 63ull) / 64ull;
}

// pairs per element slot of a namespace's cells
inline uint32_t ktw(const KindState& K) { return K.wide ? K.tw : 1u; }

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

inline laspj_batch view(laspj_ctx* ctx, int32_t kind, uint64_t R, uint32_t E, uint64_t* dev,
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

inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch()).count();
}

inline bool var_current(const laspj_var* v) { return v->resident && v->epoch == v->ns->epoch; }

// ---- laspj_nif.hip ----------------------------------------------------------------------
// the context's NIF state, made on first use (null: no memory); taken without ctx->mu
NifState* state(laspj_ctx* ctx);
// a device / a pinned block grown to `need` bytes (ctx->mu held)
int grow_dev(laspj_ctx* ctx, void** p, uint64_t* have, uint64_t need);
int grow_host(laspj_ctx* ctx, void** p, uint64_t* have, uint64_t need);
// the pinned staging grown to the two regions (ctx->mu held)
int fit_staging(laspj_ctx* ctx, NifState* S, uint64_t in_bytes, uint64_t out_bytes);
// the namespace takes elements past 64 tokens from now on (S->mu held; false: it stays narrow)
bool go_wide(NifState* S, KindState& K);
// the device images rebuilt, or patched in place (false: rebuild); S->mu held, ctx->mu not
int rebuild_etf(laspj_ctx* ctx, NifState* S, KindState& K);
bool patch_etf(laspj_ctx* ctx, NifState* S, KindState& K);
// a variable's cells given back, or widened to E slots of tw pairs (ctx->mu held)
void release_cells(laspj_ctx* ctx, laspj_var* v);
int fit_var(laspj_ctx* ctx, laspj_var* v, uint32_t E, uint32_t tw = 1);
// the call's payloads decoded against one dictionary
void one_group(Call& c, KindState* K);
// a call of one payload on one variable, decoded against the variable's namespace
inline Call var_call(Op op, laspj_var* v, const uint8_t* p, uint64_t n, int strict = 0) {
    Call c;
    c.op = op;
    c.kind = v->kind;
    c.strict = strict;
    c.n = c.m = 1;
    c.p.push_back(p);
    c.len.push_back(n);
    c.vars.push_back(v);
    one_group(c, v->ns.get());
    return c;
}
// the dictionary started afresh, its variables written out first (S->mu held, ctx->mu not)
int reset_dict(laspj_ctx* ctx, NifState* S, KindState& K);
// the call: passes and registrations; verdict[j] per answer (S->mu held, ctx->mu not)
int run(laspj_ctx* ctx, NifState* S, Call& c, std::vector<int32_t>* verdict);
// a namespace's dictionary and device images dropped, the context still alive (S->mu held)
void free_ns(KindState& K);

// ---- laspj_nif_vars.hip -----------------------------------------------------------------
// the variable's context state (null: its context is gone); the caller takes its S->mu
NifState* var_state(laspj_var* v);
// a variable in namespace `ns` (a fresh one when null); S->mu held
int var_new(laspj_ctx* ctx, NifState* S, int32_t kind, std::shared_ptr<KindState> ns,
            laspj_var** out);
// a host-held value decoded back; *ok: it is resident now (S->mu held, ctx->mu not)
int hydrate(laspj_ctx* ctx, NifState* S, laspj_var* v, bool* ok);
// write/4 of one image into the variable (S->mu held, ctx->mu not)
int var_write_locked(laspj_ctx* ctx, NifState* S, laspj_var* var, const uint8_t* value,
                     uint64_t n, int32_t* verdict);
// the variable's lazy threads and their hidden cells go (S->mu held; locked: ctx->mu too)
void lazy_clear(NifState* S, laspj_var* v, bool locked = false);
// the kinds named in a list of variables: bit 0 sets, bit 1 counters
int kinds_of(uint32_t n, laspj_var* const* vars);

// ---- laspj_nif_waiters.hip --------------------------------------------------------------
// a waiter's hidden variable leaves the registries and the device (S->mu held, ctx->mu not)
void waiter_cells_drop(NifState* S, laspj_var* c);

// ---- laspj_nif_lvars.hip ----------------------------------------------------------------
// the namespace's resident lists written out to their images (S->mu held, ctx->mu not)
int spill_lvars(NifState* S, KindState& K);
// a list variable's waiter gives its device list back, its image stays (the context alive)
void lwaiter_release(LWaiter& w);
// write/4 builds a fresh #dv (lasp_core.erl:842-843): the list variable's lazy threads go
void llazy_clear(laspj_lvar* lv);
// what a call registered in the namespace since `before`: the device images are stale
struct RegMark {
    uint32_t n = 0;
    uint64_t tb = 0;
};
RegMark reg_mark(const KindState& K);
void reg_note(NifState* S, KindState& K, const RegMark& before);
// the namespace's device images brought up to its dictionary (S->mu held, ctx->mu not; at
// least one element registered); the order tables derived from them, fully or for the
// patched slots (ctx->mu held)
int lvar_images(laspj_ctx* ctx, NifState* S, KindState& K);
int lvar_ranks(laspj_ctx* ctx, NifState* S, KindState& K);
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
// *ok: the variable's list is on the device over the current dictionary (S->mu held)
int lvar_ready(laspj_ctx* ctx, NifState* S, laspj_lvar* lv, bool* ok);
// the producers' scratch: tile sums (S->lv_tiles) and pinned totals (S->lv_ans); ctx->mu held
int lvar_scratch(laspj_ctx* ctx, NifState* S, uint32_t ntile);

// ---- laspj_nif_process.hip --------------------------------------------------------------
// a small upload through the staging ring (larger ones straight from `src`), enqueued
hipError_t proc_upload(laspj_ctx* ctx, void* dst, const void* src, uint64_t bytes);
// the elements of a proper list image (131 + the list); a STRING_EXT's bytes stand as empty
// views, or — bytes given — as SMALL_INTEGER_EXT images built there
bool image_list(const uint8_t* p, uint64_t n, std::vector<std::string_view>* out,
                std::string* bytes = nullptr);
// laspj_filter_args' list for a process over K: the slots of pm (a check pass's pending
// words) without a result in h_eval, in term order (*slots), and the image of their
// arguments' list (pair_first: a 2-tuple element gives its first component)
void proc_args_image(const KindState& K, const std::vector<uint64_t>& pm,
                     const std::vector<uint64_t>& h_eval, bool pair_first,
                     std::vector<uint32_t>* slots, std::string* image);

// ---- laspj_nif_maps.hip -----------------------------------------------------------------
// a variable / a list variable / the context goes: the maps naming it are dead from here on
// (S->mu and ctx->mu held)
void maps_var_gone(NifState* S, laspj_var* v);
void maps_lvar_gone(NifState* S, laspj_lvar* lv);
void maps_ctx_gone(laspj_ctx* ctx, NifState* S);

// ---- laspj_nif_folds.hip ----------------------------------------------------------------
// the same for the folds
void folds_var_gone(NifState* S, laspj_var* v);
void folds_lvar_gone(NifState* S, laspj_lvar* lv);
void folds_ctx_gone(laspj_ctx* ctx, NifState* S);

// ---- what the entry points open and close with ------------------------------------------
// An entry point's opening: the handle's context state, the null-argument check, the call
// lock, the membership test — in that order.  rc != LASPJ_OK is the call's answer (the error
// text is set); else S->mu is held for as long as the Entry lives.
struct Entry {
    NifState* S = nullptr;
    laspj_ctx* ctx = nullptr;
    std::unique_lock<std::mutex> lk;
    int rc = LASPJ_E_INVAL;
};

// the first three steps (S null: the handle is null or its context is gone)
inline Entry enter(NifState* S, laspj_ctx* ctx, const char* name, bool args_ok) {
    Entry e;
    if (!S) return e;
    e.S = S;
    e.ctx = ctx;
    if (!args_ok) {
        e.rc = fail(ctx, LASPJ_E_INVAL, "%s: null argument", name);
        return e;
    }
    e.lk = std::unique_lock<std::mutex>(S->mu);
    e.rc = LASPJ_OK;
    return e;
}

// a call on the context itself: its state made on first use, then the call lock
inline Entry enter_ctx(laspj_ctx* ctx) {
    Entry e = enter(state(ctx), ctx, "nif", true);
    if (!e.S) e.rc = fail(ctx, LASPJ_E_NOMEM, "nif: state allocation");
    return e;
}

// the membership test's answer
inline int unknown_variable(laspj_ctx* ctx, const char* name) {
    return fail(ctx, LASPJ_E_INVAL, "%s: unknown variable", name);
}

// all four steps for a set variable
inline Entry enter_var(laspj_var* v, const char* name, bool args_ok) {
    Entry e = enter(var_state(v), v ? v->ctx : nullptr, name, args_ok);
    if (e.rc == LASPJ_OK && !e.S->vars.count(v)) e.rc = unknown_variable(e.ctx, name);
    return e;
}

// fn's answer; a host allocation that failed inside it answers LASPJ_E_NOMEM
template <class F>
int nomem_guard(laspj_ctx* ctx, const char* name, F&& fn, const char* what = "host allocation") {
    try {
        return fn();
    } catch (const std::bad_alloc&) {
        return fail(ctx, LASPJ_E_NOMEM, "%s: %s", name, what);
    }
}

// the reference's own clause runs on the NIF side (the caller has set the verdict)
inline int fallback(NifState* S) {
    ++S->stats[ST_FALLBACKS];
    return LASPJ_OK;
}

}  // namespace laspj
