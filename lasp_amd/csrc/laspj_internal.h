// Internal definitions shared by the liblaspj translation units (not installed).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <mutex>
#include <string>
#include <string_view>
#include <vector>

#include "../../include/laspj.h"
#include "../../include/laspj_tune.h"

namespace laspj {
struct NifState;                       // laspj_nif_internal.h
struct ListEtfState;                   // laspj_list_etf.cpp
void nif_destroy(laspj_ctx* ctx);      // call without ctx->mu held
}  // namespace laspj

struct laspj_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    std::mutex mu;
    std::string err;
    int cus = 256;
    // tuning knobs (LASPJ_TUNE_*); 0 = default
    int64_t tune_grid = 0;
    int64_t tune_unroll = 0;
    int64_t tune_nt = -1;
    int64_t tune_etf = 0;
    int64_t tune_etf_read = 0;
    int64_t tune_etf_seg = 0;
    int64_t tune_etf_occ = 0;        // segment decoders: 1 = filled form, 2 = under-filled
    int64_t tune_reduce = 0;
    int64_t tune_product_rows = 0;
    int64_t tune_product_cols = 0;
    int64_t tune_list_walk = 0;
    int64_t tune_nif_passes = 0;     // NIF device passes per call (0: the default)
    int64_t tune_list_chunk = 0;     // rows per chunk of the chunked list walk (0: default)
    int64_t tune_lvar = 0;           // laspj_lvar_intersection: 1 = the two-step composition
    // device scratch for apply_ops (grown on demand)
    void* scratch = nullptr;
    uint64_t scratch_bytes = 0;
    // one device word for kernel-detected argument violations (product token slots)
    uint32_t* flag = nullptr;
    // per-replica partial records of segmented reductions (grown on demand)
    void* partials = nullptr;
    uint64_t partials_bytes = 0;
    // list kernels' scratch (merge plans, key-order arrays, hash tables, sizes)
    void* lscratch = nullptr;
    uint64_t lscratch_bytes = 0;
    // list_bind's keyfind tables, kept zeroed between calls (each call's last kernel zeroes
    // what it used), so a bind needs no memset of them; dirty: a call may have left them used
    void* ltab = nullptr;
    uint64_t ltab_bytes = 0;
    bool ltab_dirty = false;
    // list_bind's per-call words (device, kept zeroed between calls by the call's last
    // block, as ltab) and its answer (pinned, coherent: the last block writes it there)
    void* lbind = nullptr;
    uint64_t lbind_bytes = 0;
    bool lbind_dirty = false;
    void* lbind_h = nullptr;
    void* lbind_hd = nullptr;       // its device address
    uint64_t lbind_h_bytes = 0;
    // list_bind's rank-indexed path (both lists strictly ascending): per-call words and
    // look-back states (kept zeroed between calls as lbind), and the rank -> entry index
    // maps, tagged with the call's epoch so they are never cleared (0 never valid)
    void* lfz = nullptr;            // two halves: a call's words, the previous call's
    uint64_t lfz_bytes = 0;
    bool lfz_dirty = false;
    uint32_t lf_parity = 0;         // the half the last call used
    uint64_t lf_prev_use = 0;       // the bytes of it that call used (the next one zeroes them)
    void* lfi = nullptr;
    uint64_t lfi_bytes = 0;
    uint32_t lf_epoch = 0;
    // the list variables' waiter check (list_waiters_*): the value's keyfind table, the
    // waiters' flag words and the error word (device, zeroed by each pass's one memset; a
    // copy of the descriptors behind them when the pinned ring cannot hold them), and the
    // answers (pinned, coherent: the finish launch writes the met bytes there)
    void* lw_dev = nullptr;
    uint64_t lw_dev_bytes = 0;
    void* lw_h = nullptr;
    void* lw_hd = nullptr;          // its device address
    uint64_t lw_h_bytes = 0;
    // the list merges' chunked walk (k_merge_spec): per-replica round and chunk words,
    // kept zeroed between calls by the kernel's last block per replica
    void* lspec = nullptr;
    uint64_t lspec_bytes = 0;
    bool lspec_dirty = false;
    // laspj_ctx_last_list_walk: what the last list merge / union / bind did with it
    // (0 not launched, 1 launched, 2 a replica fell back to the one-wave walk)
    int last_list_walk = 0;
    // laspj_batch_bind_many_host's statuses (pinned, coherent: the kernel writes them there)
    void* many_h = nullptr;
    void* many_hd = nullptr;
    uint64_t many_h_bytes = 0;
    // pinned host staging for the small readbacks (sizes, statuses, flags): a round trip
    // into pageable memory costs ~26 us, into pinned ~13 us (tools/readback_probe.py)
    void* pinned = nullptr;
    // pinned staging for device dictionary images (laspj_etf_dict_create), grow-only: the
    // NIF path rebuilds its image whenever a call registers new terms
    void* dstage = nullptr;
    uint64_t dstage_bytes = 0;
    // pinned ring for small laspj_buf_upload calls: the bytes copied in and the copy
    // enqueued without waiting (the stream orders every later use; the ring synchronises
    // the stream when it wraps)
    void* upring = nullptr;
    uint64_t upring_at = 0;
    const uint8_t* upring_dev = nullptr;   // the ring's device address (kernels read it)
    static constexpr uint64_t kUpRing = 1 << 20, kUpSmall = 64 * 1024;
    static constexpr uint64_t kPinned = 64 * 1024;
    // released device blocks by size class (laspj::dev_alloc / dev_release): every kernel
    // runs on `stream`, so a block released after its last enqueued use can serve the
    // next allocation without waiting — no hipFree (a device-wide synchronisation) and
    // no hipMalloc on the bind path's short-lived lists and buffers
    std::map<uint64_t, std::vector<void*>> cache;
    uint64_t cached_bytes = 0;
    // the NIF-level entry points' dictionary, staging and scratch (laspj_nif.hip)
    laspj::NifState* nif = nullptr;
    // the list-image entry points' dictionary and scratch (laspj_list_etf.cpp)
    laspj::ListEtfState* listetf = nullptr;
};

struct laspj_buf {
    laspj_ctx* ctx = nullptr;
    void* dev = nullptr;
    uint64_t bytes = 0;
    // the device address was handed out (laspj_buf_device_ptr): work on other streams may
    // still use the block, so its release synchronises the device first
    mutable bool exported = false;
};

struct laspj_batch {
    laspj_ctx* ctx = nullptr;
    int32_t kind = 0;
    uint32_t elements = 0;      // E
    uint64_t replicas = 0;      // R
    uint64_t words_per_replica = 0;  // u64 words: 2E (OR-Set) or ceil(E/64) (G-Set) ...
    uint32_t elements_r = 0;    // ER of product batches
    uint64_t cells = 0;         // cells per replica: E, or EL*ER for products
    uint32_t tok_words = 1;     // {p, r} pairs per cell (LASPJ_KIND_ORSET_WIDE), else 1
    uint64_t* dev = nullptr;
    bool owns = true;           // false for laspj_batch_wrap
    mutable bool exported = false;  // laspj_batch_device_ptr handed out the address
    // LASPJ_KIND_*_LIST: entry / token capacity per replica (laspj_lists.hip)
    uint32_t cap_e = 0;
    uint32_t cap_t = 0;
    // list batches: every replica holds at most known_e entries and known_t tokens (kept
    // on the host by the operations that write lists, so a merge can size its output
    // without reading the inputs' counts back)
    uint32_t known_e = 0;
    uint32_t known_t = 0;
    // list batches, a hint only: list_bind found some replica's keys not strictly ascending
    // (or product pairs) — its rank-indexed path is not tried again until the list is
    // rewritten (upload, or a merge / bind writing it)
    mutable bool not_asc = false;
    // (a hint too) a merge of this list's keys with another's took the one-wave walk after
    // the chunked walk's walks did not meet: the next merge goes to the one-wave walk
    mutable bool no_spec = false;
};

inline bool laspj_is_list(int32_t kind) {
    return kind == LASPJ_KIND_ORSET_LIST || kind == LASPJ_KIND_GSET_LIST;
}

struct laspj_event {
    laspj_ctx* ctx = nullptr;
    hipEvent_t ev = nullptr;
};

namespace laspj {

int fail(laspj_ctx* ctx, int code, const char* fmt, ...);

inline uint64_t bytes_of(const laspj_batch* b) { return b->replicas * b->words_per_replica * 8ull; }

// Device -> host copies of up to a few pieces in one synchronisation, staged through the
// context's pinned buffer when they fit (laspj_runtime.hip).  Returns a hipError_t.
struct ReadPiece {
    void* host;
    const void* dev;
    uint64_t bytes;
};
hipError_t readback(laspj_ctx* ctx, const ReadPiece* pieces, int n);

// Device blocks through the context's cache (laspj_runtime.hip).  Blocks up to
// kCacheMax are rounded to a power of two and reused in stream order; larger ones go to
// hipMalloc / hipFree directly.  Call with the context's mutex held.
constexpr uint64_t kCacheMax = 256ull << 20;      // largest cached block
constexpr uint64_t kCacheCap = 2ull << 30;        // bytes a context keeps cached
hipError_t dev_alloc(laspj_ctx* ctx, uint64_t bytes, void** out);
// src copied into the context's pinned ring for a stream-ordered host -> device copy with
// no wait (<= 64 KiB; null: not staged).  Call with ctx->mu held.
const void* stage_small(laspj_ctx* ctx, const void* src, uint64_t bytes);
// the device address of a stage_small slot (kernels read staged bytes in place), or null
const void* staged_dev(const laspj_ctx* ctx, const void* slot);
// hipMalloc that gives the context's cached blocks back and retries once when it fails
// (every long-lived scratch allocation goes through it)
hipError_t dev_malloc(laspj_ctx* ctx, void** out, uint64_t bytes);
void dev_release(laspj_ctx* ctx, void* p, uint64_t bytes);
void dev_cache_clear(laspj_ctx* ctx);
inline hipError_t readback(laspj_ctx* ctx, void* host, const void* dev, uint64_t bytes) {
    const ReadPiece p{host, dev, bytes};
    return readback(ctx, &p, 1);
}

#define LJ_HIP(ctx, call)                                                              \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            return ::laspj::fail((ctx), LASPJ_E_DEVICE, "%s: %s (%s:%d)", #call,        \
                                 hipGetErrorString(e_), __FILE__, __LINE__);           \
    } while (0)

#define LJ_LAUNCHED(ctx)                                                               \
    do {                                                                               \
        hipError_t e_ = hipGetLastError();                                             \
        if (e_ != hipSuccess)                                                          \
            return ::laspj::fail((ctx), LASPJ_E_DEVICE, "kernel launch: %s (%s:%d)",   \
                                 hipGetErrorString(e_), __FILE__, __LINE__);           \
    } while (0)

// Launch wrappers implemented in laspj_kernels.hip.  All take validated shapes.
struct StreamTune {
    int grid;
    int unroll;
    bool nt;
};
StreamTune stream_tune(const laspj_ctx* ctx, uint64_t n16);

hipError_t launch_or(laspj_ctx* ctx, uint64_t* dst, const uint64_t* a, const uint64_t* b,
                     uint64_t words);
hipError_t launch_max(laspj_ctx* ctx, uint64_t* dst, const uint64_t* a, const uint64_t* b,
                      uint64_t words);
hipError_t launch_reduce_max(laspj_ctx* ctx, uint64_t* dst, const uint64_t* src,
                             uint64_t groups, uint32_t group, uint64_t wr);
hipError_t launch_gcounter_sums(laspj_ctx* ctx, const laspj_batch* b, uint64_t* sums);
hipError_t launch_gcounter_threshold(laspj_ctx* ctx, const laspj_batch* b, uint64_t t,
                                     bool strict, uint8_t* out);
hipError_t launch_gcounter_inflation(laspj_ctx* ctx, const laspj_batch* prev,
                                     const laspj_batch* cur, bool strict, uint8_t* out);
hipError_t launch_gcounter_incr(laspj_ctx* ctx, laspj_batch* b, const laspj_incr* incs,
                                uint64_t n);
// max_join: per-word unsigned max (G-Counter counts) instead of OR (set bitmaps)
hipError_t launch_reduce_chunks(laspj_ctx* ctx, uint64_t* dst, const uint64_t* src,
                                uint64_t words, uint32_t nchunks, bool max_join);
hipError_t launch_reduce_ptrs(laspj_ctx* ctx, uint64_t* dst, const uint64_t* const* srcs,
                              uint32_t nsrc, uint64_t words, bool max_join);
hipError_t launch_reduce_or(laspj_ctx* ctx, uint64_t* dst, const uint64_t* src,
                            uint64_t groups, uint32_t group, uint64_t words_per_replica);
hipError_t launch_fill_synthetic(laspj_ctx* ctx, laspj_batch* b, uint64_t seed,
                                 uint64_t replica_base, uint64_t tmask = ~0ull);
hipError_t launch_orset_fragment(laspj_ctx* ctx, const laspj_batch* b, uint32_t e, void* out);
hipError_t launch_orset_context(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src);
// head / next: the key chains of the KEYED form (laspj_orset_gather_inflation_keyed), or null
hipError_t launch_gather_inflation(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src,
                                   const uint32_t* index, const uint32_t* head,
                                   const uint32_t* next, const laspj_batch* prev, bool strict,
                                   uint8_t* res);
hipError_t launch_orset_value(laspj_ctx* ctx, const laspj_batch* b, uint64_t* out,
                              bool removed);
hipError_t launch_orset_stats(laspj_ctx* ctx, const laspj_batch* b, uint64_t* out);
hipError_t launch_gset_stats(laspj_ctx* ctx, const laspj_batch* b, uint64_t* out);
hipError_t launch_equal(laspj_ctx* ctx, const laspj_batch* a, const laspj_batch* b,
                        uint8_t* out);
hipError_t launch_orset_inflation(laspj_ctx* ctx, const laspj_batch* prev,
                                  const laspj_batch* cur, bool strict, uint8_t* out);
hipError_t launch_gset_inflation(laspj_ctx* ctx, const laspj_batch* prev,
                                 const laspj_batch* cur, bool strict, uint8_t* out);
hipError_t launch_apply_ops(laspj_ctx* ctx, laspj_batch* b, const laspj_op* ops,
                            uint64_t nops, int32_t* status);
hipError_t launch_orset_union(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* l,
                              const laspj_batch* r);
hipError_t launch_orset_filter(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src,
                               const uint64_t* keep);
hipError_t launch_orset_intersection(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* l,
                                     const laspj_batch* r);
hipError_t launch_orset_product(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* l,
                                const laspj_batch* r, uint32_t* flag);
hipError_t launch_orset_product_diag(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* l,
                                     const laspj_batch* r, uint32_t* flag);
hipError_t launch_orset_gather(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src,
                               const uint32_t* index);
hipError_t launch_and(laspj_ctx* ctx, uint64_t* dst, const uint64_t* a, const uint64_t* b,
                      uint64_t words);
// LASPJ_KIND_ORSET_WIDE (laspj_wide.hip)
hipError_t launch_wide_value(laspj_ctx* ctx, const laspj_batch* b, uint64_t* out, bool removed);
hipError_t launch_wide_stats(laspj_ctx* ctx, const laspj_batch* b, uint64_t* out);
hipError_t launch_wide_inflation(laspj_ctx* ctx, const laspj_batch* prev, const laspj_batch* cur,
                                 bool strict, uint8_t* out);
hipError_t launch_wide_apply(laspj_ctx* ctx, laspj_batch* b, const laspj_op* ops, uint64_t nops,
                             int32_t* status);
hipError_t launch_wide_widen(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src);
hipError_t launch_gset_filter(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src,
                              const uint64_t* keep);
hipError_t launch_gset_product(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* l,
                               const laspj_batch* r);
hipError_t launch_gset_gather(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* src,
                              const uint32_t* index);


// ---- wire codec, enqueue-only forms (laspj_codec.hip) -----------------------------------
// For callers that hold ctx->mu and know the payload offsets on the host (the NIF-level
// entry points, laspj_nif.hip): no readbacks, no synchronisation — a decode -> join ->
// encode chain then costs one host round trip.  Pointers are device addresses.
struct EtfReadPlan {
    uint64_t S = 0, nseg = 0;               // segment bytes / count (0: a wave per payload)
    std::vector<uint32_t> segbase;          // R + 1 when nseg
};
bool etf_dict_decodable(const laspj_etf_dict* d);     // from_binary runs on the device
uint32_t etf_dict_elements(const laspj_etf_dict* d);
void etf_read_plan(const laspj_ctx* ctx, const laspj_etf_dict* d, uint64_t R,
                   const unsigned long long* host_offsets, EtfReadPlan* plan);
// A segment-mode decode whose chain check is left to the join (etf_merge_size_enqueue):
// the caller gives `res` (device memory, kSegResBytes per segment: ctx->scratch is reused
// by the join); etf_read_enqueue fills the rest and sets `armed` when it decoded in
// segments.  The statuses then come from the join's launch; kDecRedo = the chain broke
// before any failing segment: decode that call again without deferring.
constexpr uint64_t kSegResBytes = 32;
// a redo pass's segments (global segment numbers; n = 0: every segment): the segments of a
// deferred pass that met terms since registered, decoded again over the cells they left
// A single payload's tokens its namespace has not seen, taken by the decoder on the spot
// (binary tokens of the dictionary's token length on known elements): each gets the next
// free slot of its element (the element's token count, then one up per new token in
// payload order — one wave decodes an element, so no two waves hand out its slots) and
// an entry {seq, element slot, token slot, image offset} in `out`, numbered by the device
// counter `cnt`; the host registers them in slot order after the call (the dictionary's
// own numbering: count, count + 1, ...).  An entry past `cap`, a slot past 63, or two new
// tokens whose order the decoder cannot tell answer UNKNOWN_TERM as before.
struct NewTok {
    uint32_t seq, e, slot, off;
};
struct NewTokArgs {
    uint32_t* cnt = nullptr;
    NewTok* out = nullptr;
    uint32_t cap = 0, seq = 0;
};

struct SegList {
    uint32_t n = 0;
    uint32_t g[31] = {};
};
constexpr int32_t kDecRedo = 64;
struct ChainJob {
    void* res = nullptr;
    const uint8_t* payload = nullptr;
    const unsigned long long* offs = nullptr;
    const uint32_t* segbase = nullptr;
    int32_t* status = nullptr;
    uint32_t nrep = 0, S = 0;
    bool armed = false;
    void* hres = nullptr;      // (or null) host-visible copy of a failed payload's results
};
// segbase: plan.segbase already on the device, or null (uploaded here); clear: zero the
// batch first (the decoders only set the cells they decode)
// redo_zeroed: R + 1 words the caller has zeroed (segment mode's redo list), or null
int etf_read_enqueue(laspj_ctx* ctx, laspj_batch* b, const laspj_etf_dict* d, int tag, int vers,
                     const uint8_t* payload, uint64_t payload_bytes,
                     const unsigned long long* offsets, const EtfReadPlan& plan,
                     const uint32_t* segbase, int32_t* status, bool clear,
                     uint32_t* redo_zeroed, ChainJob* defer = nullptr,
                     const SegList* only = nullptr, const NewTokArgs* nt = nullptr);
// every token template of the dictionary a BINARY_EXT of the record's length (the new-token
// decode compares such images bytewise, which is their term order)
bool etf_dict_bin_tokens(const laspj_etf_dict* d);
uint32_t etf_dict_tok_len(const laspj_etf_dict* d);      // the uniform token image length
// OR-Set payloads over several dictionaries decoded in one launch (the NIF's binds of many
// variables, one token namespace each): group k's payloads [p0, p1) against dictionary d
// into cells (its first payload's; E slots per replica, consecutive).  The caller stages
// etf_multi_bytes of tables (etf_multi_fill: false when some dictionary cannot take the
// shared launch — decode group by group then; host null: that check only) and hands their
// device copy to
// etf_read_multi_enqueue; offsets are every payload's (absolute), the plan and segbase
// are over all payloads (etf_read_plan with any of the dictionaries); cells are not
// cleared (the caller's are zero); defer as etf_read_enqueue's
struct EtfGroup {
    const laspj_etf_dict* d;
    uint32_t p0, p1;
    uint64_t* cells;
    uint32_t E;
};
uint64_t etf_multi_bytes(uint32_t ngroups, uint32_t npay);
bool etf_multi_fill(const laspj_ctx* ctx, const EtfGroup* g, uint32_t ngroups, uint32_t npay,
                    void* host);
int etf_read_multi_enqueue(laspj_ctx* ctx, const EtfGroup* g, uint32_t ngroups,
                           const void* dev_tabs, uint32_t npay, const uint8_t* payload,
                           uint64_t payload_bytes, const unsigned long long* offs,
                           const EtfReadPlan& plan, const uint32_t* segbase, int32_t* status,
                           ChainJob* defer, const SegList* only = nullptr);
// lasp_gset:from_binary/1's decoder (k_gset_etf_read: one wave per payload), enqueue only;
// offsets / status are device addresses; clear: zero the batch first
int gset_read_enqueue(laspj_ctx* ctx, laspj_batch* b, const laspj_etf_dict* d, int tag, int vers,
                      const uint8_t* payload, const unsigned long long* offsets, int32_t* status,
                      bool clear,
                      const unsigned long long* hoffs = nullptr);
// merge/2 of a[i] and b[i] into z fused with z's size pass (and a, b cleared behind it),
// when etf_merge_fused(ctx, R, E) holds; ticket: one zeroed word (left zero)
bool etf_merge_fused(const laspj_ctx* ctx, uint64_t R, uint32_t E);
int etf_merge_size_enqueue(laspj_ctx* ctx, uint64_t* a, uint64_t* b, const laspj_batch* z,
                           const laspj_etf_dict* d, int tag, unsigned long long* offsets,
                           uint32_t* flag, uint32_t* ticket, const unsigned long long** chunks,
                           const ChainJob* chain = nullptr);
// the NIF's single merge (R == 1): join, size pass and writer in ONE launch
// (k_orset_etf_write_rec's look-back form), when etf_merge_write_one holds; lbst: a zeroed
// word per 256-element chunk, ticket: a zeroed word (left zero), offs_out: {0, total}
// (total > cap: nothing written), chain: the deferred chain checks ride along; skip (or
// null): a device word the decoders set when they took unseen tokens (NewTok) — then
// nothing is written, {0, 0} answered and the operands kept
bool etf_merge_write_one(const laspj_ctx* ctx, const laspj_etf_dict* d, uint64_t R, uint32_t E);
int etf_merge_write_enqueue(laspj_ctx* ctx, uint64_t* a, uint64_t* b, uint32_t E,
                            const laspj_etf_dict* d, int tag, int vers,
                            unsigned long long* offs_out, uint8_t* out, uint64_t cap_bytes,
                            unsigned long long* lbst, uint32_t* ticket, const ChainJob* chain,
                            const uint32_t* skip = nullptr);
// lasp_core:bind/3 (write = false) / write/4 (write = true) of n resident variables: curs /
// ins / wprs (device arrays of n: the variable's cells, its decoded operand's cells — left
// zero — and their width in words; maxw the widest), dstat (n decode statuses: read, or —
// chain armed — written from the deferred chain check), diff (n zeroed words) and ticket
// (a zeroed word) left zero; out_res / out_st (n bytes / n int32, pinned) get the bind
// statuses and decode statuses
int var_bind_enqueue(laspj_ctx* ctx, uint64_t* const* curs, uint64_t* const* ins,
                     const uint64_t* wprs, uint64_t maxw, uint32_t n, int32_t* dstat,
                     uint32_t* diff, uint32_t* ticket, uint8_t* out_res, int32_t* out_st,
                     bool write, const ChainJob* chain);
// offsets: R + 1 (offsets[R] = total); flag: set when a present slot has no image (the
// caller zeroes it); *chunks: the split-mode chunk offsets etf_write_enqueue can reuse
// (valid until the context's scratch is next used), or null
int etf_size_enqueue(laspj_ctx* ctx, const laspj_batch* b, const laspj_etf_dict* d, int32_t kind,
                     int tag, unsigned long long* offsets, uint32_t* flag,
                     const unsigned long long** chunks);
// writes nothing when offsets[R] > cap (the caller reads offsets[R] back and re-sizes)
int etf_write_enqueue(laspj_ctx* ctx, const laspj_batch* b, const laspj_etf_dict* d,
                      int32_t kind, int tag, int vers, const unsigned long long* offsets,
                      uint8_t* out, uint64_t cap, const unsigned long long* chunks);
// value/1 of an OR-Set batch written as G-Set images straight from its cells (size pass,
// offsets and writer; few long payloads: etf_value_direct); zero_cells clears the cells
// behind the reads (even when the answer does not fit)
bool etf_value_direct(const laspj_ctx* ctx, uint64_t R, uint32_t E);
// lasp_gset:merge/2 of few long pairs written from both operands' bits (their OR never
// stored); the same condition as etf_value_direct
int etf_gset_merge_write_enqueue(laspj_ctx* ctx, const laspj_batch* lhs, const laspj_batch* rhs,
                                 const laspj_etf_dict* d, int tag, int vers,
                                 unsigned long long* offsets, uint32_t* flag, uint8_t* out,
                                 uint64_t cap);
// chain: the segment decoder's chain check deferred onto the size pass (as the merge's)
int etf_value_write_enqueue(laspj_ctx* ctx, const laspj_batch* cells, const laspj_etf_dict* d,
                            int tag, int vers, unsigned long long* offsets, uint32_t* flag,
                            uint8_t* out, uint64_t cap, bool zero_cells,
                            const ChainJob* chain = nullptr);

// laspj_etf_dict_create with per-element token headroom (up to tok_headroom more tokens
// per element than the widest has) and the host state etf_dict_patch needs, over arrays
// laspj_dict_export wrote (consistent by construction: the per-slot checks are skipped)
int etf_dict_create_ex(laspj_ctx* ctx, uint32_t E, const uint8_t* elem_blob,
                       const uint32_t* elem_off, const uint32_t* elem_order,
                       const uint8_t* tok_blob, const uint32_t* tok_off, const uint8_t* tok_order,
                       uint32_t tok_headroom, laspj_etf_dict** out);
// rewrite the device rows of element slots that gained tokens in the host dictionary
// (call without ctx->mu held); LASPJ_E_UNSUPPORTED: rebuild instead (nothing written)
int etf_dict_patch(laspj_ctx* ctx, laspj_etf_dict* d, const laspj_dict* hd,
                   const uint32_t* dirty, uint32_t n);
// host dictionary (laspj_host.cpp): element slots, tokens of a slot, its images and their
// term order (order[j] = slot of the j-th smallest)
uint32_t dict_elements(const laspj_dict* dict);
uint32_t dict_token_count(const laspj_dict* dict, uint32_t e);
uint32_t dict_max_tokens(const laspj_dict* dict);   // most tokens of one element (upper bound)
// laspj_dict_encode with tw {p, r} pairs per OR-Set element (a wide namespace's cells)
int dict_encode_cells(const laspj_dict* dict, int32_t kind, const uint8_t* blob,
                      const uint64_t* offsets, uint64_t n, int tag, uint32_t E, uint32_t tw,
                      uint64_t* out, int32_t* status);
// the element slots that gained tokens since the last call (repeats possible), cleared
void dict_take_dirty(laspj_dict* dict, std::vector<uint32_t>* out);
bool dict_tokens(const laspj_dict* dict, uint32_t e, std::vector<std::string_view>* imgs,
                 std::vector<uint8_t>* order);
// register the terms of the OR-Set payload elements that start in [from, to) (from: an
// element's first byte); a DEC status (the range's registrations undone on failure)
int dict_add_elems(laspj_dict* dict, const uint8_t* p, size_t n, size_t from, size_t to);
// update/3's Op (lasp_orset.erl:101-117, lasp_gset.erl:84-88) read from its image (131 +
// the term), flattened in application order: {add, E} / {add_all, Es} (one ADD per element,
// `mint` for an OR-Set: unique/1 mints its token), {add_by_token, T, E}, {remove, E},
// {remove_all, Es}, {update, Ops}.  LASPJ_DEC_MALFORMED: no clause of the reference's update
// takes it as written (the NIF runs the reference's, which raises)
struct UpdateOp {
    uint8_t kind = 0;            // LASPJ_OP_ADD / LASPJ_OP_REMOVE
    bool mint = false;
    std::string elem, tok;       // term images (no version byte); tok empty when minted
};
int parse_update_op(int32_t kind, const uint8_t* img, size_t n, std::vector<UpdateOp>* ops);
// the element slot of an image, -1 when absent, -2 when a term `==` to it holds a slot
// under another image (or the term is outside this path); single registrations inside a
// journal that
// dict_rollback undoes (LASPJ_DEC_* statuses as laspj_dict_add's)
int64_t dict_find_elem(const laspj_dict* dict, const uint8_t* img, size_t n);
void dict_begin(laspj_dict* dict);
void dict_rollback(laspj_dict* dict);
int dict_reg_elem(laspj_dict* dict, const uint8_t* img, size_t n, uint32_t* slot);
int dict_reg_tok(laspj_dict* dict, uint32_t e, const uint8_t* img, size_t n, uint32_t* slot);
// token slots per element (64 by default; a wide namespace's 64 k)
// token slots per element (64: the narrow cells); max_len > 0: from now on every token image
// has the length of the first (at most max_len) — false when those registered already differ
bool dict_set_tok_cap(laspj_dict* dict, uint32_t cap, uint32_t max_len = 0);
uint32_t dict_tok_cap(const laspj_dict* dict);
// a wide namespace's dictionary for its device tables: element images by slot (eblob /
// eoff) and slots in term order (eorder); per element slot e the tokens in term order,
// ranks rb[e] .. rb[e+1): rslot = the rank's token slot, its image tblob[toff[r] ..
// toff[r+1]); max_cnt = the most tokens any element holds
struct WideExport {
    std::vector<uint8_t> eblob, tblob;
    std::vector<uint32_t> eoff, eorder, rb, toff;
    std::vector<uint16_t> rslot;
    uint32_t max_cnt = 0;
};
int dict_export_wide(const laspj_dict* dict, WideExport* x);

// ---- wide namespaces (laspj_codec.hip): device tables of a dictionary whose elements may
// hold up to 64 tw tokens, cells of tw {p, r} pairs per element slot; LASPJ_E_UNSUPPORTED
// for token images of several lengths (or longer than 46 bytes)
struct WideDict;
int wide_dict_create(laspj_ctx* ctx, const WideExport& x, uint32_t tw, WideDict** out);
void wide_dict_destroy(WideDict* w);
uint32_t wide_elements(const WideDict* w);
// the answers' size pass and writer, enqueue only (offsets, out: device addresses); a wide
// namespace's operands are encoded on the host (dict_encode_cells)
int wide_size_enqueue(laspj_ctx* ctx, const WideDict* w, const uint64_t* cells, uint64_t R,
                      int tag, unsigned long long* offsets, uint32_t* flag);
int wide_write_enqueue(laspj_ctx* ctx, const WideDict* w, const uint64_t* cells, uint64_t R,
                       int tag, int vers, const unsigned long long* offsets, uint8_t* out,
                       uint64_t cap);
// dst (en x tn pairs) := src (eo x to pairs) re-laid, the rest {0, 0}; src may be null
hipError_t launch_relay(laspj_ctx* ctx, uint64_t* dst, const uint64_t* src, uint32_t eo,
                        uint32_t to, uint32_t en, uint32_t tn);


// ---- list values as images (laspj_host.cpp; used by laspj_list_etf.cpp) ---------------
// A list value as the list kernels take it (include/laspj.h "list values"): key items
// (element slot, or a pair {X, Y}: bit 62, x << 31 | y), each entry's token run
// toks[toff[i], toff[i+1]) (token g = 64 e + k, bit 63 the flag; bit 62: a pair [Tx, Ty])
struct ListItems {
    std::vector<uint64_t> keys;
    std::vector<uint32_t> toff;      // keys.size() + 1
    std::vector<uint64_t> toks;
};
// walk a term_to_binary image (131 + a list; OR-Set: of {Key, [{Token, Bool}]}, G-Set:
// of elements, in any order, duplicates kept) into items, registering its terms (the
// registrations undone when it fails); args (optional): per entry the slot of the fun's
// argument (the key; a G-Set 2-tuple element's first component).  A LASPJ_DEC_* status,
// or LASPJ_E_NOMEM
int list_walk(laspj_dict* dict, int32_t kind, const uint8_t* p, size_t n, ListItems* it,
              std::vector<uint32_t>* args);
// list_walk in pair mode (a pair-keyed list variable's images, include/laspj.h): 131 + a list
// of {{X, Y}, [{[Tx, Ty], Bool}]} — X and Y registered as elements, Tx as a token of X, Ty as
// a token of Y; key items bit 62 | x << 31 | y, token items bit 62 | gx << 31 | gy | flag.
// Anything else (a key that is no 2-tuple, a token that is no proper 2-list: LIST_EXT of two
// with a NIL tail, or STRING_EXT of two) is refused as list_walk refuses, registrations undone
int list_walk_pairs(laspj_dict* dict, const uint8_t* p, size_t n, ListItems* it);
// register one term image (no version byte) as an element; a LASPJ_DEC_* status
int list_register(laspj_dict* dict, const uint8_t* img, size_t n, uint32_t* slot);
std::string_view list_elem_image(const laspj_dict* dict, uint32_t e);
std::string_view list_tok_image(const laspj_dict* dict, uint64_t g);
size_t list_term_len(const uint8_t* p, size_t n);
uint32_t list_dict_elements(const laspj_dict* dict);
// dense term-order ranks: krank per element slot, grank per token g (64 per slot)
int list_ranks(const laspj_dict* dict, std::vector<uint32_t>* krank, std::vector<uint32_t>* grank);
// items -> 131 + the list as term_to_binary/1 writes it
int list_write(const laspj_dict* dict, int32_t kind, const ListItems& it, std::string* out);
void list_etf_destroy(laspj_ctx* ctx);     // laspj_list_etf.cpp; call without ctx->mu held

// ---- riak_dt_gcounter variables (laspj_counter_host.cpp, laspj_counters.hip) -----------
// A counter variable is one row of uint64 counts over the actor slots of its namespace (a
// host dictionary of element terms only, append-only); 0 = the actor is absent.
constexpr uint32_t kGcMaxActors = 1u << 20;      // a namespace holds at most this many
// one {Actor, Count} of an image as the kernels take it (16 bytes: one vector load)
struct GcPair {
    uint64_t count;
    uint32_t slot;
    uint32_t pad;
};
// the image [{Actor, Count}] (131 + the orddict) walked into pairs in list order, its
// unseen actors registered; a LASPJ_DEC_* status (not OK: every registration of the call
// undone through the dictionary's journal, no pairs) or LASPJ_E_NOMEM
int gc_parse(laspj_dict* dict, const uint8_t* p, size_t n, std::vector<GcPair>* out);
// pairs in term order -> 131 + the orddict as term_to_binary/1 writes it (zero counts skipped)
void gc_encode(const laspj_dict* dict, const GcPair* pairs, size_t n, std::string* out);
// a non-negative integer as term_to_binary/1 encodes it (97 / 98 / 110)
void gc_put_uint(std::string* o, uint64_t v);
// threshold_met(riak_dt_gcounter, V, T) (lasp_lattice.erl:87-90) planned from T's image:
// LASPJ_GC_NEVER / LASPJ_GC_ALWAYS / LASPJ_GC_T with *t (`*t =< value(V)`), -1: not a term
int gc_threshold_plan(const uint8_t* p, size_t n, bool strict, uint64_t* t);

struct GcVar;                                    // laspj_counters.hip
struct GcState;                                  // a context's counter variables and staging
// what the counter path shares with the set path's state (laspj_nif_internal.h): the context's
// call lock, its laspj_nif_stats counters and the slot its GcState hangs from
struct GcHooks {
    std::mutex* mu = nullptr;
    uint64_t* stats = nullptr;
    GcState** slot = nullptr;
};
bool nif_gc_hooks(laspj_ctx* ctx, GcHooks* h);
// the entry points of include/laspj.h on a counter variable (each takes the call lock)
int gc_var_create(laspj_ctx* ctx, GcVar* peer, GcVar** out);
laspj_ctx* gc_var_ctx(const GcVar* v);
int gc_var_destroy(GcVar* v);
int gc_bind_many(laspj_ctx* ctx, uint32_t n, GcVar* const* vars, const uint8_t* const* values,
                 const uint64_t* lens, int32_t* status, int32_t* verdict);
int gc_write(GcVar* v, const uint8_t* value, uint64_t n, int32_t* verdict);
int gc_read(GcVar* v, bool value, const uint8_t** out, uint64_t* out_len, int32_t* verdict);
int gc_threshold(GcVar* v, const uint8_t* threshold, uint64_t n, int strict, int32_t* result,
                 int32_t* verdict);
int gc_resident(const GcVar* v, int32_t* resident);
int gc_refuse(GcVar* v, int32_t* verdict);       // update / union: FALLBACK, counted
int gc_wait(GcVar* v, const uint8_t* threshold, uint64_t n, int strict, uint64_t id,
            int32_t* met, int32_t* verdict);
int gc_recheck(GcVar* v, uint64_t* ids, uint32_t cap, uint32_t* nmet, uint32_t* nwaiting,
               int32_t* verdict);
// recheck_many's two halves, call lock held by the caller (counters and sets together):
// every waiter of the n counters checked (one device pass at most), nmet[i] / verdict[i]
// answered and nothing removed; then the met ones' ids written in argument order and removed
int gc_recheck_check(laspj_ctx* ctx, uint32_t n, GcVar* const* vars, uint32_t* nmet,
                     int32_t* verdict);
void gc_recheck_take(GcVar* v, uint64_t* ids);
int gc_wait_cancel(GcVar* v, uint64_t id, int32_t* found);
int gc_waiter_count(const GcVar* v, uint32_t* n);
int gc_waiter_at(GcVar* v, uint32_t k, uint64_t* id, int32_t* strict, const uint8_t** threshold,
                 uint64_t* n);
int gc_increment(GcVar* v, const uint8_t* op, uint64_t nop, const uint8_t* actor, uint64_t nactor,
                 uint64_t* ids, uint32_t cap, uint32_t* nmet, uint32_t* nwaiting,
                 int32_t* verdict);
uint64_t gc_dict_elements(const GcState* G);     // laspj_nif_stats [7]'s share
// laspj_nif_reset (call lock held): rows written out to images, namespaces started afresh
int gc_ctx_reset(laspj_ctx* ctx, GcState* G);
// the context goes (call lock held, ctx->mu not): rows released, variables orphaned
void gc_ctx_destroy(laspj_ctx* ctx, GcState* G);

// ---- lasp_process re-runs over resident variables (laspj_process.hip) --------------------
// One process of a pass: filter/6 (lasp_core.erl:681-712) — in's cells masked by keep, the
// slots in holds and evaluated does not counted pending — or the G-Set intersection/7
// (:569-576: keep = r's bitmap, evaluated null: nothing is ever pending).  n: element slots
// (OR-Sets, tw {p, r} pairs each) or bitmap words (kProcGset); the bitmaps hold a bit per
// element slot; pmask (or null): n's worth of bitmap words the check pass fills with the
// pending slots.  out may be in.
constexpr uint32_t kProcNarrow = 0, kProcWide = 1, kProcGset = 2;
struct ProcDesc {
    const uint64_t* in;
    uint64_t* out;
    const uint64_t* keep;
    const uint64_t* evaluated;
    uint64_t* pmask;
    uint32_t n, tw, mode;
    uint32_t block0;                // its first block of a launch over many
};
static_assert(sizeof(ProcDesc) == 56, "descriptor layout");
// kProcCheck: rec {pending, changed} (zeroed by the caller) and pmask written, no cell
// touched; kProcWrite: out |= AccValue where rec says pending == 0 and changed;
// kProcFused: changed decided and out written in one pass (evaluated null only)
constexpr uint32_t kProcCheck = 0, kProcWrite = 1, kProcFused = 2;
uint32_t proc_blocks(const ProcDesc& d);
hipError_t launch_proc_one(laspj_ctx* ctx, const ProcDesc& d, uint32_t* rec, uint32_t pass);
// descs: n descriptors on the device (block0 ascending), rec: 2 n words, blocks: their sum
hipError_t launch_proc_many(laspj_ctx* ctx, const ProcDesc* descs, uint32_t n, uint32_t blocks,
                            uint32_t* rec, uint32_t pass);

// ---- the read side's check over resident variables (laspj_reads.hip) ---------------------
// read/6, read_any/3 and wait_needed/6 (lasp_core.erl:331-420, 730-758): one previous state
// per read (its threshold's cells) against its currents — the variable's value first, then
// the variable's lazy thresholds in list order.  A read's wave items are the tiles of
// kReadTile 16-byte units covering the longest of its blocks of cells.
constexpr uint32_t kReadTile = 128;     // units per wave item: two per lane
constexpr uint32_t kReadChunk = 16;     // currents per descriptor hand-round
constexpr uint32_t kReadNarrow = 0, kReadWide = 1, kReadGset = 2;
struct ReadDesc {
    const uint64_t* cells;              // the threshold's cells (null: [])
    uint32_t words;                     // u64 words of `cells`
    uint32_t mode_strict;               // mode << 1 | strict
    uint32_t c0, nc;                    // its currents: ReadCur [c0, c0 + nc)
    uint64_t item0;                     // its first wave item
};
struct ReadCur {
    const uint64_t* cells;
    uint32_t words;
    uint32_t read;                      // the read it belongs to
};
static_assert(sizeof(ReadDesc) == 32 && sizeof(ReadCur) == 16, "descriptor layout");
// the records of n reads over ncs currents: {flags, n_current} x ncs, then n_previous x n
inline uint64_t read_rec_bytes(uint32_t n, uint32_t ncs) { return 8ull * ncs + 4ull * n; }
// rds / cs as the device reads them, rec: read_rec_bytes of device memory (zeroed here),
// met: ncs bytes (current j of read i met: threshold_met(Type, C_j, T_i)); two launches on
// the context's stream, no synchronisation
hipError_t launch_read_check(laspj_ctx* ctx, const ReadDesc* rds, uint32_t n, const ReadCur* cs,
                             uint32_t ncs, uint64_t items, uint32_t* rec, uint8_t* met);

// ---- list-valued resident variables (laspj_lvars.hip; include/laspj.h "list-valued
// resident variables") ---------------------------------------------------------------------
// the device images the order tables are derived from (laspj_codec.hip): the element slots
// in term order (E of them, unused slots last) and, per element slot, its token slots in
// term order (64 bytes, 0xFF after the last; null without tokens)
const uint32_t* etf_dict_elem_order(const laspj_etf_dict* d);
const uint8_t* etf_dict_tok_order(const laspj_etf_dict* d);
// a list batch's arrays as its kernels address them (laspj_lists.hip owns the layout)
struct ListDev {
    uint32_t* hdr;                      // [R][2] {entries, tokens}
    uint64_t* key;                      // [R][ce]
    uint64_t* tok;                      // [R][ct]
    uint32_t* toff;                     // [R][ce + 1]
    uint32_t ce, ct;
};
ListDev list_dev(const laspj_batch* b);
// room for ce entries and ct tokens per replica (ctx->mu held); a batch that grows loses
// its contents (its known counts become the capacities until it is written)
int list_reserve(laspj_ctx* ctx, laspj_batch* b, uint32_t ce, uint32_t ct);
// reply_to_all's test (lasp_core.erl:765-825) for the waiters of a list variable: waiter k's
// threshold is a one-replica OR-Set LIST batch of n entries (the host's count), met[k] =
// is_inflation (strict: is_strict_inflation) of it -> the value (lasp_lattice.erl:72-75,
// 153-161, 235-253, as k_linf_probe / k_linf_final restate them).  One pass: a memset, the
// value's key rank -> first index table built once, one check launch over tiles of kLwTile
// threshold entries of all waiters, a one-block finish launch that writes the met bytes into
// pinned memory, one synchronisation.  value: one replica; W >= 1.
constexpr uint32_t kLwTile = 256;       // threshold entries per work item: one per thread
struct ListWaiter {
    const laspj_batch* list;
    uint32_t n;
    uint32_t strict;
};
int list_waiters_check(laspj_ctx* ctx, const laspj_batch* value, const laspj_list_order* ord,
                       const ListWaiter* ws, uint32_t W, uint8_t* met);
// read/6's and read_any/3's tests (lasp_core.erl:331-364, 371-420) on list variables, the
// transpose of the waiter check: pair k asks whether current pairs[k].cur — a variable's
// value, or one of its lazy thresholds (reply_to_all's wait clause, :795-813) — inflates
// read pairs[k].read's threshold (strict: strictly), met[k] the answer.  reads: R thresholds
// (ListWaiter: list, entries, strict); curs: C one-replica OR-Set LIST batches, n the host's
// count of each one's entries.  One pass: a memset, a first-match table per current built by
// one insert launch, one check launch over tiles of kLwTile threshold entries of all pairs,
// a one-block finish launch that writes the met bytes into pinned memory, one
// synchronisation.  R, C, P >= 1.
struct ListReadCur {
    const laspj_batch* list;
    uint32_t n;
};
struct ListReadPair {
    uint32_t read, cur;
};
int list_reads_check(laspj_ctx* ctx, const laspj_list_order* ord, const ListWaiter* reads,
                     uint32_t R, const ListReadCur* curs, uint32_t C, const ListReadPair* pairs,
                     uint32_t P, uint8_t* met);
// laspj_list_bind of one-replica lists with a tail: the check pass of ws against dst (the
// merge) enqueued behind the bind's last kernel and ahead of its one synchronisation (again
// behind the merge path when the rank-indexed bind answers retry); met is written only when
// *status comes back 1 (written).  ws null: laspj_list_bind.
int list_bind_tail(laspj_ctx* ctx, laspj_batch* dst, const laspj_batch* cur,
                   const laspj_batch* val, const laspj_list_order* ord, uint8_t* status,
                   const ListWaiter* ws, uint32_t W, uint8_t* met);
// krank[elem_order[j]] = j and grank[64 e + k] = k's place in row e of tok_order, for every
// element slot (dirty null) or the ndirty slots listed (device array; krank is untouched:
// a patch adds no element).  E slots; krank E words, grank 64 E words.
hipError_t launch_lv_ranks(laspj_ctx* ctx, const uint32_t* elem_order, const uint8_t* tok_order,
                           uint32_t E, uint32_t* krank, uint32_t* grank, const uint32_t* dirty,
                           uint32_t ndirty);
// intersection/7's OR-Set branch (lasp_core.erl:559-568, 583) from two variables' cells: per
// term-order position j < n, e = elem_order[j]; an entry iff both cells hold a token (cells
// past El / Er slots are empty); tokens Cx ++ Cy placed by grank.  Two launches, no
// synchronisation: tile sums into `tiles` (lv_isect_tiles(n) C2 pairs of u64, device), then
// the writer, whose last tile writes ans = {entries, tokens, overflow} (a host-visible
// word triple).  overflow 1: out's capacity is short; out is then the empty list.
struct LvIsect {
    const uint64_t* l;
    const uint64_t* r;
    uint32_t El, Er;
    const uint32_t* elem_order;
    uint32_t n;
    const uint32_t* grank;              // 64 words per element slot
};
constexpr uint32_t kLvTile = 1024;      // positions per block: 256 threads x 4
inline uint32_t lv_isect_tiles(uint32_t n) { return n ? (n + kLvTile - 1) / kLvTile : 1; }
hipError_t launch_lv_isect(laspj_ctx* ctx, const LvIsect& a, const ListDev& out, uint64_t* tiles,
                           uint32_t* ans);
// product/7's OR-Set branch (lasp_core.erl:499-533, lasp_lattice.erl:303-308) from two
// variables' cells.  The side pass (two launches in the k_lv_count / k_lv_write tile scheme,
// one side per blockIdx.y; tiles: 2 x lv_isect_tiles(n) C2 pairs) compacts each side's held
// positions (p != 0, tombstoned or not) in term order: slot[i] the element slot, tpre[i] the
// exclusive token prefix (tpre[held] the total), run[tpre[i] ..] the tokens in term order
// (lv_run: 64 e + k, bit 63 removed), own[t] the position token t belongs to.  Its last tile
// per side writes ans[2 s] = held, ans[2 s + 1] = tokens, ans[4 + s] = 1 when cap_t was short.
// The host reads the four totals and sizes the output; the write pass then needs no scan:
// entry o = i nr + j has key {x_i, y_j}, toff[o] = A_i TR + a_i B_j, and output token t of
// NT = TL TR finds (i, j, u, v) through own in O(1) — one key / toff word and one token word
// per thread, consecutive lanes on consecutive words, every index product 64-bit.  Its last
// block writes the header and the toff sentinel (ans[6] = 1, the empty list: out was short).
struct LvSide {
    const uint64_t* cells;
    uint32_t E;                         // element slots the cells cover
    uint32_t* slot;                     // n words
    uint32_t* tpre;                     // n + 1 words
    uint32_t* own;                      // cap_t words
    uint64_t* run;                      // cap_t words
};
struct LvProd {
    LvSide s[2];                        // l, r
    const uint32_t* elem_order;
    uint32_t n;                         // term-order positions
    uint32_t cap_t;                     // tokens a side's run and own arrays hold
    const uint32_t* grank;              // 64 words per element slot
};
hipError_t launch_lp_sides(laspj_ctx* ctx, const LvProd& a, uint64_t* tiles, uint32_t* ans);
hipError_t launch_lp_write(laspj_ctx* ctx, const LvProd& a, uint32_t nl, uint32_t nr, uint32_t TL,
                           uint32_t TR, const ListDev& out, uint32_t* ans);
// map/6's body (lasp_core.erl:641-667) from one variable's cells and a map process's tables
// (include/laspj.h "resident map processes"): per term-order position j < n, e =
// elem_order[j]; a held cell (any token, tombstoned ones too) of an evaluated slot whose
// present tokens are all mapped emits {ymap[e], its tokens through tmap[e]}, placed by y's
// rank row.  A held slot F has not seen is pending, a present token with tmap 0xFF unmapped:
// such a cell emits nothing and the host discards the pass.  The tables cover E slots.
struct LmMap {
    const uint64_t* in;
    uint32_t Ein;
    uint32_t n;
    const uint32_t* elem_order;
    const uint32_t* grank;              // 64 words per element slot
    const uint64_t* evaluated;          // `words` words
    uint64_t* pmask;                    // `words` words: the pass's pending slots
    const uint32_t* ymap;               // E words
    const uint8_t* tmap;                // 64 E bytes
    uint32_t E, words;
};
// The count launch (tile sums, pmask, rec += {pending, unmapped}: rec two device words the
// caller keeps zero between passes) and, unless count_only, the writer behind it, whose last
// tile writes ans = {entries, tokens, overflow, pending, unmapped} (host-visible) and zeroes
// rec again.  No synchronisation.
hipError_t launch_lm_map(laspj_ctx* ctx, const LmMap& a, const ListDev& out, uint64_t* tiles,
                         uint32_t* rec, uint32_t* ans, bool count_only);
// fold/6's body (lasp_core.erl:460-486) from one variable's cells and a fold process's tables
// (include/laspj.h "resident fold processes"): per term-order position j < n, e =
// elem_order[j]; a held cell of an evaluated slot whose present tokens are all in fmapped[e]
// emits frow[e].count entries — row r = first + i gives {ykey[r], its tokens through tmap[r]},
// placed by that key's rank row.  Pending and unmapped as the map's; a slot with no rows
// emits nothing.  The slot tables cover E slots, the row tables `rows` rows.
struct LfFold {
    const uint64_t* in;
    uint32_t Ein;
    uint32_t n;
    const uint32_t* elem_order;
    const uint32_t* grank;              // 64 words per element slot
    const uint64_t* evaluated;          // `words` words
    uint64_t* pmask;                    // `words` words: the pass's pending slots
    const uint64_t* frow;               // E words: first row | row count << 32
    const uint64_t* fmapped;            // E words: the token slots mapped in every row
    const uint32_t* ykey;               // `rows` words: the element slot V took
    const uint8_t* tmap;                // 64 `rows` bytes
    uint32_t E, words, rows;
};
// As launch_lm_map; ans = {entries, tokens, overflow, pending, unmapped, fault}: the caller
// zeroes ans[5], and a writer that finds the row tables at odds with frow / fmapped (a row
// past `rows`, a key past E, a tmap byte of a promised token that names no slot or one taken
// already) writes in-range items and sets it.
hipError_t launch_lf_fold(laspj_ctx* ctx, const LfFold& a, const ListDev& out, uint64_t* tiles,
                          uint32_t* rec, uint32_t* ans, bool count_only);

// the host's half (laspj_reads_host.cpp: no device, no lock)
// wave items of a read whose longest block of cells has `words` u64 words
inline uint64_t read_tiles(uint64_t words) {
    return ((words + 1) / 2 + kReadTile - 1) / kReadTile;
}
// item0 of n descriptors from their tiles (tiles[i] from read_tiles); the total
uint64_t read_lay_items(ReadDesc* rds, uint32_t n, const uint64_t* tiles);
// The fold of read_any/3 (lasp_core.erl:372-414) over the device's answers.  Read i names
// variable var_of[i] (dense, < nvars; a variable may be named again), whose lazy list had
// nlazy[var] entries when the call began; ans[i]: 1 + nlazy[var] met bytes, the value's then
// one per lazy entry.  A read is visited while none before it was met: its fired entries
// are those still in the list (reply_to_all, :795-813); met ends the fold and stores
// nothing (:353-354, 399-400); unmet blocks — a waiter, and the fired entries leave (:362,
// :408).
struct ReadFold {
    int32_t found = -1;                          // the first met read, or -1
    std::vector<std::vector<uint32_t>> fired;    // per read: positions in its variable's
                                                 // list as the call found it, in list order
    std::vector<uint8_t> blocked;                // per read: it leaves a waiter
    std::vector<std::vector<uint32_t>> still;    // per variable: the positions that stay
    uint64_t total = 0;                          // fired ids over all reads
};
void read_fold(uint32_t n, const uint32_t* var_of, uint32_t nvars, const uint32_t* nlazy,
               const uint8_t* const* ans, ReadFold* out);

}  // namespace laspj
