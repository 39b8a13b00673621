// The wire codec's dictionary tables: what the host builder (laspj_dict_tables.cpp, plain
// C++, no device call) and the device decoders and writers (laspj_codec.hip) must agree on,
// and the builder's types.  Usable from plain C++ and from HIP.
#pragma once

#include <cstdint>
#include <string>
#include <utility>
#include <vector>

#include "../../include/laspj.h"

#if defined(__HIP__)
#define LASPJ_HD __host__ __device__
#else
#define LASPJ_HD
#endif

namespace laspj {

constexpr uint32_t kBuckets = 1024;      // token buckets per element
// an element's key when no bucket window separates its tokens: the batch paths find no
// bucket (its table entries are 0xFFFF) and leave it to decode_elems, which matches its
// records against each template
constexpr uint32_t kNoBuckets = 0x80000000u;
// the element-batch decoders take elements of at most this many tokens (small_dict)
constexpr uint32_t kSmallTok = 8;

// the header-template hash (host and device agree): ceil(hl / 4) words, bytes >= hl zero
LASPJ_HD inline uint32_t hdr_mix(uint32_t h, uint32_t v) {
    h ^= v;
    h *= 0x9E3779B1u;
    return h ^ (h >> 16);
}

LASPJ_HD inline __attribute__((always_inline)) uint32_t fnv1a(const uint8_t* p, uint32_t n) {
    uint32_t h = 2166136261u;
    for (uint32_t i = 0; i < n; ++i) h = (h ^ p[i]) * 16777619u;
    return h;
}

// a token image that is BINARY_EXT of exactly the rest of its bytes
inline bool tok_is_binary(const uint8_t* p, uint32_t len) {
    return len >= 5u && p[0] == 109 &&
           (((uint32_t)p[1] << 24) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 8) | p[4]) == len - 5u;
}

// one row of a dictionary patch (k_patch scatters them)
struct PatchRec {
    unsigned long long dst;   // byte offset in the dictionary's block
    uint32_t src, len;        // bytes [src, src + len) of the staged patch data
};

// the ReadTabs tables of E element ranks, one after the other: desc (16 E) | hdr (64 E) |
// tb (2 E tok_max) | ros (64 E); offsets from the tables' start
struct RdLayout {
    uint64_t desc = 0, hdr, tb, ros, bytes;
    RdLayout(uint64_t E, uint64_t tok_max)
        : hdr(16 * E), tb(hdr + 64 * E), ros(tb + 2 * E * tok_max), bytes(ros + 64 * E + 64) {}
};

// the arrays laspj_etf_dict_create takes (laspj_dict_export writes them); the token arrays
// null together: a G-Set dictionary
struct DictSource {
    uint32_t E;
    const uint8_t* elem_blob;
    const uint32_t* elem_off;     // E + 1
    const uint32_t* elem_order;   // E
    const uint8_t* tok_blob;
    const uint32_t* tok_off;      // 64 E + 1
    const uint8_t* tok_order;     // 64 E
};

// where each array sits in the dictionary's device block (256-byte aligned), and its size
struct DictLayout {
    uint64_t eoff = 0, eord = 0, eb = 0, mask = 0, toff = 0, tord = 0, eblob = 0, epoff = 0,
             epad = 0, tpad = 0, tdesc = 0, rpad = 0, hpad = 0, hpoff = 0, rd = 0, htab = 0,
             gsh = 0, gsr = 0, gsb = 0, gsi = 0, bytes = 0;
};

// a dictionary's tables on the host: dict_tables_build's result, dict_tables_write's source
struct DictTables {
    // the facts laspj_etf_dict keeps
    bool toks = false;            // token arrays given (an OR-Set dictionary)
    bool dev_toff = false;        // the device keeps tok_off (mixed token image lengths)
    bool gs = false;              // the G-Set from_binary tables exist
    uint32_t tok_uniform = 0, tok_max = 0, rec_len = 0, rec_stride = 0;
    bool bin_tokens = false;
    uint32_t big_elems = 0, ehdr_max = 0;
    uint32_t rd_hmask = 0;
    uint64_t rd_hlens = 0;
    uint32_t gs_hmask = 0;
    int64_t gs_ilo = 0;
    uint32_t gs_in = 0;           // entries of gs_itab (0: no integer table)
    // the derived tables (rpad .. htab with record templates only: rec_len != 0)
    std::vector<uint8_t> ebyte, epad, tpad, rpad, hpad, rd;
    std::vector<uint64_t> tmask, tdesc, gs_itab;
    std::vector<uint32_t> epoff, hpoff, htab, gs_htab, gs_rank, gs_byte;
    uint64_t epad_n = 0, tpad_n = 0;      // bytes of epad / tpad the image holds
    DictLayout lay;
    // dict_patch_rows' state: slot -> rank, each token slot's padded image offset
    // (0xFFFFFFFF: none), the padded-image area's use
    bool patchable = false;
    std::vector<uint32_t> h_rank, h_tpoff;
    uint64_t tpad_used = 0, tpad_cap = 0;
    std::string err;              // the failure's message
};

// Validates the arrays (trusted: arrays the library exported itself from its host
// dictionary, where offsets ascend, the order is a permutation and token orders name
// exactly the used slots by construction — those checks, passes over every slot, are left
// out) and derives every table.  tok_headroom: the per-element token tables take up to that
// many more tokens per element than the widest element has (at most 8 while that stays
// <= 8, at most 64), with room for appended token images and the patch state kept.
// LASPJ_OK, or the status laspj_etf_dict_create reports with its message in t->err.  The
// element arrays are not null (the caller's check).
int dict_tables_build(const DictSource& s, uint32_t tok_headroom, bool trusted, DictTables* t);
// the block's image into img (t.lay.bytes): every array, zeros in the alignment gaps
void dict_tables_write(const DictSource& s, const DictTables& t, void* img);

// what a patch reads of a built dictionary
struct DictPatchIn {
    bool patchable;               // built with token headroom (and record templates)
    uint32_t E, tok_max, rec_len, rec_stride, tok_uniform;
    const DictLayout* lay;
    const uint32_t* h_rank;
    const uint32_t* h_tpoff;
    uint64_t tpad_used, tpad_cap;
};
struct DictPatch {
    std::vector<uint8_t> data;            // the rows' bytes, each row on a 16-byte boundary
    std::vector<PatchRec> recs;           // where each goes in the block
    std::vector<std::pair<uint64_t, uint32_t>> new_tpoff;   // (64 e + slot, padded offset)
    uint64_t tpad_used = 0;
    uint32_t big_add = 0;                 // elements that grew past kSmallTok tokens
    bool lost_bin = false;                // a token that is no BINARY_EXT was seen
};
// The rows of element slots `dirty` (each gained tokens in the host dictionary hd) as a full
// build writes them: token mask, term order, new tokens' padded images (appended), writer
// descriptors, record templates, and of the element's rank the bucket choice, buckets and
// slot -> rank.  LASPJ_E_UNSUPPORTED (no records) when only a rebuild will do: a dictionary
// built without headroom, an element past its token headroom, a token image of another
// length, the image area full.
int dict_patch_rows(const DictPatchIn& d, const laspj_dict* hd, const uint32_t* dirty, uint32_t n,
                    DictPatch* out);

}  // namespace laspj
