// The wire codec's dictionary tables, built on the host (laspj_dict_tables.h): plain C++,
// no device call.  laspj_etf_dict_create (laspj_codec.hip) builds them, writes their image
// into its pinned staging and copies it to the device; etf_dict_patch assembles the rows of
// a few elements with the same per-element row writers.

#include "laspj_dict_tables.h"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string_view>

namespace laspj {

// laspj_host.cpp
bool dict_tokens(const laspj_dict* dict, uint32_t e, std::vector<std::string_view>* imgs,
                 std::vector<uint8_t>* order);

namespace {

inline uint64_t pad16(uint64_t x) { return (x + 15ull) & ~15ull; }

int fail(DictTables* t, int code, const char* fmt, ...) {
    char buf[256];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t->err = buf;
    return code;
}

// ---- one element's rows, as the full build and a patch both write them ----------------

// an element's tokens: its slots in term order and, by slot, each token's image, length and
// padded image offset
struct ElemToks {
    uint32_t cnt = 0;
    const uint8_t* order = nullptr;
    const uint8_t* img[64];
    uint32_t len[64], poff[64];
};

// writer descriptors by term rank: slot | length << 8 | padded offset << 32, 0xFF after the
// last
void row_tok_desc(const ElemToks& x, uint32_t tok_max, uint64_t* row) {
    for (uint32_t j = 0; j < tok_max; ++j) {
        const uint64_t k = j < x.cnt ? x.order[j] : 0xFFull;
        row[j] = j < x.cnt ? k | (std::min<uint64_t>(x.len[k], 0xFFFFFFull) << 8) |
                                 ((uint64_t)x.poff[k] << 32)
                           : k;
    }
}

// record templates by term rank: 104 2 <token image> (the rest of each row is zero already)
void row_templates(const ElemToks& x, uint64_t rec_stride, uint8_t* rows) {
    for (uint32_t j = 0; j < x.cnt; ++j) {
        uint8_t* r = rows + j * rec_stride;
        r[0] = 104;
        r[1] = 2;
        std::memcpy(r + 2, x.img[x.order[j]], x.len[x.order[j]]);
    }
}

// The bucket choice over an element's templates: a template word and shift that put its
// cnt tokens in distinct buckets, kc = {word | shift << 8, cnt} and tb the bucket per term
// rank (entries past cnt are zero already); no such window: kNoBuckets and 0xFFFF.
void row_buckets(const uint8_t* rows, uint64_t rec_stride, uint32_t rec_len, uint32_t cnt,
                 uint32_t* kc, uint16_t* tb) {
    kc[0] = 0;
    kc[1] = cnt;
    if (cnt == 0) return;
    uint32_t keys[64];
    for (uint32_t wi = rec_len / 4; wi-- > 0;) {          // whole words of the template
        uint32_t diff = 0;                // the bits where some token differs
        for (uint32_t j = 0; j < cnt; ++j) {
            std::memcpy(&keys[j], rows + j * rec_stride + 4 * wi, 4);
            diff |= keys[j] ^ keys[0];
        }
        if (cnt > 1 && !diff) continue;     // one word for all: no window parts them
        for (uint32_t sh = 0; sh + 10 <= 32; ++sh) {
            // (a window without a differing bit puts every token in one bucket)
            if (cnt > 1 && !((diff >> sh) & (kBuckets - 1u))) continue;
            bool ok = true;
            if (cnt <= 16) {
                for (uint32_t j = 1; j < cnt && ok; ++j) {
                    const uint32_t bj = (keys[j] >> sh) & (kBuckets - 1u);
                    for (uint32_t i = 0; i < j && ok; ++i)
                        ok = ((keys[i] >> sh) & (kBuckets - 1u)) != bj;
                }
            } else {
                uint64_t seen[kBuckets / 64] = {};
                for (uint32_t j = 0; j < cnt && ok; ++j) {
                    const uint32_t bk = (keys[j] >> sh) & (kBuckets - 1u);
                    ok = !((seen[bk / 64] >> (bk % 64)) & 1ull);
                    seen[bk / 64] |= 1ull << (bk % 64);
                }
            }
            if (!ok) continue;
            kc[0] = wi | (sh << 8);
            for (uint32_t j = 0; j < cnt; ++j)
                tb[j] = (uint16_t)((keys[j] >> sh) & (kBuckets - 1u));
            return;
        }
    }
    // no one 10-bit window tells this element's tokens apart (tokens that agree everywhere
    // but where others also agree): its records are matched against each of its templates
    // instead (rare, and only this element)
    kc[0] = kNoBuckets;
    for (uint32_t j = 0; j < cnt; ++j) tb[j] = 0xFFFFu;
}

// token slot -> term rank, 0xFF: no token
void row_slot_rank(const ElemToks& x, uint8_t* ros) {
    std::memset(ros, 0xFF, 64);
    for (uint32_t j = 0; j < x.cnt; ++j) ros[x.order[j]] = (uint8_t)j;
}

// ---- the full build's phases ---------------------------------------------------------

// what the token scan finds of the token images' lengths and kind
struct TokScan {
    uint32_t uniform = 0;
    bool mixed = false, binall = true;
};

// elem_byte, and the element arrays' checks
int scan_elements(const DictSource& s, bool trusted, DictTables* t) {
    const uint32_t E = s.E;
    t->ebyte.assign(E, 0);
    std::vector<uint8_t> ranked(trusted ? 0 : E, 0);    // (the order must be a permutation)
    for (uint32_t e = 0; e < E; ++e) {
        if (!trusted && (s.elem_off[e + 1] < s.elem_off[e] || s.elem_order[e] >= E ||
                         ranked[s.elem_order[e]]++))
            return fail(t, LASPJ_E_RANGE, "etf_dict_create: element offsets / order invalid");
        t->ebyte[e] = s.elem_off[e + 1] - s.elem_off[e] == 2 && s.elem_blob[s.elem_off[e]] == 97;
    }
    return LASPJ_OK;
}

// tok_mask, each token's padded image offset (an empty slot keeps ~0u, the patch's "no
// image" mark), the image lengths' scan, and the token arrays' checks
int scan_tokens(const DictSource& s, bool trusted, DictTables* t, TokScan* ts) {
    const uint32_t E = s.E;
    uint32_t bad = 0;                             // (branch-free: it vectorises)
    for (uint64_t k = 0; !trusted && k < 64ull * E; ++k) bad |= s.tok_off[k + 1] < s.tok_off[k];
    if (bad) return fail(t, LASPJ_E_RANGE, "etf_dict_create: token offsets decrease");
    t->h_tpoff.assign(64ull * E, 0xFFFFFFFFu);
    for (uint32_t e = 0; e < E; ++e) {
        const uint32_t* to = s.tok_off + 64ull * e;
        if (to[64] == to[0]) continue;            // no tokens: the common case, one test
        uint64_t m = 0;
        for (uint32_t k = 0; k < 64 && to[k] != to[64]; ++k) {   // (to the last token)
            const uint32_t len = to[k + 1] - to[k];
            if (!len) continue;
            m |= 1ull << k;
            if (!ts->uniform) ts->uniform = len;
            else if (ts->uniform != len) ts->mixed = true;
            if (ts->binall) ts->binall = tok_is_binary(s.tok_blob + to[k], len);
            t->h_tpoff[64ull * e + k] = (uint32_t)t->tpad_n;
            t->tpad_n += pad16(len);
        }
        t->tmask[e] = m;
    }
    for (uint32_t e = 0; e < E && !trusted; ++e) {
        uint64_t seen = 0;
        for (int j = 0; j < 64; ++j) {
            uint8_t k = s.tok_order[64ull * e + j];
            if (k >= 64) break;
            if (!((t->tmask[e] >> k) & 1ull) || ((seen >> k) & 1ull))
                return fail(t, LASPJ_E_RANGE,
                            "etf_dict_create: token order of element %u names slot %u "
                            "twice or without an image", e, k);
            seen |= 1ull << k;
        }
        if (seen != t->tmask[e])
            return fail(t, LASPJ_E_RANGE,
                        "etf_dict_create: token order of element %u misses a slot", e);
    }
    return LASPJ_OK;
}

// 16-byte-aligned copies of every image (the write kernels load them 16 B at a time)
int pad_images(const DictSource& s, DictTables* t) {
    const uint32_t E = s.E;
    t->epoff.resize(E);
    for (uint32_t e = 0; e < E; ++e) {
        t->epoff[e] = (uint32_t)t->epad_n;
        t->epad_n += pad16(s.elem_off[e + 1] - s.elem_off[e]);
    }
    t->epad_n += 48;              // a 48-byte load past the last image stays inside
    t->tpad_n += 48;
    if (t->epad_n >= (1ull << 32) || t->tpad_n >= (1ull << 32))
        return fail(t, LASPJ_E_RANGE, "etf_dict_create: images exceed 4 GiB");
    t->epad.assign(t->epad_n, 0);
    t->tpad.assign(t->tpad_n, 0);
    for (uint32_t e = 0; e < E; ++e)
        std::copy(s.elem_blob + s.elem_off[e], s.elem_blob + s.elem_off[e + 1],
                  t->epad.begin() + t->epoff[e]);
    for (uint64_t e = 0; t->toks && e < E; ++e)
        for (uint64_t m = t->tmask[e]; m; m &= m - 1) {       // the slots holding a token
            const uint64_t k = 64ull * e + __builtin_ctzll(m);
            std::copy(s.tok_blob + s.tok_off[k], s.tok_blob + s.tok_off[k + 1],
                      t->tpad.begin() + t->h_tpoff[k]);
        }
    return LASPJ_OK;
}

// element header templates 104 2 <elem image> 108, padded as the images are
int header_templates(const DictSource& s, DictTables* t) {
    const uint32_t E = s.E;
    t->hpoff.resize(E);
    uint64_t hn = 0, ehdr_max = 0;
    for (uint32_t e = 0; e < E; ++e) {
        const uint64_t hl = s.elem_off[e + 1] - s.elem_off[e] + 3ull;
        t->hpoff[e] = (uint32_t)hn;
        hn += pad16(hl);
        ehdr_max = std::max(ehdr_max, hl);
    }
    t->ehdr_max = (uint32_t)std::min<uint64_t>(ehdr_max, 0xFFFFFFFFull);
    if (hn + 48 >= (1ull << 32) || t->rpad.size() >= (1ull << 40))
        return fail(t, LASPJ_E_RANGE, "etf_dict_create: record templates too large");
    t->hpad.assign(hn + 48, 0);
    for (uint32_t e = 0; e < E; ++e) {
        uint8_t* h = t->hpad.data() + t->hpoff[e];
        h[0] = 104;
        h[1] = 2;
        std::copy(s.elem_blob + s.elem_off[e], s.elem_blob + s.elem_off[e + 1], h + 2);
        h[2 + s.elem_off[e + 1] - s.elem_off[e]] = 108;
    }
    return LASPJ_OK;
}

// The per-element token rows.  The writer's descriptors by (element, term rank), tok_max
// per element (not 64: a rebuild then builds and uploads what the elements hold); with
// uniform token images the record templates 104 2 <image> per (element, term rank) and the
// from_binary tables by element rank (by slot, each slot's rank looked up: the slot-indexed
// sources read in order).
void token_rows(const DictSource& s, DictTables* t) {
    const uint32_t E = s.E, RK = t->tok_max;
    const RdLayout rl(E, RK);
    ElemToks x;
    for (uint32_t e = 0; e < E; ++e) {
        x.order = s.tok_order + 64ull * e;
        for (x.cnt = 0; x.cnt < RK && x.order[x.cnt] < 64; ++x.cnt) {
            const uint32_t k = x.order[x.cnt];
            const uint64_t g = 64ull * e + k;
            x.img[k] = s.tok_blob + s.tok_off[g];
            x.len[k] = s.tok_off[g + 1] - s.tok_off[g];
            x.poff[k] = t->h_tpoff[g];
        }
        if (x.cnt) row_tok_desc(x, RK, t->tdesc.data() + (uint64_t)e * RK);
        if (!t->rec_len) continue;
        const uint64_t r = t->h_rank[e];
        const uint32_t hl = s.elem_off[e + 1] - s.elem_off[e] + 3u;
        uint8_t* rd = t->rd.data();
        uint32_t* desc = reinterpret_cast<uint32_t*>(rd + rl.desc) + 4 * r;
        uint8_t* rows = t->rpad.data() + (uint64_t)e * RK * t->rec_stride;
        row_templates(x, t->rec_stride, rows);
        desc[0] = e;
        desc[1] = hl;
        std::memcpy(rd + rl.hdr + 64 * r, t->hpad.data() + t->hpoff[e], std::min(hl, 64u));
        row_buckets(rows, t->rec_stride, t->rec_len, x.cnt, desc + 2,
                    reinterpret_cast<uint16_t*>(rd + rl.tb) + r * RK);
        row_slot_rank(x, rd + rl.ros + 64 * r);
    }
}

// segment mode: header template (<= 64 bytes) -> rank, hashed as the device hashes
void header_hash(uint32_t E, DictTables* t) {
    uint64_t cap = 64;
    while (cap < 2ull * E) cap <<= 1;
    t->htab.assign(cap, 0);
    t->rd_hmask = (uint32_t)(cap - 1);
    const RdLayout rl(E, t->tok_max);
    const uint8_t* hdr = t->rd.data() + rl.hdr;
    const uint32_t* desc = reinterpret_cast<const uint32_t*>(t->rd.data() + rl.desc);
    for (uint64_t r = 0; r < E; ++r) {
        const uint32_t hl = desc[4 * r + 1];
        if (hl < 4 || hl > 64) continue;
        uint32_t h = hl * 0x85EBCA6Bu;
        for (uint32_t i = 0; 4 * i < hl; ++i) {         // ceil(hl / 4) words
            uint32_t v;
            std::memcpy(&v, hdr + 64 * r + 4 * i, 4);   // zero past hl
            h = hdr_mix(h, v);
        }
        uint64_t i = h & (cap - 1);
        while (t->htab[i]) i = (i + 1) & (cap - 1);
        t->htab[i] = (uint32_t)r + 1u;
        t->rd_hlens |= 1ull << (hl - 1);
    }
}

// a minimal integer image's value (SMALL_INTEGER for 0..255, INTEGER past it)
bool int_of(const DictSource& s, uint32_t e, int64_t* v) {
    const uint32_t n = s.elem_off[e + 1] - s.elem_off[e];
    const uint8_t* img = s.elem_blob + s.elem_off[e];
    if (n == 2 && img[0] == 97) {
        *v = img[1];
        return true;
    }
    if (n == 5 && img[0] == 98) {
        *v = (int32_t)((uint32_t)img[1] << 24 | (uint32_t)img[2] << 16 | (uint32_t)img[3] << 8 |
                       img[4]);
        return *v < 0 || *v > 255;
    }
    return false;
}

// G-Set from_binary tables: ranks (equal terms share one), image hash, byte values, and the
// integer elements by value
void gset_tables(const DictSource& s, DictTables* t) {
    const uint32_t E = s.E;
    uint64_t cap = 64;
    while (cap < 2ull * E) cap <<= 1;
    t->gs_hmask = (uint32_t)(cap - 1);
    t->gs_rank.assign(E, 0);
    t->gs_byte.assign(256, 0);
    uint32_t rk = 0;
    for (uint32_t k = 0; k < E; ++k) {
        const uint32_t e = s.elem_order[k];
        if (k) {
            const uint32_t p = s.elem_order[k - 1];
            int c = 1;
            const bool both = s.elem_off[e + 1] > s.elem_off[e] && s.elem_off[p + 1] > s.elem_off[p];
            if (!both ||
                laspj_term_compare(s.elem_blob + s.elem_off[p], s.elem_off[p + 1] - s.elem_off[p],
                                   s.elem_blob + s.elem_off[e], s.elem_off[e + 1] - s.elem_off[e],
                                   &c) != LASPJ_OK)
                c = 1;
            if (c != 0) ++rk;
        }
        t->gs_rank[e] = rk;
    }
    t->gs_htab.assign(cap, 0);
    for (uint32_t e = 0; e < E; ++e) {
        const uint32_t n = s.elem_off[e + 1] - s.elem_off[e];
        if (!n) continue;
        const uint8_t* img = s.elem_blob + s.elem_off[e];
        if (n == 2 && img[0] == 97 && !t->gs_byte[img[1]]) t->gs_byte[img[1]] = e + 1;
        uint64_t i = fnv1a(img, n) & (cap - 1);
        bool dup = false;
        while (t->gs_htab[i] && !dup) {
            const uint32_t o = t->gs_htab[i] - 1;
            // an image twice: the first slot keeps it
            dup = s.elem_off[o + 1] - s.elem_off[o] == n &&
                  std::memcmp(s.elem_blob + s.elem_off[o], img, n) == 0;
            if (!dup) i = (i + 1) & (cap - 1);
        }
        if (!dup) t->gs_htab[i] = e + 1;
    }
    int64_t lo = INT64_MAX, hi = INT64_MIN, v;
    uint64_t cnt = 0;
    for (uint32_t e = 0; e < E; ++e)
        if (int_of(s, e, &v)) lo = std::min(lo, v), hi = std::max(hi, v), ++cnt;
    if (cnt && (uint64_t)(hi - lo) < std::max<uint64_t>(4 * cnt, 1ull << 16)) {
        t->gs_ilo = lo;
        t->gs_itab.assign((uint64_t)(hi - lo) + 1, 0);
        for (uint32_t e = 0; e < E; ++e)
            if (int_of(s, e, &v) && !t->gs_itab[v - lo])      // one value twice: the first slot
                t->gs_itab[v - lo] = (e + 1ull) | ((uint64_t)t->gs_rank[e] << 32);
        t->gs_in = (uint32_t)t->gs_itab.size();
    }
}

// On the device: the token offsets only for mixed image lengths (the size pass reads them
// then); the token images themselves and their padded offsets never (the kernels read the
// padded copies through tok_desc) — 64 E-slot arrays the NIF path's rebuilds would
// otherwise stage and copy every time.
void lay_out(const DictSource& s, DictTables* t) {
    const uint64_t E = s.E;
    DictLayout& L = t->lay;
    uint64_t at = 0;
    auto take = [&at](uint64_t n) {
        const uint64_t o = at;
        at += (n + 255ull) & ~255ull;
        return o;
    };
    L.eoff = take(4 * (E + 1));
    L.eord = take(4 * E);
    L.eb = take(E);
    L.mask = take(8 * E);
    L.toff = take(t->dev_toff ? 4 * (64 * E + 1) : 0);
    L.tord = take(t->toks ? 64 * E : 0);
    L.eblob = take(s.elem_off[E] + 1ull);
    L.epoff = take(4 * E);
    L.epad = take(t->epad_n);
    L.tpad = take(t->tpad_cap);
    L.tdesc = take(8 * t->tdesc.size() + 8);
    L.rpad = take(t->rpad.size());
    L.hpad = take(t->hpad.size());
    L.hpoff = take(4 * t->hpoff.size() + 4);
    L.rd = take(t->rd.size() + 8);
    L.htab = take(4 * t->htab.size() + 4);
    L.gsh = take(4 * (t->gs_hmask + 1ull));
    L.gsr = take(4 * t->gs_rank.size());
    L.gsb = take(4 * t->gs_byte.size());
    L.gsi = take(8 * t->gs_itab.size() + 8);
    L.bytes = at;
}

}  // namespace

int dict_tables_build(const DictSource& s, uint32_t tok_headroom, bool trusted, DictTables* t) {
    const uint32_t E = s.E;
    if (E == 0) return fail(t, LASPJ_E_SHAPE, "etf_dict_create: no element slots");
    t->toks = s.tok_off != nullptr;
    if (t->toks && (!s.tok_order || (!s.tok_blob && s.tok_off[64ull * E])))
        return fail(t, LASPJ_E_INVAL, "etf_dict_create: token arrays incomplete");
    t->tmask.assign(E, 0);
    TokScan ts;
    if (int st = scan_elements(s, trusted, t)) return st;
    if (t->toks)
        if (int st = scan_tokens(s, trusted, t, &ts)) return st;
    if (int st = pad_images(s, t)) return st;
    for (uint32_t e = 0; e < E; ++e) {
        const uint32_t n = (uint32_t)__builtin_popcountll(t->tmask[e]);
        t->big_elems += n > kSmallTok ? 1u : 0u;
        t->tok_max = std::max(t->tok_max, n);
    }
    // (past 8 the head-room grows with the count: a hot element re-added again and again —
    // add_elem never collects a token — then rebuilds the images every count / 2 adds, not
    // every tok_headroom)
    if (tok_headroom && t->toks)
        t->tok_max = t->tok_max <= 8
                         ? std::min(8u, t->tok_max + tok_headroom)
                         : std::min(64u, t->tok_max + std::max(tok_headroom, t->tok_max / 2));
    t->tok_uniform = ts.mixed ? 0u : ts.uniform;
    t->dev_toff = t->toks && ts.mixed;
    // room for token images appended by a patch
    t->tpad_cap = t->tpad_n +
                  (tok_headroom && t->toks ? std::max<uint64_t>(t->tpad_n / 4, 1ull << 16) : 0);
    t->tpad_used = t->tpad_n - 48;
    // record templates: uniform token images only
    t->rec_len = (t->toks && t->tok_uniform && t->tok_uniform + 2u <= 48u) ? t->tok_uniform + 2u : 0u;
    t->rec_stride = (uint32_t)pad16(t->rec_len);
    t->bin_tokens = t->rec_len && t->tok_uniform >= 5u && ts.binall;
    t->patchable = tok_headroom && t->rec_len;
    t->tdesc.assign(t->toks ? (uint64_t)t->tok_max * E : 0, 0xFFull);
    if (t->rec_len) {
        t->rpad.assign((uint64_t)E * t->tok_max * t->rec_stride + 48, 0);
        if (int st = header_templates(s, t)) return st;
        t->rd.assign(RdLayout(E, t->tok_max).bytes, 0);
        t->h_rank.resize(E);
        for (uint32_t r = 0; r < E; ++r) t->h_rank[s.elem_order[r]] = r;
    }
    if (t->toks) token_rows(s, t);
    if (t->rec_len) header_hash(E, t);
    // Not for the library's own OR-Set namespaces (trusted, with tokens): their payloads are
    // OR-Set images only, and the tables cost a term comparison per slot per rebuild
    t->gs = !(trusted && t->toks);
    if (t->gs) gset_tables(s, t);
    else t->gs_hmask = 63;
    lay_out(s, t);
    return LASPJ_OK;
}

void dict_tables_write(const DictSource& s, const DictTables& t, void* image) {
    const uint64_t E = s.E;
    const DictLayout& L = t.lay;
    uint8_t* img = static_cast<uint8_t*>(image);
    // the arrays in layout order, zeros in the alignment gaps between them (nothing reads
    // them; kept deterministic) — no zero fill of the whole image first
    uint64_t at = 0;
    auto up = [&](uint64_t off, const void* src, uint64_t n) {
        if (off > at) std::memset(img + at, 0, off - at);
        if (n) std::memcpy(img + off, src, n);
        at = off + n;
    };
    up(L.eoff, s.elem_off, 4 * (E + 1));
    up(L.eord, s.elem_order, 4 * E);
    up(L.eb, t.ebyte.data(), E);
    up(L.mask, t.tmask.data(), 8 * E);
    if (t.dev_toff) up(L.toff, s.tok_off, 4 * (64 * E + 1));
    if (t.toks) up(L.tord, s.tok_order, 64 * E);
    up(L.eblob, s.elem_blob, s.elem_off[E]);
    up(L.epoff, t.epoff.data(), 4 * E);
    up(L.epad, t.epad.data(), t.epad_n);
    if (t.toks) up(L.tpad, t.tpad.data(), t.tpad_n);
    if (t.toks) up(L.tdesc, t.tdesc.data(), 8 * t.tdesc.size());
    if (t.rec_len) {
        up(L.rpad, t.rpad.data(), t.rpad.size());
        up(L.hpad, t.hpad.data(), t.hpad.size());
        up(L.hpoff, t.hpoff.data(), 4 * t.hpoff.size());
        up(L.rd, t.rd.data(), t.rd.size());
        up(L.htab, t.htab.data(), 4 * t.htab.size());
    }
    if (t.gs) {
        up(L.gsh, t.gs_htab.data(), 4 * t.gs_htab.size());
        up(L.gsr, t.gs_rank.data(), 4 * E);
        up(L.gsb, t.gs_byte.data(), 4 * 256);
    }
    if (t.gs_in) up(L.gsi, t.gs_itab.data(), 8 * t.gs_itab.size());
    if (L.bytes > at) std::memset(img + at, 0, L.bytes - at);
}

int dict_patch_rows(const DictPatchIn& d, const laspj_dict* hd, const uint32_t* dirty, uint32_t n,
                    DictPatch* out) {
    const uint32_t E = d.E, RK = d.tok_max, RL = d.rec_len, TL = d.tok_uniform;
    const uint64_t RS = d.rec_stride;
    const DictLayout& L = *d.lay;
    const RdLayout rl(E, RK);
    *out = DictPatch();
    DictPatch& p = *out;
    // (no records when it fails)
    auto unsupported = [&p] {
        p.data.clear(), p.recs.clear(), p.new_tpoff.clear();
        return LASPJ_E_UNSUPPORTED;
    };
    if (!d.patchable) return unsupported();
    // a row's place in the data (zeroed, padded to 16 bytes) and its record
    auto put = [&p](uint64_t dst, uint32_t len) {
        const uint32_t at = (uint32_t)p.data.size();
        p.data.resize(p.data.size() + pad16(len), 0);
        p.recs.push_back(PatchRec{dst, at, len});
        return at;
    };
    auto put_bytes = [&](uint64_t dst, const void* src, uint32_t len) {
        const uint32_t at = put(dst, len);
        std::memcpy(p.data.data() + at, src, len);
    };
    p.tpad_used = d.tpad_used;
    std::vector<std::string_view> imgs;
    std::vector<uint8_t> order;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t e = dirty[i];
        if (e >= E || !dict_tokens(hd, e, &imgs, &order)) return unsupported();
        const uint32_t cnt = (uint32_t)imgs.size();
        if (cnt > RK || cnt > 64 || cnt == 0) return unsupported();
        {
            uint32_t had = 0;                  // (the element's count the images hold)
            for (uint32_t k = 0; k < 64; ++k) had += d.h_tpoff[64ull * e + k] != 0xFFFFFFFFu;
            if (had <= kSmallTok && cnt > kSmallTok) ++p.big_add;
        }
        for (const auto& im : imgs)
            if (im.size() != TL || TL + 2u != RL) return unsupported();
        for (const auto& im : imgs)
            if (!tok_is_binary(reinterpret_cast<const uint8_t*>(im.data()), TL)) p.lost_bin = true;
        // token mask and term order
        const uint64_t mask = cnt == 64 ? ~0ull : (1ull << cnt) - 1ull;
        put_bytes(L.mask + 8ull * e, &mask, 8);
        uint8_t ord[64];
        std::memset(ord, 0xFF, 64);
        std::memcpy(ord, order.data(), cnt);
        put_bytes(L.tord + 64ull * e, ord, 64);
        // padded images of the new slots, appended
        ElemToks x;
        x.cnt = cnt;
        x.order = order.data();
        for (uint32_t k = 0; k < cnt; ++k) {
            uint32_t o = d.h_tpoff[64ull * e + k];
            for (const auto& nt : p.new_tpoff)
                if (nt.first == 64ull * e + k) o = nt.second;
            if (o == 0xFFFFFFFFu) {
                const uint64_t need = pad16(TL);
                if (p.tpad_used + need + 48 > d.tpad_cap) return unsupported();
                o = (uint32_t)p.tpad_used;
                p.tpad_used += need;
                put_bytes(L.tpad + o, imgs[k].data(), TL);
                p.new_tpoff.emplace_back(64ull * e + k, o);
            }
            x.img[k] = reinterpret_cast<const uint8_t*>(imgs[k].data());
            x.len[k] = TL;
            x.poff[k] = o;
        }
        // the token rows, and the from_binary tables of the element's rank (of its
        // descriptor {slot, header length, key, tokens} the first two do not change)
        const uint32_t r = d.h_rank[e];
        const uint32_t a_td = put(L.tdesc + 8ull * RK * e, 8 * RK);
        const uint32_t a_rows = put(L.rpad + (uint64_t)e * RK * RS, (uint32_t)(RK * RS));
        const uint32_t a_kc = put(L.rd + rl.desc + 16ull * r + 8, 8);
        const uint32_t a_tb = put(L.rd + rl.tb + 2ull * r * RK, 2 * RK);
        const uint32_t a_ros = put(L.rd + rl.ros + 64ull * r, 64);
        uint8_t* base = p.data.data();
        row_tok_desc(x, RK, reinterpret_cast<uint64_t*>(base + a_td));
        row_templates(x, RS, base + a_rows);
        row_buckets(base + a_rows, RS, RL, cnt, reinterpret_cast<uint32_t*>(base + a_kc),
                    reinterpret_cast<uint16_t*>(base + a_tb));
        row_slot_rank(x, base + a_ros);
    }
    return LASPJ_OK;
}

}  // namespace laspj
