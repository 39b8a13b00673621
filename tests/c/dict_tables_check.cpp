// The wire codec's dictionary builder (laspj_dict_tables.cpp: plain host C++) as a program
// of its own, so that it can be built with the host sanitizers (tests/test_dict_tables_host.py
// builds and runs it; nothing here touches a GPU).
//
//   1. A fixed list of small dictionaries, one per branch of the builder: each one's facts,
//      block size and a 64-bit FNV-1a of the written image are compared with
//      tests/golden/dict_tables.txt (recorded from the builder as it stood inside
//      laspj_etf_dict_create before it became a unit of its own).
//   2. Arrays the builder must refuse: its status and message.
//   3. Patches against rebuilds: tokens added to a host dictionary, the patch's records
//      applied to the image, the patched elements compared with a fresh build.

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "../../lasp_amd/csrc/laspj_dict_tables.h"
#include "../../lasp_amd/csrc/laspj_internal.h"

using laspj::DictLayout;
using laspj::DictSource;
using laspj::DictTables;
using laspj::RdLayout;

static int bad = 0;
#define CHECK(c, ...)                 \
    do {                              \
        if (!(c)) {                   \
            std::printf(__VA_ARGS__); \
            std::printf("\n");        \
            ++bad;                    \
        }                             \
    } while (0)

// ---- term images ---------------------------------------------------------------------
static std::string be32(uint32_t v) {
    return {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
}
static std::string small_int(uint8_t v) { return std::string{(char)97, (char)v}; }
static std::string integer(int32_t v) { return std::string(1, (char)98) + be32((uint32_t)v); }
static std::string atom(const std::string& a) {
    return std::string{(char)100, 0, (char)a.size()} + a;
}
// BINARY_EXT of n bytes in all, its payload drawn from seed
static std::string binary(uint32_t n, uint64_t seed) {
    std::string s = std::string(1, (char)109) + be32(n - 5);
    for (uint32_t i = 5; i < n; ++i) {
        seed = seed * 6364136223846793005ull + 1442695040888963407ull;
        s += (char)(seed >> 56);
    }
    return s;
}

// ---- a dictionary as laspj_etf_dict_create takes it ------------------------------------
struct Spec {
    std::string name;
    std::vector<std::string> elems;                  // by slot ("": a slot without an image)
    std::vector<std::vector<std::string>> toks;      // by slot, by token slot; empty: a G-Set
    uint32_t headroom = 0;
    bool trusted = false;
    std::vector<uint8_t> eblob, tblob, tord;
    std::vector<uint32_t> eoff, eord, toff;

    static bool less(const std::string& a, const std::string& b) {
        int c = 0;
        laspj_term_compare((const uint8_t*)a.data(), a.size(), (const uint8_t*)b.data(), b.size(), &c);
        return c < 0;
    }
    // the arrays: slots in term order (those without an image last), tokens likewise
    void lay() {
        const uint32_t E = (uint32_t)elems.size();
        eoff.assign(1, 0);
        for (const auto& e : elems) {
            eblob.insert(eblob.end(), e.begin(), e.end());
            eoff.push_back((uint32_t)eblob.size());
        }
        for (uint32_t e = 0; e < E; ++e) eord.push_back(e);
        std::stable_sort(eord.begin(), eord.end(), [&](uint32_t a, uint32_t b) {
            if (elems[a].empty() || elems[b].empty()) return !elems[a].empty() && elems[b].empty();
            return less(elems[a], elems[b]);
        });
        if (toks.empty()) return;
        toks.resize(E);
        toff.assign(1, 0);
        tord.assign(64ull * E, 0xFF);
        for (uint32_t e = 0; e < E; ++e) {
            std::vector<uint8_t> o;
            for (uint32_t k = 0; k < 64; ++k) {
                if (k < toks[e].size() && !toks[e][k].empty()) {
                    tblob.insert(tblob.end(), toks[e][k].begin(), toks[e][k].end());
                    o.push_back((uint8_t)k);
                }
                toff.push_back((uint32_t)tblob.size());
            }
            std::stable_sort(o.begin(), o.end(),
                             [&](uint8_t a, uint8_t b) { return less(toks[e][a], toks[e][b]); });
            std::copy(o.begin(), o.end(), tord.begin() + 64ull * e);
        }
    }
    DictSource src() const {
        const bool t = !toks.empty();
        return {(uint32_t)elems.size(), eblob.data(), eoff.data(), eord.data(),
                t ? tblob.data() : nullptr, t ? toff.data() : nullptr, t ? tord.data() : nullptr};
    }
};

static std::vector<std::string> tokens(uint32_t n, uint32_t len, uint64_t seed) {
    std::vector<std::string> v;
    for (uint32_t k = 0; k < n; ++k) v.push_back(binary(len, seed * 1000 + k));
    return v;
}

std::vector<Spec> cases() {
    std::vector<Spec> v;
    auto add = [&v](const char* name, std::vector<std::string> elems,
                    std::vector<std::vector<std::string>> toks, uint32_t headroom, bool trusted) {
        Spec s;
        s.name = name;
        s.elems = std::move(elems);
        s.toks = std::move(toks);
        s.headroom = headroom;
        s.trusted = trusted;
        s.lay();
        v.push_back(std::move(s));
    };
    const std::string bin9 = binary(9, 77);
    add("a", {small_int(5)}, {}, 0, false);
    // one image twice, a slot without an image, an integer table over -3 .. 300
    add("b", {small_int(7), integer(-3), "", integer(300), atom("ab"), bin9, small_int(7)}, {}, 0,
        false);
    // integers too far apart for a table
    add("c", {small_int(0), integer(1 << 20), "", atom("ab"), bin9, small_int(0)}, {}, 0, false);
    const std::vector<std::string> e3 = {atom("x"), small_int(1), bin9};
    const std::vector<std::vector<std::string>> t013 = {{}, tokens(1, 20, 1), tokens(3, 20, 2)};
    add("d-h0", e3, t013, 0, false);
    add("d-h0-trusted", e3, t013, 0, true);
    add("d-h4", e3, t013, 4, false);
    add("d-h4-trusted", e3, t013, 4, true);
    // token images of two lengths: no record templates, the device keeps tok_off
    add("e", {atom("x"), small_int(1)}, {tokens(2, 20, 3), tokens(1, 7, 4)}, 0, false);
    // two-byte tokens that are no binaries: records of one whole word
    add("f", {atom("x"), small_int(1)}, {{small_int(3), small_int(9)}, {small_int(3)}}, 0, false);
    // the head-room rule past 8 tokens, the bucket search's bitmap past 16, a full mask
    const std::vector<std::vector<std::string>> tg = {tokens(9, 20, 5), tokens(17, 20, 6),
                                                      tokens(64, 20, 7)};
    add("g-h0", e3, tg, 0, false);
    add("g-h4-trusted", e3, tg, 4, true);
    // two tokens alike in every whole word of their record: no bucket window
    std::string h1 = binary(20, 8), h2 = h1;
    h2[18] ^= 1;
    h2[19] ^= 2;
    add("h", {atom("x")}, {{h1, h2}}, 0, false);
    // header templates of 4, 64 and 65 bytes (the last not hashed)
    add("i", {std::string(1, (char)106), binary(61, 9), binary(62, 10)},
        {tokens(1, 20, 11), tokens(1, 20, 12), tokens(1, 20, 13)}, 0, false);
    return v;
}

// ---- facts -----------------------------------------------------------------------------
static uint64_t fnv64(const void* p, uint64_t n, uint64_t h = 14695981039346656037ull) {
    const uint8_t* b = static_cast<const uint8_t*>(p);
    for (uint64_t i = 0; i < n; ++i) h = (h ^ b[i]) * 1099511628211ull;
    return h;
}

struct Facts {
    uint32_t toks, tok_uniform, tok_max, rec_len, rec_stride, bin_tokens, big_elems, ehdr_max,
        rd_hmask, gs, gs_hmask, gs_in, dev_toff, patchable;
    uint64_t rd_hlens, tpad_used, tpad_cap, bytes, image, patch_state;
    int64_t gs_ilo;
};

std::string line(const std::string& name, const Facts& f) {
    char buf[512];
    std::snprintf(buf, sizeof buf,
                  "%s toks=%u uniform=%u tok_max=%u rec_len=%u rec_stride=%u bin=%u big=%u "
                  "ehdr_max=%u rd_hmask=%u rd_hlens=%llx gs=%u gs_hmask=%u gs_ilo=%lld gs_in=%u "
                  "dev_toff=%u patchable=%u tpad_used=%llu tpad_cap=%llu patch_state=%016llx "
                  "bytes=%llu image=%016llx",
                  name.c_str(), f.toks, f.tok_uniform, f.tok_max, f.rec_len, f.rec_stride,
                  f.bin_tokens, f.big_elems, f.ehdr_max, f.rd_hmask, (unsigned long long)f.rd_hlens,
                  f.gs, f.gs_hmask, (long long)f.gs_ilo, f.gs_in, f.dev_toff, f.patchable,
                  (unsigned long long)f.tpad_used, (unsigned long long)f.tpad_cap,
                  (unsigned long long)f.patch_state, (unsigned long long)f.bytes,
                  (unsigned long long)f.image);
    return buf;
}

// the image in a heap block of exactly its size (a write past it is the sanitizer's to find)
static std::vector<uint8_t> image_of(const DictSource& s, const DictTables& t) {
    std::vector<uint8_t> img(t.lay.bytes, 0xA5);
    laspj::dict_tables_write(s, t, img.data());
    return img;
}

static Facts facts_of(const DictTables& t, const std::vector<uint8_t>& img) {
    Facts f{};
    f.toks = t.toks, f.tok_uniform = t.tok_uniform, f.tok_max = t.tok_max, f.rec_len = t.rec_len;
    f.rec_stride = t.rec_stride, f.bin_tokens = t.bin_tokens, f.big_elems = t.big_elems;
    f.ehdr_max = t.ehdr_max, f.rd_hmask = t.rd_hmask, f.rd_hlens = t.rd_hlens, f.gs = t.gs;
    f.gs_hmask = t.gs_hmask, f.gs_ilo = t.gs_ilo, f.gs_in = t.gs_in, f.dev_toff = t.dev_toff;
    f.patchable = t.patchable;
    if (t.patchable) {             // (the state a dictionary keeps only then)
        f.tpad_used = t.tpad_used, f.tpad_cap = t.tpad_cap;
        f.patch_state = fnv64(t.h_rank.data(), 4 * t.h_rank.size());
        f.patch_state = fnv64(t.h_tpoff.data(), 4 * t.h_tpoff.size(), f.patch_state);
    }
    f.bytes = t.lay.bytes;
    f.image = fnv64(img.data(), img.size());
    return f;
}

static size_t check_golden(const char* path) {
    std::ifstream in(path);
    std::vector<std::string> want;
    for (std::string l; std::getline(in, l);) want.push_back(l);
    const std::vector<Spec> cs = cases();
    CHECK(want.size() == cs.size(), "golden: %zu lines for %zu cases", want.size(), cs.size());
    for (size_t i = 0; i < cs.size(); ++i) {
        DictTables t;
        const int st = laspj::dict_tables_build(cs[i].src(), cs[i].headroom, cs[i].trusted, &t);
        CHECK(st == LASPJ_OK, "%s: status %d (%s)", cs[i].name.c_str(), st, t.err.c_str());
        if (st != LASPJ_OK) continue;
        const std::string got = line(cs[i].name, facts_of(t, image_of(cs[i].src(), t)));
        CHECK(i < want.size() && got == want[i], "golden differs:\n  got  %s\n  want %s", got.c_str(),
              i < want.size() ? want[i].c_str() : "(none)");
        if (cs[i].name == "h") {   // (its one element has no bucket window)
            uint32_t key = 0;
            std::memcpy(&key, t.rd.data() + RdLayout(1, t.tok_max).desc + 8, 4);
            CHECK(key == laspj::kNoBuckets, "h: key %x", key);
        }
    }
    return cs.size();
}

// ---- refused arrays --------------------------------------------------------------------
static void refused(const char* what, const Spec& s, int status, const char* msg) {
    DictTables t;
    const int st = laspj::dict_tables_build(s.src(), s.headroom, false, &t);
    CHECK(st == status && t.err == msg, "%s: status %d, \"%s\"", what, st, t.err.c_str());
}

static void check_refused() {
    Spec base;
    base.elems = {atom("x"), small_int(1), binary(9, 77)};
    base.toks = {{}, tokens(1, 20, 1), tokens(3, 20, 2)};
    base.lay();
    Spec s = base;
    s.eord[1] = s.eord[0];
    refused("order no permutation", s, LASPJ_E_RANGE, "etf_dict_create: element offsets / order invalid");
    s = base;
    s.eoff[1] = s.eoff[2] + 1;
    refused("element offsets", s, LASPJ_E_RANGE, "etf_dict_create: element offsets / order invalid");
    s = base;
    s.toff[64 * 2 + 1] = s.toff[64 * 2 + 2] + 1;
    refused("token offsets", s, LASPJ_E_RANGE, "etf_dict_create: token offsets decrease");
    s = base;
    s.tord[64 * 1 + 1] = 5;
    refused("order names an empty slot", s, LASPJ_E_RANGE,
            "etf_dict_create: token order of element 1 names slot 5 twice or without an image");
    s = base;
    s.tord[64 * 2 + 2] = 0xFF;
    refused("order misses a slot", s, LASPJ_E_RANGE,
            "etf_dict_create: token order of element 2 misses a slot");
    s = base;
    s.elems.clear();            // (the arrays stay: E = 0 reads none of them)
    refused("no slots", s, LASPJ_E_SHAPE, "etf_dict_create: no element slots");
}

// ---- patch against rebuild -------------------------------------------------------------
// a host dictionary (laspj_host.cpp) and the device tables built from its export
struct Built {
    std::vector<uint8_t> eblob, tblob, tord;
    std::vector<uint32_t> eoff, eord, toff;
    DictTables t;
    std::vector<uint8_t> img;
    DictSource src() const {
        return {(uint32_t)eord.size(), eblob.data(), eoff.data(), eord.data(), tblob.data(),
                toff.data(), tord.data()};
    }
    laspj::DictPatchIn in() const {
        return {t.patchable, (uint32_t)eord.size(), t.tok_max, t.rec_len, t.rec_stride, t.tok_uniform,
                &t.lay, t.h_rank.data(), t.h_tpoff.data(), t.tpad_used, t.tpad_cap};
    }
};

static bool build_from(const laspj_dict* hd, uint32_t headroom, Built* b) {
    uint32_t E = 0;
    uint64_t eb = 0, tb = 0;
    if (laspj_dict_info(hd, &E, &eb, &tb) != LASPJ_OK) return false;
    b->eblob.resize(eb + 1), b->tblob.resize(tb + 1), b->tord.resize(64ull * E);
    b->eoff.resize(E + 1), b->eord.resize(E), b->toff.resize(64ull * E + 1);
    if (laspj_dict_export(hd, E, b->eblob.data(), b->eoff.data(), b->eord.data(), b->tblob.data(),
                          b->toff.data(), b->tord.data()) != LASPJ_OK)
        return false;
    if (laspj::dict_tables_build(b->src(), headroom, true, &b->t) != LASPJ_OK) return false;
    b->img = image_of(b->src(), b->t);
    return true;
}

static laspj_dict* host_dict(const std::vector<std::string>& elems, const std::vector<uint32_t>& ntok,
                             uint64_t seed) {
    laspj_dict* hd = nullptr;
    laspj_dict_create(&hd);
    for (size_t e = 0; e < elems.size(); ++e) {
        uint32_t slot = 0, ts = 0;
        int st = laspj::dict_reg_elem(hd, (const uint8_t*)elems[e].data(), elems[e].size(), &slot);
        CHECK(st == LASPJ_DEC_OK && slot == e, "dict_reg_elem: %d", st);
        for (uint32_t k = 0; k < ntok[e]; ++k) {
            const std::string tk = binary(20, seed * 1000 + 100 * e + k);
            st = laspj::dict_reg_tok(hd, slot, (const uint8_t*)tk.data(), tk.size(), &ts);
            CHECK(st == LASPJ_DEC_OK && ts == k, "dict_reg_tok: %d", st);
        }
    }
    return hd;
}

static void add_tokens(laspj_dict* hd, uint32_t e, uint32_t n, uint32_t len, uint64_t seed) {
    for (uint32_t k = 0; k < n; ++k) {
        const std::string tk = binary(len, seed * 1000 + k);
        uint32_t slot = 0;
        const int st = laspj::dict_reg_tok(hd, e, (const uint8_t*)tk.data(), tk.size(), &slot);
        CHECK(st == LASPJ_DEC_OK, "dict_reg_tok: %d", st);
    }
}

// the patch of `dirty` applied to a's image and host state, then each dirty element compared
// with the fresh build of the grown dictionary
static void patch_and_compare(const char* what, const laspj_dict* hd, Built* a, uint32_t headroom,
                              const std::vector<uint32_t>& dirty) {
    laspj::DictPatch p;
    const int st = laspj::dict_patch_rows(a->in(), hd, dirty.data(), (uint32_t)dirty.size(), &p);
    CHECK(st == LASPJ_OK && !p.recs.empty(), "%s: patch status %d", what, st);
    if (st != LASPJ_OK) return;
    for (const auto& r : p.recs) {
        const bool inside = r.dst + r.len <= a->img.size() && (uint64_t)r.src + r.len <= p.data.size();
        CHECK(inside, "%s: record outside the block or the data", what);
        if (inside) std::memcpy(a->img.data() + r.dst, p.data.data() + r.src, r.len);
    }
    for (const auto& nt : p.new_tpoff) a->t.h_tpoff[nt.first] = nt.second;
    a->t.tpad_used = p.tpad_used;
    a->t.big_elems += p.big_add;
    Built b;
    CHECK(build_from(hd, headroom, &b), "%s: rebuild", what);
    CHECK(a->t.tpad_used == b.t.tpad_used && a->t.big_elems == b.t.big_elems,
          "%s: image area use / big elements differ from the rebuild's", what);
    const DictLayout &la = a->t.lay, &lb = b.t.lay;
    const uint32_t ka = a->t.tok_max, kb = b.t.tok_max, E = (uint32_t)a->eord.size();
    const RdLayout ra(E, ka), rb(E, kb);
    const uint8_t *ia = a->img.data(), *ib = b.img.data();
    auto same = [&](const char* row, uint64_t oa, uint64_t ob, uint64_t n) {
        CHECK(std::memcmp(ia + oa, ib + ob, n) == 0, "%s: %s differs from the rebuild's", what, row);
    };
    for (uint32_t e : dirty) {
        const uint64_t r = a->t.h_rank[e];
        CHECK(r == b.t.h_rank[e], "%s: rank moved", what);
        same("mask", la.mask + 8ull * e, lb.mask + 8ull * e, 8);
        same("token order", la.tord + 64ull * e, lb.tord + 64ull * e, 64);
        same("slot -> rank", la.rd + ra.ros + 64 * r, lb.rd + rb.ros + 64 * r, 64);
        if (ka == kb) {
            const uint64_t rs = a->t.rec_stride;
            same("record templates", la.rpad + e * ka * rs, lb.rpad + e * ka * rs, ka * rs);
            same("desc key and count", la.rd + ra.desc + 16 * r + 8, lb.rd + rb.desc + 16 * r + 8, 8);
            same("buckets", la.rd + ra.tb + 2 * r * ka, lb.rd + rb.tb + 2 * r * ka, 2ull * ka);
        }
        // each writer descriptor: the same slot and length, and through its padded offset
        // the same image bytes
        for (uint32_t j = 0; j < std::min(ka, kb); ++j) {
            uint64_t da, db;
            std::memcpy(&da, ia + la.tdesc + 8 * ((uint64_t)e * ka + j), 8);
            std::memcpy(&db, ib + lb.tdesc + 8 * ((uint64_t)e * kb + j), 8);
            CHECK((uint32_t)da == (uint32_t)db, "%s: descriptor %u of element %u differs", what, j, e);
            if ((da & 0xFF) == 0xFF || (uint32_t)da != (uint32_t)db) continue;
            const uint64_t len = (da >> 8) & 0xFFFFFF;
            CHECK((da >> 32) + len <= a->t.tpad_cap && (db >> 32) + len <= b.t.tpad_cap,
                  "%s: descriptor %u of element %u leaves the image area", what, j, e);
            same("token image", la.tpad + (da >> 32), lb.tpad + (db >> 32), len);
        }
    }
}

static void unsupported(const char* what, const laspj::DictPatchIn& in, const laspj_dict* hd,
                        uint32_t e) {
    laspj::DictPatch p;
    const int st = laspj::dict_patch_rows(in, hd, &e, 1, &p);
    CHECK(st == LASPJ_E_UNSUPPORTED && p.recs.empty() && p.data.empty(), "%s: status %d, %zu records",
          what, st, p.recs.size());
}

static void check_patches() {
    const std::vector<std::string> e3 = {atom("x"), small_int(1), binary(9, 77)};
    {   // (d): tok_max 7 before and after, then an element grows and the rebuild's is 8
        laspj_dict* hd = host_dict(e3, {0, 1, 3}, 21);
        Built a;
        CHECK(build_from(hd, 4, &a) && a.t.patchable && a.t.tok_max == 7, "d: build");
        add_tokens(hd, 0, 1, 20, 22);
        add_tokens(hd, 1, 1, 20, 23);
        patch_and_compare("d, two elements", hd, &a, 4, {0, 1});
        add_tokens(hd, 2, 2, 20, 24);
        patch_and_compare("d, wider rebuild", hd, &a, 4, {2});
        // only a rebuild will do
        add_tokens(hd, 2, 3, 20, 25);
        unsupported("past the headroom", a.in(), hd, 2);
        add_tokens(hd, 0, 1, 7, 26);
        unsupported("another token length", a.in(), hd, 0);
        add_tokens(hd, 1, 1, 20, 27);
        laspj::DictPatchIn full = a.in();
        full.tpad_cap = full.tpad_used + 48;
        unsupported("image area full", full, hd, 1);
        Built plain;
        CHECK(build_from(hd, 0, &plain) && !plain.t.patchable, "d: build without headroom");
        unsupported("built without headroom", plain.in(), hd, 1);
        laspj_dict_destroy(hd);
    }
    {   // (g): the bitmap search and tok_max 64
        laspj_dict* hd = host_dict(e3, {9, 17, 64}, 31);
        Built a;
        CHECK(build_from(hd, 4, &a) && a.t.patchable && a.t.tok_max == 64, "g: build");
        add_tokens(hd, 0, 1, 20, 32);
        add_tokens(hd, 1, 2, 20, 33);
        patch_and_compare("g, two elements", hd, &a, 4, {0, 1});
        laspj_dict_destroy(hd);
    }
}

int main(int argc, char** argv) {
    if (argc < 2) {
        std::printf("usage: dict_tables_check tests/golden/dict_tables.txt\n");
        return 2;
    }
    const size_t n = check_golden(argv[1]);
    check_refused();
    check_patches();
    std::printf("%zu dictionaries, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
