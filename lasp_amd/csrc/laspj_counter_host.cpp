// riak_dt_gcounter images on the host (no GPU involved): the parser, encoder and threshold
// planner behind the counter variables of laspj_counters.hip, and the three
// laspj_gcounter_etf_* / laspj_gcounter_threshold_plan entry points of include/laspj.h.
//
// A counter's value is the orddict [{Actor, Count}] (riak_dt_gcounter's state; restated in
// oracle/core.py: _GCounter).  Counters hold one entry per client, so an image is tens to a
// few thousand entries: the host walks it with one hash probe per actor and ships
// {slot, count} pairs; nothing decodes a counter image on the device.

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>

#include "laspj_internal.h"

namespace laspj {

namespace {

enum : int {
    kSmallInt = 97, kInt = 98, kFloatOld = 99, kSmallTuple = 104, kLargeTuple = 105, kNil = 106,
    kList = 108, kSmallBig = 110, kLargeBig = 111, kNewFloat = 70
};

inline uint32_t be32(const uint8_t* p) {
    return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}

bool is_int_tag(uint8_t t) { return t == kSmallInt || t == kInt || t == kSmallBig || t == kLargeBig; }

// an integer term (its whole extent [p, p + n) checked by the caller) as sign and uint64
// magnitude: 0 ok, 1 the magnitude needs more than 64 bits
int read_int(const uint8_t* p, int* sign, uint64_t* mag) {
    switch (p[0]) {
        case kSmallInt:
            *mag = p[1];
            *sign = p[1] ? 1 : 0;
            return 0;
        case kInt: {
            const int64_t v = (int32_t)be32(p + 1);
            *sign = v < 0 ? -1 : (v > 0 ? 1 : 0);
            *mag = (uint64_t)(v < 0 ? -v : v);
            return 0;
        }
        default: {
            const bool small = p[0] == kSmallBig;
            size_t len = small ? p[1] : be32(p + 1);
            const uint8_t* s = p + (small ? 2 : 5);
            const uint8_t* d = s + 1;
            while (len && d[len - 1] == 0) --len;
            *sign = len ? (s[0] ? -1 : 1) : 0;
            *mag = 0;
            if (len > 8) return 1;
            for (size_t k = len; k-- > 0;) *mag = (*mag << 8) | d[k];
            return 0;
        }
    }
}

// NEW_FLOAT_EXT / FLOAT_EXT
double read_float(const uint8_t* x) {
    double f;
    if (x[0] == kNewFloat) {
        uint64_t b = 0;
        for (int i = 0; i < 8; ++i) b = (b << 8) | x[1 + i];
        std::memcpy(&f, &b, 8);
    } else {
        char buf[32];
        std::memcpy(buf, x + 1, 31);
        buf[31] = 0;
        f = std::strtod(buf, nullptr);
    }
    return f;
}

void put_be32(std::string* o, uint32_t v) {
    const char b[4] = {(char)(v >> 24), (char)(v >> 16), (char)(v >> 8), (char)v};
    o->append(b, 4);
}

}  // namespace

void gc_put_uint(std::string* o, uint64_t v) {
    if (v < 256) {
        o->push_back((char)kSmallInt);
        o->push_back((char)v);
    } else if (v <= 0x7FFFFFFFull) {
        o->push_back((char)kInt);
        put_be32(o, (uint32_t)v);
    } else {
        int len = 0;
        for (uint64_t m = v; m; m >>= 8) ++len;
        o->push_back((char)kSmallBig);
        o->push_back((char)len);
        o->push_back(0);
        for (int k = 0; k < len; ++k) o->push_back((char)(v >> (8 * k)));
    }
}

int gc_parse(laspj_dict* dict, const uint8_t* p, size_t n, std::vector<GcPair>* out) {
    out->clear();
    if (!p || n < 2 || p[0] != 131) return LASPJ_DEC_MALFORMED;
    const uint8_t* t = p + 1;
    const size_t tn = n - 1;
    // the image is one term, whole (binary_to_term/1 would take it)
    if (list_term_len(t, tn) != tn) return LASPJ_DEC_MALFORMED;
    if (t[0] == kNil) return LASPJ_DEC_OK;
    if (t[0] != kList) return LASPJ_DEC_UNREPRESENTABLE;          // (a string: no tuples)
    const uint32_t cnt = be32(t + 1);
    dict_begin(dict);
    int st = LASPJ_DEC_OK;
    size_t off = 5;
    const uint8_t* prev = nullptr;
    size_t prev_n = 0;
    try {
        out->reserve(cnt);
        for (uint32_t i = 0; i < cnt && st == LASPJ_DEC_OK; ++i) {
            // {Actor, Count}
            size_t a;
            if (t[off] == kSmallTuple && t[off + 1] == 2) {
                a = off + 2;
            } else if (t[off] == kLargeTuple && be32(t + off + 1) == 2) {
                a = off + 5;
            } else {
                st = LASPJ_DEC_UNREPRESENTABLE;
                break;
            }
            const size_t an = list_term_len(t + a, tn - a);
            const size_t c = a + an;
            const size_t cn = list_term_len(t + c, tn - c);
            off = c + cn;
            // orddict keys ascend strictly in term order
            if (prev) {
                int cmp = 0;
                if (laspj_term_compare(prev, prev_n, t + a, an, &cmp) != LASPJ_OK || cmp >= 0) {
                    st = LASPJ_DEC_UNREPRESENTABLE;
                    break;
                }
            }
            prev = t + a;
            prev_n = an;
            int sign = 0;
            uint64_t mag = 0;
            if (!is_int_tag(t[c]) || read_int(t + c, &sign, &mag) || sign <= 0) {
                st = LASPJ_DEC_UNREPRESENTABLE;
                break;
            }
            uint32_t slot = 0;
            st = dict_reg_elem(dict, t + a, an, &slot);
            if (st == LASPJ_E_NOMEM) {
                dict_rollback(dict);
                out->clear();
                return LASPJ_E_NOMEM;
            }
            if (st != LASPJ_DEC_OK) break;
            if (dict_elements(dict) > kGcMaxActors) {
                st = LASPJ_DEC_UNREPRESENTABLE;
                break;
            }
            out->push_back(GcPair{mag, slot, 0});
        }
    } catch (const std::bad_alloc&) {
        dict_rollback(dict);
        out->clear();
        return LASPJ_E_NOMEM;
    }
    // the tail of a proper list
    if (st == LASPJ_DEC_OK && t[off] != kNil) st = LASPJ_DEC_UNREPRESENTABLE;
    if (st != LASPJ_DEC_OK) {
        dict_rollback(dict);
        out->clear();
    }
    return st;
}

void gc_encode(const laspj_dict* dict, const GcPair* pairs, size_t n, std::string* out) {
    out->clear();
    out->push_back((char)131);
    size_t live = 0;
    for (size_t i = 0; i < n; ++i) live += pairs[i].count ? 1 : 0;
    if (!live) {
        out->push_back((char)kNil);
        return;
    }
    out->push_back((char)kList);
    put_be32(out, (uint32_t)live);
    for (size_t i = 0; i < n; ++i) {
        if (!pairs[i].count) continue;
        out->push_back((char)kSmallTuple);
        out->push_back(2);
        const std::string_view a = list_elem_image(dict, pairs[i].slot);
        out->append(a.data(), a.size());
        gc_put_uint(out, pairs[i].count);
    }
    out->push_back((char)kNil);
}

int gc_threshold_plan(const uint8_t* p, size_t n, bool strict, uint64_t* t) {
    *t = 0;
    if (!p || n < 2 || p[0] != 131 || list_term_len(p + 1, n - 1) != n - 1) return -1;
    const uint8_t* x = p + 1;
    const size_t xn = n - 1;
    // a non-number is above every number in term order: never `=<` a sum
    if (!is_int_tag(x[0]) && x[0] != kNewFloat && x[0] != kFloatOld) return LASPJ_GC_NEVER;
    // T against 0 and 2^64 by the dictionary's exact integer / float comparison
    static const uint8_t zero[2] = {kSmallInt, 0};
    static const uint8_t two64[12] = {kSmallBig, 9, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1};
    if (x[0] == kNewFloat || x[0] == kFloatOld) {
        if (std::isnan(read_float(x))) return LASPJ_GC_NEVER;
    }
    int c0 = 0, c64 = 0;
    if (laspj_term_compare(x, xn, zero, sizeof zero, &c0) != LASPJ_OK ||
        laspj_term_compare(x, xn, two64, sizeof two64, &c64) != LASPJ_OK)
        return -1;
    if (c0 < 0) return LASPJ_GC_ALWAYS;            // ceil(T) and floor(T) + 1 are both =< 0
    if (c64 >= 0) return LASPJ_GC_NEVER;
    uint64_t v;                                    // 0 =< T < 2^64
    if (is_int_tag(x[0])) {
        int sign = 0;
        read_int(x, &sign, &v);
        if (strict) {
            if (v == ~0ull) return LASPJ_GC_NEVER;          // T + 1 = 2^64
            ++v;
        }
    } else {
        const double f = read_float(x);
        // a double below 2^64 has an integral floor and ceiling of at most 2^64 - 2048:
        // both convert exactly, and floor + 1 does not wrap
        v = strict ? (uint64_t)std::floor(f) + 1 : (uint64_t)std::ceil(f);
    }
    if (v == 0) return LASPJ_GC_ALWAYS;
    *t = v;
    return LASPJ_GC_T;
}

}  // namespace laspj

extern "C" {

int laspj_gcounter_etf_parse(laspj_dict* dict, const uint8_t* image, uint64_t n, uint32_t* slots,
                             uint64_t* counts, uint32_t cap, uint32_t* npairs, int32_t* status) {
    if (!dict || !image || !npairs || !status || (cap && (!slots || !counts))) return LASPJ_E_INVAL;
    *npairs = 0;
    std::vector<laspj::GcPair> pairs;
    const int st = laspj::gc_parse(dict, image, n, &pairs);
    if (st < 0) return st;
    *status = st;
    if (st != LASPJ_DEC_OK) return LASPJ_OK;
    *npairs = (uint32_t)pairs.size();
    if (pairs.size() > cap) return LASPJ_E_RANGE;
    for (size_t i = 0; i < pairs.size(); ++i) {
        slots[i] = pairs[i].slot;
        counts[i] = pairs[i].count;
    }
    return LASPJ_OK;
}

int laspj_gcounter_etf_encode(const laspj_dict* dict, const uint32_t* slots,
                              const uint64_t* counts, uint32_t npairs, uint8_t* out, uint64_t cap,
                              uint64_t* out_len) {
    if (!dict || !out_len || (npairs && (!slots || !counts)) || (cap && !out)) return LASPJ_E_INVAL;
    try {
        std::vector<laspj::GcPair> pairs(npairs);
        for (uint32_t i = 0; i < npairs; ++i) {
            if (slots[i] >= laspj::dict_elements(dict)) return LASPJ_E_RANGE;
            pairs[i] = laspj::GcPair{counts[i], slots[i], 0};
        }
        std::string img;
        laspj::gc_encode(dict, pairs.data(), pairs.size(), &img);
        *out_len = img.size();
        if (img.size() > cap) return LASPJ_E_RANGE;
        std::memcpy(out, img.data(), img.size());
    } catch (const std::bad_alloc&) {
        return LASPJ_E_NOMEM;
    }
    return LASPJ_OK;
}

int laspj_gcounter_threshold_plan(const uint8_t* threshold, uint64_t n, int strict, int32_t* plan,
                                  uint64_t* t) {
    if (!threshold || !plan || !t) return LASPJ_E_INVAL;
    const int k = laspj::gc_threshold_plan(threshold, n, strict != 0, t);
    if (k < 0) return LASPJ_E_INVAL;
    *plan = k;
    return LASPJ_OK;
}

}  // extern "C"
