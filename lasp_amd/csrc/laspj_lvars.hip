// List-valued resident variables (include/laspj.h "list-valued resident variables"): the
// kernels of a namespace's order tables and of intersection/7's OR-Set branch run straight
// from two resident variables' cells.
//
// lasp_core:intersection/7 (lasp_core.erl:559-568, 583) walks l's orddict in term order and,
// where lists:keyfind finds the key in r, emits {X, Cx ++ Cy}.  Over cells that is one
// producer over term-order positions: position j names element slot e = elem_order[j]; it
// emits an entry iff both cells hold a token, with popcount(l.p) + popcount(r.p) tokens.
// The composition it replaces (laspj_list_from_set, then laspj_list_intersection_set) writes
// l's whole list form and reads it back, and places an element's tokens by walking its 64
// term-order ranks serially.  Here a token's place inside its run is the popcount of the
// run's tokens of lower rank: the ranks present are gathered into one 64-bit mask (one table
// load per present token, none for a one-token run) and each token lands at the popcount of
// the mask below its own rank.
//
// Shape: tiles of 1024 positions per 256-thread block, four consecutive positions per
// thread (one 16-byte load of elem_order, a 16-byte load per cell).  k_lv_count leaves each
// tile's {entries, tokens}; k_lv_write sums the tiles before its own (at most 1024 of them
// at 2^20 elements: four loads per thread), scans its items in the block and writes; the
// last tile writes the list's header, the token-offset sentinel and the totals the host
// reads after the bind's synchronisation.  No block waits on another: the two launches are
// ordered by the stream.  Every write is checked against the output's capacity.
//
// map/6 (lasp_core.erl:641-667; include/laspj.h "resident map processes") is the same producer
// over one variable's cells and a map process's tables: k_lm_count / k_lm_write below; fold/6
// (lasp_core.erl:460-486; "resident fold processes") emits a run of entries per cell:
// k_lf_count / k_lf_write.  product/7 (lasp_core.erl:499-533; "pair-keyed list variables")
// compacts both inputs' cells the same way (k_lp_count / k_lp_side) and writes the |L| x |R|
// output from the two sides' prefixes without a scan (k_lp_write).

#include "laspj_internal.h"

namespace laspj {

namespace {

typedef uint64_t u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kLvT = 256;            // threads per tile block
constexpr uint32_t kLvI = 4;              // consecutive positions per thread
static_assert(kLvT * kLvI == kLvTile, "a tile is a block's positions");
constexpr u64 kLvRemoved = 1ull << 63;
constexpr uint32_t kLvNoElem = 0xFFFFFFFFu;   // a position past the last: no cell holds it

struct Cnt {
    uint32_t e, t;
};

// exclusive block scan of {entries, tokens}; *total: the block's sums
__device__ __forceinline__ Cnt lv_block_excl(Cnt v, Cnt* lds, Cnt* total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    Cnt x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t ye = __shfl_up(x.e, off, 64), yt = __shfl_up(x.t, off, 64);
        if ((int)lane >= off) {
            x.e += ye;
            x.t += yt;
        }
    }
    if (lane == 63) lds[w] = x;
    __syncthreads();
    Cnt before{0, 0}, all{0, 0};
#pragma unroll
    for (uint32_t i = 0; i < kLvT / 64; ++i) {
        const Cnt t = lds[i];
        if (i < w) {
            before.e += t.e;
            before.t += t.t;
        }
        all.e += t.e;
        all.t += t.t;
    }
    __syncthreads();
    *total = all;
    return Cnt{before.e + x.e - v.e, before.t + x.t - v.t};
}

// the element slots of a thread's four positions (kLvNoElem past the last position); A: the
// producer's arguments (elem_order, n)
template <class A>
__device__ __forceinline__ void lv_slots(const A& a, uint32_t j0, uint32_t* e) {
    if (j0 + kLvI <= a.n && (reinterpret_cast<uintptr_t>(a.elem_order) & 15u) == 0) {
        const u32x4 v = *reinterpret_cast<const u32x4*>(a.elem_order + j0);
        e[0] = v.x, e[1] = v.y, e[2] = v.z, e[3] = v.w;
        return;
    }
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) e[k] = j0 + k < a.n ? a.elem_order[j0 + k] : kLvNoElem;
}

// both variables' cells {p, r} of element slot e: a variable whose cells cover fewer slots
// than the namespace is empty beyond them
__device__ __forceinline__ void lv_cells(const LvIsect& a, uint32_t e, u64x2* L, u64x2* R) {
    *L = u64x2{0, 0};
    *R = u64x2{0, 0};
    if (e < a.El) *L = *reinterpret_cast<const u64x2*>(a.l + 2ull * e);
    if (e < a.Er) *R = *reinterpret_cast<const u64x2*>(a.r + 2ull * e);
}

__device__ __forceinline__ Cnt lv_count(const u64x2& L, const u64x2& R) {
    if (!L.x || !R.x) return Cnt{0, 0};
    return Cnt{1u, (uint32_t)(__popcll(L.x) + __popcll(R.x))};
}

// one cell's tokens in term order at T: token k's place is the number of the cell's tokens
// whose rank (g: the element's 64 rank words) is below k's
__device__ __forceinline__ void lv_run(u64* T, uint32_t e, u64 p, u64 rm, const uint32_t* g) {
    if ((p & (p - 1)) == 0) {                              // one token: no rank needed
        const uint32_t k = (uint32_t)__builtin_ctzll(p);
        T[0] = (64ull * e + k) | (((rm >> k) & 1ull) ? kLvRemoved : 0ull);
        return;
    }
    u64 present = 0;
    for (u64 b = p; b; b &= b - 1) present |= 1ull << (g[__builtin_ctzll(b)] & 63u);
    for (u64 b = p; b; b &= b - 1) {
        const uint32_t k = (uint32_t)__builtin_ctzll(b);
        const uint32_t at = (uint32_t)__popcll(present & ((1ull << (g[k] & 63u)) - 1ull));
        T[at] = (64ull * e + k) | (((rm >> k) & 1ull) ? kLvRemoved : 0ull);
    }
}

__global__ __launch_bounds__(kLvT) void k_lv_count(LvIsect a, u64* tiles) {
    __shared__ Cnt lds[kLvT / 64];
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    Cnt mine{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        u64x2 L, R;
        lv_cells(a, e[k], &L, &R);
        const Cnt c = lv_count(L, R);
        mine.e += c.e;
        mine.t += c.t;
    }
    Cnt tot;
    lv_block_excl(mine, lds, &tot);
    if (threadIdx.x == 0) {
        tiles[2ull * blockIdx.x] = tot.e;
        tiles[2ull * blockIdx.x + 1] = tot.t;
    }
}

__global__ __launch_bounds__(kLvT) void k_lv_write(LvIsect a, ListDev out, const u64* tiles,
                                                   uint32_t* ans) {
    __shared__ Cnt lds[kLvT / 64];
    // the tiles before this one
    Cnt pre{0, 0};
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kLvT) {
        pre.e += (uint32_t)tiles[2ull * i];
        pre.t += (uint32_t)tiles[2ull * i + 1];
    }
    Cnt base;
    lv_block_excl(pre, lds, &base);
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    u64x2 L[kLvI], R[kLvI];
    Cnt c[kLvI], mine{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        lv_cells(a, e[k], &L[k], &R[k]);
        c[k] = lv_count(L[k], R[k]);
        mine.e += c[k].e;
        mine.t += c[k].t;
    }
    Cnt tot;
    const Cnt ex = lv_block_excl(mine, lds, &tot);
    uint32_t pos = base.e + ex.e, tp = base.t + ex.t;
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        if (!c[k].e) continue;
        if (pos < out.ce && (u64)tp + c[k].t <= out.ct) {
            out.key[pos] = e[k];
            out.toff[pos] = tp;
            const uint32_t* g = a.grank + 64ull * e[k];
            lv_run(out.tok + tp, e[k], L[k].x, L[k].y, g);                       // Cx
            lv_run(out.tok + tp + __popcll(L[k].x), e[k], R[k].x, R[k].y, g);    // ++ Cy
        }
        pos += 1;
        tp += c[k].t;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const uint32_t ne = base.e + tot.e, nt = base.t + tot.t;
        const bool over = ne > out.ce || nt > out.ct;
        out.hdr[0] = over ? 0u : ne;
        out.hdr[1] = over ? 0u : nt;
        out.toff[over ? 0u : ne] = over ? 0u : nt;
        ans[0] = ne;
        ans[1] = nt;
        ans[2] = over ? 1u : 0u;
    }
}

// ---- map/6 (lasp_core.erl:641-667) from a variable's cells and a map process's tables ------
// One entry {F(X), Cx} per held slot e: the key is ymap[e], the element slot F(X) took in the
// input's namespace, and each token of the cell is named by the slot its image holds under
// that element (tmap[e][k]), so every run is ordered inside one rank row, y's — also where
// F sends two inputs to one key.

// what slot e's cell gives: its entry's counts, the key, the present and removed masks in
// the key's slot space; un: present tokens without a mapping (the cell then emits nothing,
// as does a held slot F has not been asked about: the slot-order half counts that one)
struct LmCell {
    Cnt c;
    uint32_t y, un;
    u64 q, qr;
};

__device__ __forceinline__ LmCell lm_cell(const LmMap& a, uint32_t e) {
    LmCell o{Cnt{0, 0}, 0, 0, 0, 0};
    if (e >= a.Ein || e >= a.E) return o;
    const u64x2 C = *reinterpret_cast<const u64x2*>(a.in + 2ull * e);
    if (!C.x || !((a.evaluated[e >> 6] >> (e & 63u)) & 1ull)) return o;
    o.y = a.ymap[e];
    const uint8_t* tm = a.tmap + 64ull * e;
    if (o.y >= a.E) {                                      // (no table row: nothing to place by)
        o.un = (uint32_t)__popcll(C.x);
        return o;
    }
    if ((C.x & (C.x - 1)) == 0) {                          // one token: one byte
        const uint32_t k = (uint32_t)__builtin_ctzll(C.x), k2 = tm[k];
        if (k2 >= 64u) {
            o.un = 1;
            return o;
        }
        o.q = 1ull << k2;
        o.qr = ((C.y >> k) & 1ull) << k2;
    } else {
        for (u64 b = C.x; b; b &= b - 1) {
            const uint32_t k = (uint32_t)__builtin_ctzll(b), k2 = tm[k];
            if (k2 >= 64u) {
                ++o.un;
                continue;
            }
            o.q |= 1ull << k2;
            o.qr |= ((C.y >> k) & 1ull) << k2;
        }
        if (o.un) return o;
    }
    o.c = Cnt{1u, (uint32_t)__popcll(o.q)};
    return o;
}

__device__ __forceinline__ void lm_rec_add(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(kLvT) void k_lm_count(LmMap a, u64* tiles, uint32_t* rec) {
    __shared__ Cnt lds[kLvT / 64];
    const uint32_t lane = threadIdx.x & 63u;
    // the filter's check over this tile's element slots in slot order: a wave's 64 slots are
    // one word of the bitmaps, four words per wave
    {
        const uint32_t w0 = (blockIdx.x * kLvTile + (threadIdx.x & ~63u) * kLvI) >> 6;
        uint32_t pend = 0;
#pragma unroll
        for (uint32_t i = 0; i < kLvI; ++i) {
            const uint32_t w = w0 + i, s = 64u * w + lane;
            if (w >= a.words) break;                       // (wave-uniform)
            const bool held = s < a.Ein && a.in[2ull * s] != 0;
            const u64 pm = __ballot(held) & ~a.evaluated[w];
            if (lane == 0) a.pmask[w] = pm;
            pend += (uint32_t)__popcll(pm);
        }
        if (lane == 0 && pend) lm_rec_add(rec, pend);
    }
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    Cnt mine{0, 0};
    uint32_t un = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        const LmCell c = lm_cell(a, e[k]);
        mine.e += c.c.e;
        mine.t += c.c.t;
        un += c.un;
    }
    if (__ballot(un != 0)) {                               // (rare: a token minted since)
        for (int s = 32; s; s >>= 1) un += __shfl_xor(un, s, 64);
        if (lane == 0) lm_rec_add(rec + 1, un);
    }
    Cnt tot;
    lv_block_excl(mine, lds, &tot);
    if (threadIdx.x == 0) {
        tiles[2ull * blockIdx.x] = tot.e;
        tiles[2ull * blockIdx.x + 1] = tot.t;
    }
}

__global__ __launch_bounds__(kLvT) void k_lm_write(LmMap a, ListDev out, const u64* tiles,
                                                   uint32_t* rec, uint32_t* ans) {
    __shared__ Cnt lds[kLvT / 64];
    Cnt pre{0, 0};
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kLvT) {
        pre.e += (uint32_t)tiles[2ull * i];
        pre.t += (uint32_t)tiles[2ull * i + 1];
    }
    Cnt base;
    lv_block_excl(pre, lds, &base);
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    LmCell c[kLvI];
    Cnt mine{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        c[k] = lm_cell(a, e[k]);
        mine.e += c[k].c.e;
        mine.t += c[k].c.t;
    }
    Cnt tot;
    const Cnt ex = lv_block_excl(mine, lds, &tot);
    uint32_t pos = base.e + ex.e, tp = base.t + ex.t;
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        if (!c[k].c.e) continue;
        if (pos < out.ce && (u64)tp + c[k].c.t <= out.ct) {
            out.key[pos] = c[k].y;
            out.toff[pos] = tp;
            // the run in y's slot space, placed by the popcount of lower ranks in y's row
            lv_run(out.tok + tp, c[k].y, c[k].q, c[k].qr, a.grank + 64ull * c[k].y);
        }
        pos += 1;
        tp += c[k].c.t;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const uint32_t ne = base.e + tot.e, nt = base.t + tot.t;
        const bool over = ne > out.ce || nt > out.ct;
        out.hdr[0] = over ? 0u : ne;
        out.hdr[1] = over ? 0u : nt;
        out.toff[over ? 0u : ne] = over ? 0u : nt;
        ans[0] = ne;
        ans[1] = nt;
        ans[2] = over ? 1u : 0u;
        // the count launch's {pending, unmapped} (the stream put it ahead of this one), and
        // the words zero again for the next pass
        ans[3] = __hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ans[4] = __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rec[0] = 0;
        rec[1] = 0;
    }
}

// ---- fold/6 (lasp_core.erl:460-486) from a variable's cells and a fold process's tables ----
// AccValue = foldl(fun({X, C}, Acc) -> Acc ++ [{V, C} || V <- F(X)] end, [], Value): a held
// slot e emits one entry per row of its run frow[e] = {first, count} of the row pool, row r
// keyed ykey[r] with the cell's tokens named through tmap[r] in that key's rank row.  The
// count is O(1) per position (fmapped[e] says which token slots every row of e maps); the
// writer spreads a tile's output entries, not its positions, over the block.

// what slot e's cell gives: its entries and tokens; un: present tokens outside fmapped (the
// cell then emits nothing, as does a held slot F has not been asked about)
struct LfPos {
    Cnt c;
    uint32_t un;
};

__device__ __forceinline__ LfPos lf_pos(const LfFold& a, uint32_t e) {
    LfPos o{Cnt{0, 0}, 0};
    if (e >= a.Ein || e >= a.E) return o;
    const u64x2 C = *reinterpret_cast<const u64x2*>(a.in + 2ull * e);
    if (!C.x || !((a.evaluated[e >> 6] >> (e & 63u)) & 1ull)) return o;
    const uint32_t cnt = (uint32_t)(a.frow[e] >> 32);
    if (!cnt) return o;                                    // F(X) = []
    const u64 miss = C.x & ~a.fmapped[e];
    if (miss) {
        o.un = (uint32_t)__popcll(miss);
        return o;
    }
    o.c = Cnt{cnt, cnt * (uint32_t)__popcll(C.x)};
    return o;
}

__global__ __launch_bounds__(kLvT) void k_lf_count(LfFold a, u64* tiles, uint32_t* rec) {
    __shared__ Cnt lds[kLvT / 64];
    const uint32_t lane = threadIdx.x & 63u;
    // the pending check over this tile's element slots in slot order, as k_lm_count's
    {
        const uint32_t w0 = (blockIdx.x * kLvTile + (threadIdx.x & ~63u) * kLvI) >> 6;
        uint32_t pend = 0;
#pragma unroll
        for (uint32_t i = 0; i < kLvI; ++i) {
            const uint32_t w = w0 + i, s = 64u * w + lane;
            if (w >= a.words) break;                       // (wave-uniform)
            const bool held = s < a.Ein && a.in[2ull * s] != 0;
            const u64 pm = __ballot(held) & ~a.evaluated[w];
            if (lane == 0) a.pmask[w] = pm;
            pend += (uint32_t)__popcll(pm);
        }
        if (lane == 0 && pend) lm_rec_add(rec, pend);
    }
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    Cnt mine{0, 0};
    uint32_t un = 0;
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        const LfPos c = lf_pos(a, e[k]);
        mine.e += c.c.e;
        mine.t += c.c.t;
        un += c.un;
    }
    if (__ballot(un != 0)) {                               // (rare: a token minted since)
        for (int s = 32; s; s >>= 1) un += __shfl_xor(un, s, 64);
        if (lane == 0) lm_rec_add(rec + 1, un);
    }
    Cnt tot;
    lv_block_excl(mine, lds, &tot);
    if (threadIdx.x == 0) {
        tiles[2ull * blockIdx.x] = tot.e;
        tiles[2ull * blockIdx.x + 1] = tot.t;
    }
}

__global__ __launch_bounds__(kLvT) void k_lf_write(LfFold a, ListDev out, const u64* tiles,
                                                   uint32_t* rec, uint32_t* ans) {
    __shared__ Cnt lds[kLvT / 64];
    __shared__ uint32_t off_e[kLvTile], off_t[kLvTile];   // each position's exclusive offsets
    Cnt pre{0, 0};
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kLvT) {
        pre.e += (uint32_t)tiles[2ull * i];
        pre.t += (uint32_t)tiles[2ull * i + 1];
    }
    Cnt base;
    lv_block_excl(pre, lds, &base);
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    Cnt tot;
    {
        uint32_t e[kLvI];
        lv_slots(a, j0, e);
        Cnt c[kLvI], mine{0, 0};
#pragma unroll
        for (uint32_t k = 0; k < kLvI; ++k) {
            c[k] = lf_pos(a, e[k]).c;
            mine.e += c[k].e;
            mine.t += c[k].t;
        }
        Cnt ex = lv_block_excl(mine, lds, &tot);
#pragma unroll
        for (uint32_t k = 0; k < kLvI; ++k) {
            off_e[threadIdx.x * kLvI + k] = ex.e;
            off_t[threadIdx.x * kLvI + k] = ex.t;
            ex.e += c[k].e;
            ex.t += c[k].t;
        }
    }
    __syncthreads();
    // the tile's output entries over the block: entry i belongs to the last position whose
    // offset is <= i (one that emits: the positions without output share the next one's)
    for (uint32_t i = threadIdx.x; i < tot.e; i += kLvT) {
        uint32_t lo = 0, hi = kLvTile - 1;
        while (lo < hi) {
            const uint32_t mid = (lo + hi + 1) >> 1;
            if (off_e[mid] <= i) lo = mid;
            else hi = mid - 1;
        }
        const uint32_t j = blockIdx.x * kLvTile + lo;
        if (j >= a.n) continue;                            // (never: such a position emits nothing)
        const uint32_t e = a.elem_order[j];
        if (e >= a.Ein || e >= a.E) continue;              // (likewise)
        const u64x2 C = *reinterpret_cast<const u64x2*>(a.in + 2ull * e);
        const uint32_t pc = (uint32_t)__popcll(C.x), d = i - off_e[lo];
        const uint32_t pos = base.e + i;
        const u64 tp = (u64)base.t + off_t[lo] + (u64)d * pc;
        if (pos >= out.ce || tp + pc > out.ct) continue;
        const u64 row = (u64)(uint32_t)a.frow[e] + d;
        // whatever the row tables hold, the items name a slot below E and a token below 64
        bool bad = row >= a.rows;
        uint32_t y = bad ? e : a.ykey[row];
        if (y >= a.E) {
            bad = true;
            y = e;
        }
        u64 q = 0, qr = 0;
        if (!bad) {
            const uint8_t* tm = a.tmap + 64ull * row;
            for (u64 b = C.x; b; b &= b - 1) {
                const uint32_t k = (uint32_t)__builtin_ctzll(b), k2 = tm[k];
                if (k2 >= 64u || ((q >> k2) & 1ull)) {     // fmapped promised a slot of its own
                    bad = true;
                    break;
                }
                q |= 1ull << k2;
                qr |= ((C.y >> k) & 1ull) << k2;
            }
        }
        out.key[pos] = y;
        out.toff[pos] = (uint32_t)tp;
        if (bad) {
            ans[5] = 1;
            for (uint32_t t = 0; t < pc; ++t) out.tok[tp + t] = 64ull * y + t;
        } else {
            lv_run(out.tok + tp, y, q, qr, a.grank + 64ull * y);
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const uint32_t ne = base.e + tot.e, nt = base.t + tot.t;
        const bool over = ne > out.ce || nt > out.ct;
        out.hdr[0] = over ? 0u : ne;
        out.hdr[1] = over ? 0u : nt;
        out.toff[over ? 0u : ne] = over ? 0u : nt;
        ans[0] = ne;
        ans[1] = nt;
        ans[2] = over ? 1u : 0u;
        ans[3] = __hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        ans[4] = __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        rec[0] = 0;
        rec[1] = 0;
    }
}

// ---- product/7 (lasp_core.erl:499-533) from two variables' cells --------------------------
// AccValue = [{{X, Y}, orset_causal_product(Cx, Cy)} || {X, Cx} <- L, {Y, Cy} <- R]
// (lasp_lattice.erl:303-308: both foldls reversed).  The side pass compacts each side's held
// positions; with held counts nl, nr and token totals TL, TR the output is a closed form of
// the two sides' prefixes, so the write pass scans nothing (LvProd, laspj_internal.h).

constexpr u64 kLvPair = 1ull << 62;           // a pair key {X, Y} / a 2-list token [Tx, Ty]
constexpr u64 kLvId = 0x7FFFFFFFull;

__device__ __forceinline__ u64x2 lp_cell(const LvSide& s, uint32_t e) {
    if (e >= s.E) return u64x2{0, 0};
    return *reinterpret_cast<const u64x2*>(s.cells + 2ull * e);
}

__global__ __launch_bounds__(kLvT) void k_lp_count(LvProd a, u64* tiles) {
    __shared__ Cnt lds[kLvT / 64];
    const LvSide& s = a.s[blockIdx.y];
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    Cnt mine{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        const u64x2 C = lp_cell(s, e[k]);
        if (!C.x) continue;
        mine.e += 1;
        mine.t += (uint32_t)__popcll(C.x);
    }
    Cnt tot;
    lv_block_excl(mine, lds, &tot);
    if (threadIdx.x == 0) {
        const u64 at = (u64)blockIdx.y * gridDim.x + blockIdx.x;
        tiles[2 * at] = tot.e;
        tiles[2 * at + 1] = tot.t;
    }
}

__global__ __launch_bounds__(kLvT) void k_lp_side(LvProd a, const u64* tiles, uint32_t* ans) {
    __shared__ Cnt lds[kLvT / 64];
    const LvSide& s = a.s[blockIdx.y];
    const u64* mine_tiles = tiles + 2ull * blockIdx.y * gridDim.x;
    Cnt pre{0, 0};
    for (uint32_t i = threadIdx.x; i < blockIdx.x; i += kLvT) {
        pre.e += (uint32_t)mine_tiles[2ull * i];
        pre.t += (uint32_t)mine_tiles[2ull * i + 1];
    }
    Cnt base;
    lv_block_excl(pre, lds, &base);
    const uint32_t j0 = blockIdx.x * kLvTile + threadIdx.x * kLvI;
    uint32_t e[kLvI];
    lv_slots(a, j0, e);
    u64x2 C[kLvI];
    Cnt mine{0, 0};
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        C[k] = lp_cell(s, e[k]);
        if (!C[k].x) continue;
        mine.e += 1;
        mine.t += (uint32_t)__popcll(C[k].x);
    }
    Cnt tot;
    const Cnt ex = lv_block_excl(mine, lds, &tot);
    uint32_t pos = base.e + ex.e, tp = base.t + ex.t;
#pragma unroll
    for (uint32_t k = 0; k < kLvI; ++k) {
        if (!C[k].x) continue;
        const uint32_t c = (uint32_t)__popcll(C[k].x);
        // (held positions are at most n; the token arrays hold cap_t)
        if (pos < a.n && (u64)tp + c <= a.cap_t) {
            s.slot[pos] = e[k];
            s.tpre[pos] = tp;
            lv_run(s.run + tp, e[k], C[k].x, C[k].y, a.grank + 64ull * e[k]);
            for (uint32_t t = 0; t < c; ++t) s.own[tp + t] = pos;
        }
        pos += 1;
        tp += c;
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        const uint32_t ne = base.e + tot.e, nt = base.t + tot.t;
        const bool over = ne > a.n || nt > a.cap_t;
        if (!over) s.tpre[ne] = nt;
        ans[2 * blockIdx.y] = ne;
        ans[2 * blockIdx.y + 1] = nt;
        ans[4 + blockIdx.y] = over ? 1u : 0u;
    }
}

__global__ __launch_bounds__(256) void k_lp_write(LvProd a, uint32_t nl, uint32_t nr, uint32_t TL,
                                                  uint32_t TR, ListDev out, uint32_t* ans) {
    const LvSide& L = a.s[0];
    const LvSide& R = a.s[1];
    const u64 g = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 NE = (u64)nl * nr, NT = (u64)TL * TR;
    const bool over = NE > out.ce || NT > out.ct;
    if (!over && g < NE) {
        // entry o = i nr + j: l-major, the term order of the 2-tuples
        const uint32_t i = (uint32_t)(g / nr), j = (uint32_t)(g - (u64)i * nr);
        const uint32_t Ai = L.tpre[i], ai = L.tpre[i + 1] - Ai;
        out.key[g] = kLvPair | ((u64)(L.slot[i] & kLvId) << 31) | (R.slot[j] & kLvId);
        out.toff[g] = (uint32_t)((u64)Ai * TR + (u64)ai * R.tpre[j]);
    }
    if (!over && g < NT) {
        // token g: l's token g / TR names i; inside i's rows r's token rem / a_i names j
        const uint32_t q = (uint32_t)(g / TR);
        const uint32_t i = L.own[q];
        if (i < nl) {
            const uint32_t Ai = L.tpre[i], ai = L.tpre[i + 1] - Ai;
            const u64 rem = g - (u64)Ai * TR;
            const uint32_t m = ai ? (uint32_t)(rem / ai) : TR;
            const uint32_t j = m < TR ? R.own[m] : nr;
            if (j < nr) {
                const uint32_t Bj = R.tpre[j], bj = R.tpre[j + 1] - Bj;
                const u64 w = rem - (u64)ai * Bj;            // inside the a_i b_j run
                const uint32_t u = bj ? (uint32_t)(w / bj) : ai;
                if (u < ai) {
                    const uint32_t v = (uint32_t)(w - (u64)u * bj);
                    // both runs reversed, as the double foldl leaves them
                    const u64 X = L.run[Ai + (ai - 1 - u)], Y = R.run[Bj + (bj - 1 - v)];
                    out.tok[g] = kLvPair | ((X & kLvId) << 31) | (Y & kLvId) |
                                 ((X | Y) & kLvRemoved);     // XDeleted orelse YDeleted
                }
            }
        }
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) {
        out.hdr[0] = over ? 0u : (uint32_t)NE;
        out.hdr[1] = over ? 0u : (uint32_t)NT;
        out.toff[over ? 0u : (uint32_t)NE] = over ? 0u : (uint32_t)NT;
        ans[6] = over ? 1u : 0u;
    }
}

// one wave per element slot: lane j reads the slot of term-order place j of its tokens
__global__ __launch_bounds__(256) void k_lv_ranks(const uint32_t* __restrict__ elem_order,
                                                  const uint8_t* __restrict__ tok_order, uint32_t E,
                                                  uint32_t* __restrict__ krank,
                                                  uint32_t* __restrict__ grank,
                                                  const uint32_t* __restrict__ dirty, uint32_t nd) {
    const u64 t = (u64)blockIdx.x * 256 + threadIdx.x;
    const u64 w = t >> 6;
    const uint32_t j = (uint32_t)(t & 63u);
    if (!dirty && t < E) {
        const uint32_t e = elem_order[t];
        if (e < E) krank[e] = (uint32_t)t;
    }
    if (w >= (dirty ? nd : E)) return;
    const uint32_t e = dirty ? dirty[w] : (uint32_t)w;
    if (e >= E) return;
    const uint32_t k = tok_order[64ull * e + j];
    if (k < 64u) grank[64ull * e + k] = j;
}

}  // namespace

hipError_t launch_lv_ranks(laspj_ctx* ctx, const uint32_t* elem_order, const uint8_t* tok_order,
                           uint32_t E, uint32_t* krank, uint32_t* grank, const uint32_t* dirty,
                           uint32_t ndirty) {
    if (!E || (dirty && !ndirty)) return hipSuccess;
    const uint64_t waves = dirty ? ndirty : E;
    hipLaunchKernelGGL(k_lv_ranks, dim3((unsigned)((waves * 64 + 255) / 256)), dim3(256), 0,
                       ctx->stream, elem_order, tok_order, E, krank, grank, dirty, ndirty);
    return hipGetLastError();
}

hipError_t launch_lv_isect(laspj_ctx* ctx, const LvIsect& a, const ListDev& out, uint64_t* tiles,
                           uint32_t* ans) {
    const uint32_t ntile = lv_isect_tiles(a.n);
    hipLaunchKernelGGL(k_lv_count, dim3(ntile), dim3(kLvT), 0, ctx->stream, a, tiles);
    hipLaunchKernelGGL(k_lv_write, dim3(ntile), dim3(kLvT), 0, ctx->stream, a, out, tiles, ans);
    return hipGetLastError();
}

hipError_t launch_lp_sides(laspj_ctx* ctx, const LvProd& a, uint64_t* tiles, uint32_t* ans) {
    const dim3 grid(lv_isect_tiles(a.n), 2);
    hipLaunchKernelGGL(k_lp_count, grid, dim3(kLvT), 0, ctx->stream, a, tiles);
    hipLaunchKernelGGL(k_lp_side, grid, dim3(kLvT), 0, ctx->stream, a, tiles, ans);
    return hipGetLastError();
}

hipError_t launch_lp_write(laspj_ctx* ctx, const LvProd& a, uint32_t nl, uint32_t nr, uint32_t TL,
                           uint32_t TR, const ListDev& out, uint32_t* ans) {
    const uint64_t span = std::max<uint64_t>({(uint64_t)nl * nr, (uint64_t)TL * TR, 1});
    hipLaunchKernelGGL(k_lp_write, dim3((unsigned)((span + 255) / 256)), dim3(256), 0, ctx->stream,
                       a, nl, nr, TL, TR, out, ans);
    return hipGetLastError();
}

hipError_t launch_lm_map(laspj_ctx* ctx, const LmMap& a, const ListDev& out, uint64_t* tiles,
                         uint32_t* rec, uint32_t* ans, bool count_only) {
    const uint32_t ntile = lv_isect_tiles(a.n);
    hipLaunchKernelGGL(k_lm_count, dim3(ntile), dim3(kLvT), 0, ctx->stream, a, tiles, rec);
    if (!count_only)
        hipLaunchKernelGGL(k_lm_write, dim3(ntile), dim3(kLvT), 0, ctx->stream, a, out, tiles, rec,
                           ans);
    return hipGetLastError();
}

hipError_t launch_lf_fold(laspj_ctx* ctx, const LfFold& a, const ListDev& out, uint64_t* tiles,
                          uint32_t* rec, uint32_t* ans, bool count_only) {
    const uint32_t ntile = lv_isect_tiles(a.n);
    hipLaunchKernelGGL(k_lf_count, dim3(ntile), dim3(kLvT), 0, ctx->stream, a, tiles, rec);
    if (!count_only)
        hipLaunchKernelGGL(k_lf_write, dim3(ntile), dim3(kLvT), 0, ctx->stream, a, out, tiles, rec,
                           ans);
    return hipGetLastError();
}

}  // namespace laspj
