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

// the element slots of a thread's four positions (kLvNoElem past the last position)
__device__ __forceinline__ void lv_slots(const LvIsect& a, uint32_t j0, uint32_t* e) {
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

}  // namespace laspj
