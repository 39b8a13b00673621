// lasp_process re-runs over resident variables (include/laspj.h "resident processes"): the
// kernels of laspj_filter_run / laspj_filter_run_many / laspj_var_intersection.  The host
// side (handles, lifecycle, the fun table's host mirror) is in laspj_nif_process.hip.
//
// filter/6 (lasp_core.erl:681-712) keeps the entries of `in` whose Function(V) =:= true;
// the fun's results live beside the variable as two bitmaps over the namespace's element
// slots (evaluated: F was called; keep: it answered true), so a re-run is
//   pending  = |{slots held by in} \ evaluated|
//   AccValue = in's cells masked by keep            (valid when pending == 0)
//   bind/3 (:291-312): Value0 =:= AccValue ? no-op : out |= AccValue
// intersection/7 for G-Sets (:569-576) is the same with r's bitmap as the mask and nothing
// ever pending.  These are latency-bound: a value is a few KiB, so the shape aims at one
// launch per answer and one device-scope atomic per wave with something to report.
//
// A pass is kProcCheck (counts pending, decides changed, leaves each wave's pending mask in
// the filter's pmask; writes no cell), kProcWrite (a process whose record says pending == 0
// and changed: out |= AccValue) or kProcFused (both at once, where nothing can be pending).

#include "laspj_internal.h"

namespace laspj {

namespace {

typedef unsigned long long proc2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ proc2 ld2(const uint64_t* p) {
    return *reinterpret_cast<const proc2*>(p);
}
__device__ __forceinline__ void st2(uint64_t* p, proc2 v) { *reinterpret_cast<proc2*>(p) = v; }

__device__ __forceinline__ void rec_add(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rec_or(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_or(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// block `blk` of one process (256 lanes); rec = its {pending, changed}
__device__ __forceinline__ void proc_block(const ProcDesc& d, uint32_t blk, uint32_t* rec,
                                           uint32_t pass) {
    if (pass == kProcWrite) {
        // only a process known ready and unequal writes (block-uniform)
        const uint32_t pend = __hip_atomic_load(rec, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t chg = __hip_atomic_load(rec + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (pend != 0 || chg == 0) return;
    }
    const bool check = pass != kProcWrite, write = pass != kProcCheck;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t u = blk * 256u + threadIdx.x;         // element slot / bitmap word
    if (d.mode == kProcGset) {
        // one lane per bitmap word: value, evaluated and keep share the slot numbering
        uint32_t pend = 0;
        bool ch = false;
        if (u < d.n) {
            const uint64_t in = d.in[u], o = d.out[u];
            const uint64_t acc = in & d.keep[u];
            if (check) {
                const uint64_t pm = d.evaluated ? in & ~d.evaluated[u] : 0ull;
                if (d.pmask) d.pmask[u] = pm;
                pend = (uint32_t)__popcll(pm);
                ch = o != acc;                           // Value0 =/= AccValue
            }
            if (write && (o | acc) != o) d.out[u] = o | acc;
        }
        if (check) {
            for (int s = 32; s; s >>= 1) pend += __shfl_xor(pend, s, 64);
            const bool any = __ballot(ch) != 0;
            if (lane == 0 && pend) rec_add(rec, pend);
            if (lane == 0 && any) rec_or(rec + 1, 1u);
        }
        return;
    }
    // OR-Sets, one lane per element slot: a wave's 64 slots are one word of each bitmap
    const uint32_t w = __builtin_amdgcn_readfirstlane(u >> 6);
    if (64u * w >= d.n) return;                          // (the wave is past the last slot)
    const uint64_t ev = d.evaluated ? d.evaluated[w] : ~0ull;
    const bool keep = (d.keep[w] >> lane) & 1ull;
    const bool live = u < d.n;
    bool present = false, ch = false;
    if (d.mode == kProcNarrow) {
        proc2 c = {0ull, 0ull}, o = {0ull, 0ull};
        if (live) {
            c = ld2(d.in + 2ull * u);                    // a wave: 1 KiB, coalesced
            o = ld2(d.out + 2ull * u);
        }
        present = c.x != 0;
        const proc2 a = keep ? c : proc2{0ull, 0ull};
        ch = o.x != a.x || o.y != a.y;
        if (write && live && ((o.x | a.x) != o.x || (o.y | a.y) != o.y))
            st2(d.out + 2ull * u, proc2{o.x | a.x, o.y | a.y});
    } else if (live) {
        const uint64_t base = 2ull * u * d.tw;
        for (uint32_t j = 0; j < d.tw; ++j) {
            const proc2 c = ld2(d.in + base + 2 * j), o = ld2(d.out + base + 2 * j);
            present |= c.x != 0;
            const proc2 a = keep ? c : proc2{0ull, 0ull};
            ch |= o.x != a.x || o.y != a.y;
            if (write && ((o.x | a.x) != o.x || (o.y | a.y) != o.y))
                st2(d.out + base + 2 * j, proc2{o.x | a.x, o.y | a.y});
        }
    }
    if (check) {
        const uint64_t pm = __ballot(present) & ~ev;
        const bool any = __ballot(ch) != 0;
        if (lane == 0) {
            if (d.pmask) d.pmask[w] = pm;
            if (pm) rec_add(rec, (uint32_t)__popcll(pm));
            if (any) rec_or(rec + 1, 1u);
        }
    }
}

__global__ void __launch_bounds__(256) k_proc_one(ProcDesc d, uint32_t* rec, uint32_t pass) {
    proc_block(d, blockIdx.x, rec, pass);
}

// n processes in one launch: block b belongs to the last descriptor whose block0 <= b (a
// process with no blocks shares its block0 with its successor and is never chosen)
__global__ void __launch_bounds__(256) k_proc_many(const ProcDesc* __restrict__ ds, uint32_t n,
                                                   uint32_t* rec, uint32_t pass) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) / 2;
        if (ds[mid].block0 <= blockIdx.x) lo = mid;
        else hi = mid;
    }
    const ProcDesc d = ds[lo];
    proc_block(d, blockIdx.x - d.block0, rec + 2 * lo, pass);
}

}  // namespace

uint32_t proc_blocks(const ProcDesc& d) { return (d.n + 255u) / 256u; }

hipError_t launch_proc_one(laspj_ctx* ctx, const ProcDesc& d, uint32_t* rec, uint32_t pass) {
    const uint32_t blocks = proc_blocks(d);
    if (!blocks) return hipSuccess;
    hipLaunchKernelGGL(k_proc_one, dim3(blocks), dim3(256), 0, ctx->stream, d, rec, pass);
    return hipGetLastError();
}

hipError_t launch_proc_many(laspj_ctx* ctx, const ProcDesc* descs, uint32_t n, uint32_t blocks,
                            uint32_t* rec, uint32_t pass) {
    if (!blocks || !n) return hipSuccess;
    hipLaunchKernelGGL(k_proc_many, dim3(blocks), dim3(256), 0, ctx->stream, descs, n, rec, pass);
    return hipGetLastError();
}

}  // namespace laspj
