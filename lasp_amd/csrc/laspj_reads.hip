// The read side's check over resident variables (include/laspj.h "lazy threads and
// one-pass reads"): the kernel of laspj_var_read / laspj_var_read_any /
// laspj_var_wait_needed.  The host side (hidden cells, lazy lists, the fold of read_any) is
// in laspj_nif_waiters.hip and laspj_reads_host.cpp.
//
// read/6 (lasp_core.erl:331-364) and each step of read_any/3's fold (:371-420) ask, of one
// threshold T,
//   threshold_met(Type, LazyThreshold_j, T)  for every lazy thread j  (reply_to_all, :795-813)
//   threshold_met(Type, Value, T)                                      (:352)
// which is is_inflation / is_strict_inflation (lasp_lattice.erl:62-75) with T as the
// previous state and 1 + L current states: the value and each lazy threshold.  k_waiter_check
// (laspj_nif_waiters.hip) tests many previous states against one current state; this is the
// transpose.  A wave item is one tile of kReadTile 16-byte units of one read: T's two units
// per lane are loaded once and held in registers, the currents are taken in chunks of
// kReadChunk (one descriptor per lane, handed round by shuffles), their loads issued four
// at a time ahead of their use.  Units, modes and predicates are k_waiter_check's (the
// comment above kWaitTile), roles swapped:
//   OR-Set: violation = some cell has pT & ~pC; strict also needs a common element's cell
//     to differ, removed flags included, or nT < nC
//   wide: the same per {p, r} pair; strict = and some pair differs
//   G-Set: violation = t & ~c; strict also needs the words to differ
// Records (zeroed ahead of the launch): per current {flags: 1 violation, 2 changed; nC},
// per read nT (each tile is one wave's: counted once); device-scope atomics, one per wave
// and nonzero result.  The met bytes are written by a one-block finish launch behind the
// check (the stream orders them: no wave waits for another).  No LDS, no scratch.

#include "laspj_internal.h"

namespace laspj {

namespace {

typedef unsigned long long read2 __attribute__((ext_vector_type(2)));

// unit q of a block of `words` u64 words (as wait_ld of laspj_nif_waiters.hip: units past the end
// are absent, an odd last word is a unit's first half; null cells have no words)
__device__ __forceinline__ read2 read_ld(const uint64_t* base, uint64_t q, uint32_t words) {
    read2 v = {0ull, 0ull};
    if (2 * q + 1 < words) v = *reinterpret_cast<const read2*>(base + 2 * q);
    else if (2 * q < words) v.x = base[2 * q];
    return v;
}

__global__ void __launch_bounds__(256) k_read_check(const ReadDesc* rds, uint32_t n,
                                                    const ReadCur* cs, uint64_t items,
                                                    uint32_t* rec, uint32_t* np) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4;
    for (uint64_t s = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6; s < items; s += nwaves) {
        uint32_t lo = 0, hi = n;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (rds[mid].item0 <= s) lo = mid;
            else hi = mid;
        }
        const ReadDesc R = rds[lo];
        const uint32_t mode = R.mode_strict >> 1;
        const uint64_t q0 = (s - R.item0) * kReadTile + lane, q1 = q0 + 64;
        const read2 t0 = read_ld(R.cells, q0, R.words), t1 = read_ld(R.cells, q1, R.words);
        if (mode == kReadNarrow) {
            const uint32_t k = __popcll(__ballot(t0.x != 0)) + __popcll(__ballot(t1.x != 0));
            if (lane == 0 && k) atomicAdd(np + lo, k);
        }
        const uint32_t jend = R.c0 + R.nc;
        for (uint32_t j0 = R.c0; j0 < jend; j0 += kReadChunk) {
            const uint32_t j1 = min(jend, j0 + kReadChunk);
            // the chunk's descriptors: one per lane, handed round by shuffles
            uint64_t dp = 0;
            uint32_t dw = 0;
            if (j0 + lane < j1) {
                dp = reinterpret_cast<uint64_t>(cs[j0 + lane].cells);
                dw = cs[j0 + lane].words;
            }
            for (uint32_t j = j0; j < j1; j += 4) {
                read2 c0[4], c1[4];
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    // (lanes past the chunk hold no words: nothing is read for them)
                    const auto* C = reinterpret_cast<const uint64_t*>(
                        (uint64_t)__shfl((unsigned long long)dp, (int)(j + k - j0), 64));
                    const uint32_t w = __shfl(dw, (int)(j + k - j0), 64);
                    c0[k] = read_ld(C, q0, w);
                    c1[k] = read_ld(C, q1, w);
                }
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k) {
                    if (j + k >= j1) break;
                    const read2 a = c0[k], b = c1[k];
                    bool viol, changed;
                    uint32_t ncur = 0;
                    if (mode == kReadNarrow) {
                        viol = ((t0.x & ~a.x) | (t1.x & ~b.x)) != 0;
                        changed = ((t0.x != 0) & (a.x != 0) & ((t0.x != a.x) | (t0.y != a.y))) |
                                  ((t1.x != 0) & (b.x != 0) & ((t1.x != b.x) | (t1.y != b.y)));
                        ncur = __popcll(__ballot(a.x != 0)) + __popcll(__ballot(b.x != 0));
                    } else if (mode == kReadWide) {
                        viol = ((t0.x & ~a.x) | (t1.x & ~b.x)) != 0;
                        changed = (t0.x != a.x) | (t0.y != a.y) | (t1.x != b.x) | (t1.y != b.y);
                    } else {
                        viol = ((t0.x & ~a.x) | (t0.y & ~a.y) | (t1.x & ~b.x) | (t1.y & ~b.y)) != 0;
                        changed = (t0.x != a.x) | (t0.y != a.y) | (t1.x != b.x) | (t1.y != b.y);
                    }
                    const uint32_t f = (__ballot(viol) != 0 ? 1u : 0u) | (__ballot(changed) != 0 ? 2u : 0u);
                    if (lane == 0) {
                        if (f) atomicOr(rec + 2 * (j + k), f);
                        if (ncur) atomicAdd(rec + 2 * (j + k) + 1, ncur);
                    }
                }
            }
        }
    }
}

// wait_finish's rule (laspj_nif_waiters.hip) with the roles swapped: current j of read i is met when
// T_i -> C_j is an inflation, strictly so for a strict read
__global__ void __launch_bounds__(256) k_read_finish(const ReadDesc* rds, const ReadCur* cs,
                                                     uint32_t ncs, uint32_t* rec, uint32_t* np,
                                                     uint8_t* met) {
    for (uint32_t j = threadIdx.x; j < ncs; j += 256) {
        const uint32_t i = cs[j].read, ms = rds[i].mode_strict;
        const uint32_t f = __hip_atomic_load(rec + 2 * j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t ncur = __hip_atomic_load(rec + 2 * j + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const uint32_t npv = __hip_atomic_load(np + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const bool infl = !(f & 1u);
        bool res = infl;
        if (ms & 1u) res = infl && ((f & 2u) || ((ms >> 1) == kReadNarrow && npv < ncur));
        met[j] = res ? 1 : 0;
    }
}

}  // namespace

hipError_t launch_read_check(laspj_ctx* ctx, const ReadDesc* rds, uint32_t n, const ReadCur* cs,
                             uint32_t ncs, uint64_t items, uint32_t* rec, uint8_t* met) {
    if (!n || !ncs) return hipSuccess;
    uint32_t* np = rec + 2ull * ncs;
    hipError_t e = hipMemsetAsync(rec, 0, read_rec_bytes(n, ncs), ctx->stream);
    if (e != hipSuccess) return e;
    if (items) {
        const unsigned grid = (unsigned)std::max<uint64_t>(
            1, std::min<uint64_t>((items + 3) / 4, (uint64_t)ctx->cus * 8));
        hipLaunchKernelGGL(k_read_check, dim3(grid), dim3(256), 0, ctx->stream, rds, n, cs, items,
                           rec, np);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    hipLaunchKernelGGL(k_read_finish, dim3(1), dim3(256), 0, ctx->stream, rds, cs, ncs, rec, np, met);
    return hipGetLastError();
}

}  // namespace laspj
