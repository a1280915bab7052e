// The wave and workgroup primitives of every HIP unit, stated once (reached through common.h; gfx950: 64 lanes).
//
// Reductions over the 64 lanes are the xor butterfly: after it EVERY lane holds the result, and the order of the operations is
// the same in every lane and every run.  The sums built on it below (block_sum, wave_sum_rows) add in one fixed order and use
// no atomics: they are the library's bitwise reproducible sums ("Reproducible sums").
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

namespace mgs {

// ---- the butterfly, written once ------------------------------------------------------------------------------------------------
// v = OP(v, the partner lane's v) over the lane distances 32 .. 1.  A statement, for the sites where the compiler schedules the
// inlined function differently from the loop written in place (DESIGN.md names them); everything else calls the functions below.
#define MGS_WAVE_ADD(a, b) ((a) + (b))
#define MGS_WAVE_REDUCE(v, OP) \
    _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) v = OP(v, __shfl_xor(v, o_, 64))
// two values in one pass (the two shuffles of a step in flight together)
#define MGS_WAVE_REDUCE2(a, OPA, b, OPB) \
    _Pragma("unroll") for (int o_ = 32; o_ > 0; o_ >>= 1) { a = OPA(a, __shfl_xor(a, o_, 64)); b = OPB(b, __shfl_xor(b, o_, 64)); }

// ---- one value over the wave; every lane gets the result -------------------------------------------------------------------
template <typename T>                       // float, double, uint32_t
__device__ __forceinline__ T wave_sum(T v) { MGS_WAVE_REDUCE(v, MGS_WAVE_ADD); return v; }
__device__ __forceinline__ float wave_max(float v) { MGS_WAVE_REDUCE(v, fmaxf); return v; }
__device__ __forceinline__ float wave_min(float v) { MGS_WAVE_REDUCE(v, fminf); return v; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { MGS_WAVE_REDUCE(v, max); return v; }
// minimum over the 64 lanes on the DPP data path, returned to every lane: four row shifts, two row broadcasts, one lane read
__device__ __forceinline__ uint32_t wave_min_dpp(uint32_t v) {
#define MGS_DPP_MIN(ctrl, row_mask) v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, ctrl, row_mask, 0xf, false))
    MGS_DPP_MIN(0x111, 0xf);      // row_shr:1
    MGS_DPP_MIN(0x112, 0xf);      // row_shr:2
    MGS_DPP_MIN(0x114, 0xf);      // row_shr:4
    MGS_DPP_MIN(0x118, 0xf);      // row_shr:8   -> lane 15 of each row holds the row's minimum
    MGS_DPP_MIN(0x142, 0xa);      // row_bcast:15 into rows 1, 3
    MGS_DPP_MIN(0x143, 0xc);      // row_bcast:31 into rows 2, 3 -> lane 63 holds the wave's
#undef MGS_DPP_MIN
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}
// the value of one lane (a wave-uniform index) in a scalar register
__device__ __forceinline__ uint32_t bcast(uint32_t v, int lane) {
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}

// ---- 64-lane inclusive scans ------------------------------------------------------------------------------------------------
// u32 add on the DPP data path: 4 row shifts + 2 row broadcasts, ~60 cycles, instead of six __shfl_up round trips through
// ds_bpermute (the LDS crossbar, >100 cycles each).
__device__ __forceinline__ uint32_t wave_incl_scan_dpp(uint32_t v) {
#define MGS_DPP_ADD(ctrl, row_mask) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, ctrl, row_mask, 0xf, false)
    MGS_DPP_ADD(0x111, 0xf);      // row_shr:1
    MGS_DPP_ADD(0x112, 0xf);      // row_shr:2
    MGS_DPP_ADD(0x114, 0xf);      // row_shr:4
    MGS_DPP_ADD(0x118, 0xf);      // row_shr:8   -> inclusive within each row of 16
    MGS_DPP_ADD(0x142, 0xa);      // row_bcast:15 into rows 1, 3
    MGS_DPP_ADD(0x143, 0xc);      // row_bcast:31 into rows 2, 3
#undef MGS_DPP_ADD
    return v;
}
// u64 add (DPP moves 32 bits): the __shfl_up ladder
__device__ __forceinline__ uint64_t wave_incl_scan_u64(uint64_t v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t u = (uint64_t)__shfl_up((unsigned long long)v, o, 64);
        v += lane >= o ? u : 0ull;
    }
    return v;
}

// ---- the reproducible sums ----------------------------------------------------------------------------------------------------
// Sum over a workgroup of 256 threads = four waves, in a fixed order: the butterfly, lane 0 of each wave to LDS (s_a: four
// entries), ONE barrier, then ((w0 + w1) + (w2 + w3)).  Every thread gets the sum.  (The butterfly as a statement, not a call of
// wave_sum: the call moved one instruction of the label kernels.)
template <typename A>
__device__ __forceinline__ A block_sum(A a, A* s_a) {
    MGS_WAVE_REDUCE(a, MGS_WAVE_ADD);
    if ((threadIdx.x & 63) == 0) s_a[threadIdx.x >> 6] = a;
    __syncthreads();
    return (s_a[0] + s_a[1]) + (s_a[2] + s_a[3]);
}
// two values, of possibly different types, behind the same barrier
template <typename A, typename B>
__device__ __forceinline__ void block_sum(A& a, B& b, A* s_a, B* s_b) {
    MGS_WAVE_REDUCE2(a, MGS_WAVE_ADD, b, MGS_WAVE_ADD);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (lane == 0) { s_a[wv] = a; s_b[wv] = b; }
    __syncthreads();
    a = (s_a[0] + s_a[1]) + (s_a[2] + s_a[3]);
    b = (s_b[0] + s_b[1]) + (s_b[2] + s_b[3]);
}
// One wave adds per-workgroup partials in a fixed order: lane l adds rows l, l + 64, ... (N values each, `stride` apart), then
// the butterfly.  Every lane gets the N totals.
template <int N, typename T>
__device__ __forceinline__ void wave_sum_rows(const T* __restrict__ rows, size_t stride, int nrows, int lane, T (&v)[N]) {
#pragma unroll
    for (int k = 0; k < N; ++k) v[k] = T(0);
    for (int b = lane; b < nrows; b += 64) {
        const T* o = rows + (size_t)b * stride;
#pragma unroll
        for (int k = 0; k < N; ++k) v[k] += o[k];
    }
#pragma unroll
    for (int k = 0; k < N; ++k) MGS_WAVE_REDUCE(v[k], MGS_WAVE_ADD);
}

}  // namespace mgs
