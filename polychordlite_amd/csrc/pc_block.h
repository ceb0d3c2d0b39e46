// pc_block.h -- the two device helpers that more than one of the contraction's files needs: block_argmin (k_consume of pc_contract.hip,
// k_install_live of pc_rows.hip) and wave_copy_masked (the row kernels of pc_rows.hip, k_clean_scatter of pc_update_steps.hip).  Not in pc_dev.h:
// that header is embedded and handed to hiprtc for every source handle, and nothing the run-time unit launches uses these.
#pragma once
#include "pc_state.h"

// ------------------------------------------------------------------------------------------
// block-level helpers (NT threads; NT == 64 needs no barrier traffic)
// ------------------------------------------------------------------------------------------
template <int NT>
__device__ __forceinline__ vk_t block_argmin(vk_t v, vk_t *scratch)
{
    v = wave_argmin(v);
    if (NT == 64) return v;
    const int wid = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) scratch[wid] = v;
    __syncthreads();
    vk_t r = scratch[0];
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) r = vk_min(r, scratch[i]);
    __syncthreads();
    return r;
}

// Copy the rows selected by a wave-uniform bit mask (row of bit b = src0 + b*nT) to consecutive rows at dst.
// Eight rows travel together: their loads are independent, so a batch costs one memory round trip
// instead of eight (rows written by other XCDs come from HBM / Infinity Cache, ~1 us each).
__device__ __forceinline__ int wave_copy_masked(const double *src0, unsigned long long mask, double *dst, int nT, int lane)
{
    int n = 0;
    while (mask) {
        int idx[8], cnt = 0;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            idx[u] = 0;
            if (mask) { idx[u] = __ffsll((long long)mask) - 1; mask &= mask - 1; cnt = u + 1; }
        }
        for (int e = lane; e < nT; e += 64) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (u < cnt) v[u] = src0[(size_t)idx[u] * nT + e];
#pragma unroll
            for (int u = 0; u < 8; ++u) if (u < cnt) dst[(size_t)(n + u) * nT + e] = v[u];
        }
        n += cnt;
    }
    return n;
}
