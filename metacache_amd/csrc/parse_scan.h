// metacache_amd/csrc/parse_scan.h -- what the byte passes of parse.hip and parse_cut.hip share: the tile, and the block scans that turn
// a thread's values into what lies in front of the thread.  Device code; internal.
#pragma once

#include "rows_common.h"

namespace mcamd {
namespace parsek {

constexpr uint32_t kBlock = 256, kWaves = kBlock / 64, kTile = kBlock * 16, kNone = 0xFFFFFFFFu;

// ---- block scans: every thread of the block calls them; the values become what lies in front of the thread, tot the block's ----------
template <int NS, int NM>
__device__ __forceinline__ void block_excl_scan(uint32_t (&s)[NS], uint32_t (&m)[NM], uint32_t (&sTot)[NS], uint32_t (&mTot)[NM], uint32_t* lds /* [(NS + NM) * kWaves] */)
{
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    uint32_t si[NS], mi[NM];
#pragma unroll
    for (int k = 0; k < NS; ++k) { si[k] = wave_incl_scan_u32(s[k], lane); if (lane == 63) lds[k * kWaves + wave] = si[k]; }
#pragma unroll
    for (int k = 0; k < NM; ++k) { mi[k] = wave_incl_scan_max_u32(m[k]); if (lane == 63) lds[(NS + k) * kWaves + wave] = mi[k]; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < NS; ++k) {
        uint32_t base = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) { const uint32_t x = lds[k * kWaves + w]; if (w < wave) base += x; all += x; }
        s[k] = base + si[k] - s[k];
        sTot[k] = all;
    }
#pragma unroll
    for (int k = 0; k < NM; ++k) {
        uint32_t base = 0, all = 0;
#pragma unroll
        for (uint32_t w = 0; w < kWaves; ++w) { const uint32_t x = lds[(NS + k) * kWaves + w]; if (w < wave) base = max(base, x); all = max(all, x); }
        const uint32_t up = (uint32_t)__shfl_up((int)mi[k], 1);
        m[k] = max(base, lane ? up : 0u);
        mTot[k] = all;
    }
    __syncthreads();
}

__device__ __forceinline__ uint32_t block_min(uint32_t v, uint32_t* lds /* [kWaves] */)
{
    v = wave_min_u32(v);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = lds[0];
#pragma unroll
    for (uint32_t w = 1; w < kWaves; ++w) r = min(r, lds[w]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ uint32_t block_max(uint32_t v, uint32_t* lds /* [kWaves] */)
{
    v = wave_max_u32(v);
    if ((threadIdx.x & 63u) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    uint32_t r = lds[0];
#pragma unroll
    for (uint32_t w = 1; w < kWaves; ++w) r = max(r, lds[w]);
    __syncthreads();
    return r;
}

}  // namespace parsek
}  // namespace mcamd
