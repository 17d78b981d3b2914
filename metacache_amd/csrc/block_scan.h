// metacache_amd/csrc/block_scan.h -- the block scans: a thread's values become what lies in front of the thread in its block.  The 32-bit
// forms (sums and maxima, several at a time, through the wave scans of device_common.h) are the byte passes'; the 64-bit form and
// tile_scan_kernel are those of the count / scan / write sequences of format.hip and table_info.hip.
// EVERY scan here assumes a block of kScanBlock = 256 threads, all of which call it; a file that uses them static_asserts its own kBlock.
// Device code; internal.
#pragma once

#include "device_common.h"

namespace mcamd {

constexpr uint32_t kScanBlock = 256;

namespace parsek {

constexpr uint32_t kBlock = kScanBlock, kWaves = kBlock / 64;

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

// exclusive scan of one 64-bit value per thread of the block; total = the block's sum.  sc: kScanBlock entries of LDS.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* sc, uint64_t& total)
{
    const uint32_t t = threadIdx.x;
    sc[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kScanBlock; d <<= 1) {
        const uint64_t add = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    total = sc[kScanBlock - 1];
    const uint64_t incl = sc[t];
    __syncthreads();
    return incl - v;
}

namespace {

// sums[tiles] -> their exclusive scan in place, *total = the grand total (one block).  Internal linkage, and a template (T: uint64_t): an
// object that launches it holds its own, one that does not holds none.
template <class T>
__global__ __launch_bounds__(kScanBlock) void tile_scan_kernel(T* __restrict__ sums, uint32_t tiles, T* __restrict__ total)
{
    __shared__ T sc[kScanBlock];
    T carry = 0;
    for (uint32_t base = 0; base < tiles; base += kScanBlock) {                  // (the same trips for every lane)
        const uint32_t j = base + threadIdx.x;
        const T v = j < tiles ? sums[j] : 0;
        T chunk;
        const T excl = block_excl_scan(v, sc, chunk);
        if (j < tiles) sums[j] = carry + excl;
        carry += chunk;
    }
    if (threadIdx.x == 0) *total = carry;
}

}  // namespace

}  // namespace mcamd
