// metacache_amd/csrc/table_info.hip -- what a loaded table HOLDS, read back from the device: mc_table_histogram, mc_table_features,
// mc_table_lookup (include/metacache_amd.h, "table content").  The reference answers `info <db> statistics | featurecounts | featuremap`
// from its hash table (host_hashmap.hpp:376-445; its GPU build reduces the size statistics on the device, gpu_hashmap.cu:278-321); here
// the bucket table in HBM is the only copy there is, so the same questions are three small kernel sequences over it:
//   table_hist_kernel        one pass over the buckets' size words: 256 (+1) private 32-bit bins per block in LDS, flushed once with one
//                            64-bit atomic per non-zero bin.  Everything on the statistics line follows on the host in exact integers.
//   table_enumerate          the occupied slots as (key << 16) | size words: count per tile, scan of the tile counts, write -- no block
//                            waits for another (the three-launch shape of format.hip) -- then the library's radix sort on the key bits.
//                            Slot placement depends on the insert order (table_build.hip); the sort is what makes the output deterministic.
//   table_lookup             sizes: one lane per requested key walks its probe sequence and leaves size and payload; the same count /
//                            scan / write shape turns the sizes into offsets; gather: one thread per OUTPUT location finds its list by a
//                            binary search in the offsets (the pattern of table_values_kernel) and takes the location from the inline
//                            payload, the 8-byte store or the compact store (gw_widen).  Stores to the output are lane-consecutive.
// All three work on the buckets alone (never the direct-address index), wait for their own work and keep nothing in the context.
#include "rows_common.h"
#include "block_scan.h"

#include <rocprim/device/device_radix_sort.hpp>

#include <string>
#include <vector>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256;
static_assert(kBlock == kScanBlock, "the scans of block_scan.h are for blocks of 256 threads");
constexpr uint32_t kMaxTiles = 2048;             // tiles of the count / scan / write sequences: one single-block scan reaches them all
constexpr uint32_t kBins = 256;                  // hist[0 .. 255]; bin 256 collects what mc_table_* does not support (sizes above 255)
constexpr uint32_t kPieceKeys = 1u << 22;        // mc_table_lookup: keys per staged piece
constexpr uint64_t kPieceLocs = 1ull << 26;      // ... and locations per gather launch (512 MB of staging at the most)
constexpr uint64_t kPieceWords = 1ull << 22;     // mc_table_features: words per copy to the host
constexpr uint32_t kFlagSize = 1, kFlagStore = 2;

// the four u16 sizes of a bucket in one 8-byte load (0 = free slot)
__device__ __forceinline__ uint64_t bucket_sizes(const TableBucket* buckets, uint64_t b) { return *reinterpret_cast<const uint64_t*>(buckets[b].size); }
__device__ __forceinline__ uint32_t occupied(uint64_t sz)
{
    return ((sz & 0xFFFFull) != 0) + ((sz & 0xFFFF0000ull) != 0) + ((sz & 0xFFFF00000000ull) != 0) + ((sz >> 48) != 0);
}

__global__ __launch_bounds__(kBlock) void table_hist_kernel(const TableBucket* __restrict__ buckets, uint32_t nbuckets, unsigned long long* __restrict__ hist)
{
    __shared__ uint32_t bins[kBins + 1];
    for (uint32_t t = threadIdx.x; t <= kBins; t += kBlock) bins[t] = 0;
    __syncthreads();
    for (uint64_t b = (uint64_t)blockIdx.x * kBlock + threadIdx.x; b < nbuckets; b += (uint64_t)gridDim.x * kBlock) {
        const uint64_t sz = bucket_sizes(buckets, b);
#pragma unroll
        for (uint32_t j = 0; j < kSlotsPerBucket; ++j) {
            const uint32_t s = (uint32_t)(sz >> (16 * j)) & 0xFFFFu;
            if (s) atomicAdd(&bins[min(s, kBins)], 1u);
        }
    }
    __syncthreads();
    for (uint32_t t = threadIdx.x; t <= kBins; t += kBlock)
        if (bins[t]) atomicAdd(&hist[t], (unsigned long long)bins[t]);
}

// tile `blockIdx.x` = items [blockIdx.x * tileLen, ...): sums[tile] = its occupied slots
__global__ __launch_bounds__(kBlock) void table_count_kernel(const TableBucket* __restrict__ buckets, uint32_t nbuckets, uint32_t tileLen, uint64_t* __restrict__ sums)
{
    __shared__ uint64_t sc[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * tileLen, t1 = min(t0 + (uint64_t)tileLen, (uint64_t)nbuckets);
    uint64_t mine = 0;
    for (uint64_t b = t0 + threadIdx.x; b < t1; b += kBlock) mine += occupied(bucket_sizes(buckets, b));
    uint64_t total;
    (void)block_excl_scan(mine, sc, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void table_compact_kernel(const TableBucket* __restrict__ buckets, uint32_t nbuckets, uint32_t tileLen,
                                                               const uint64_t* __restrict__ sums, uint64_t* __restrict__ words, uint64_t cap,
                                                               unsigned int* __restrict__ flag)
{
    __shared__ uint64_t sc[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * tileLen, t1 = min(t0 + (uint64_t)tileLen, (uint64_t)nbuckets);
    uint64_t running = sums[blockIdx.x];
    for (uint64_t base = t0; base < t1; base += kBlock) {                        // (the same trips for every lane)
        const uint64_t b = base + threadIdx.x;
        const uint64_t sz = b < t1 ? bucket_sizes(buckets, b) : 0;
        uint64_t chunk;
        uint64_t at = running + block_excl_scan(occupied(sz), sc, chunk);
        running += chunk;
#pragma unroll
        for (uint32_t j = 0; j < kSlotsPerBucket; ++j) {
            const uint32_t s = (uint32_t)(sz >> (16 * j)) & 0xFFFFu;
            if (!s) continue;
            if (s >= kBins) atomicOr(flag, kFlagSize);
            if (at < cap) words[at] = ((uint64_t)buckets[b].key[j] << 16) | s;
            ++at;
        }
    }
}

// one lane per requested key: the walk of probe_finish (kernels.hip) -- found, or a bucket with a free slot, or maxProbe buckets end it
__global__ __launch_bounds__(kBlock) void table_lookup_sizes_kernel(DeviceTable tab, const uint32_t* __restrict__ keys, uint32_t m, uint32_t tileLen,
                                                                    uint32_t* __restrict__ sizes, uint64_t* __restrict__ pays, uint64_t* __restrict__ sums,
                                                                    unsigned int* __restrict__ flag)
{
    __shared__ uint64_t sc[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * tileLen, t1 = min(t0 + (uint64_t)tileLen, (uint64_t)m);
    uint64_t mine = 0;
    for (uint64_t i = t0 + threadIdx.x; i < t1; i += kBlock) {
        const uint32_t f = keys[i];
        const uint32_t home = home_group(f, tab.nbuckets);
        uint32_t cur = home, size = 0;
        uint64_t pay = 0;
        for (uint32_t step = 1;; ++step) {
            const bool anyFree = bucket_match(load_bucket(tab, cur), f, size, pay);
            if (size != 0 || anyFree || step >= tab.maxProbe) break;
            cur = next_bucket(home, cur, step, tab.nbuckets);
        }
        if (size >= kBins) { atomicOr(flag, kFlagSize); size = 0; }
        sizes[i] = size;
        pays[i] = pay;
        mine += size;
    }
    uint64_t total;
    (void)block_excl_scan(mine, sc, total);
    if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// off[i] = locations in front of list i (off[m] is tile_scan_kernel's total)
__global__ __launch_bounds__(kBlock) void table_offsets_kernel(const uint32_t* __restrict__ sizes, uint32_t m, uint32_t tileLen, const uint64_t* __restrict__ sums,
                                                               uint64_t* __restrict__ off)
{
    __shared__ uint64_t sc[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * tileLen, t1 = min(t0 + (uint64_t)tileLen, (uint64_t)m);
    uint64_t running = sums[blockIdx.x];
    for (uint64_t base = t0; base < t1; base += kBlock) {                        // (the same trips for every lane)
        const uint64_t i = base + threadIdx.x;
        uint64_t chunk;
        const uint64_t excl = block_excl_scan(i < t1 ? sizes[i] : 0u, sc, chunk);
        if (i < t1) off[i] = running + excl;
        running += chunk;
    }
}

// output locations [o0, o1) of the piece -> out[0 .. o1 - o0): list = last i with off[i] <= t (off has m + 1 entries, m >= 1)
__global__ __launch_bounds__(kBlock) void table_gather_kernel(DeviceTable tab, const uint64_t* __restrict__ off, const uint64_t* __restrict__ pays, uint32_t m,
                                                              uint64_t o0, uint64_t o1, uint64_t storeEntries, uint64_t* __restrict__ out,
                                                              unsigned int* __restrict__ flag)
{
    const uint64_t t = o0 + (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t >= o1) return;
    uint32_t lo = 0, hi = m;
    while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid] <= t) lo = mid; else hi = mid;
    }
    const uint64_t first = off[lo], size = off[lo + 1] - first, pay = pays[lo];
    uint64_t loc = pay;                                                          // size 1: the location itself, always the 8-byte form
    if (size > 1) {
        const uint64_t at = pay + (t - first);                                   // a padded list begins at its payload index and has `size` valid entries
        if (at >= storeEntries) { atomicOr(flag, kFlagStore); loc = 0; }
        else loc = tab.loc(at);
    }
    out[t - o0] = loc;
}

struct Tmp {                                  // a device allocation that lives as long as the call
    void* p = nullptr;
    ~Tmp() { if (p) (void)hipFree(p); }
    template <class T> T* as() const { return static_cast<T*>(p); }
};

int take(mc_ctx* ctx, const char* fn, Tmp& t, uint64_t bytes)
{
    if (hipMalloc(&t.p, std::max<uint64_t>(bytes, 16)) == hipSuccess) return MC_OK;
    (void)hipGetLastError();
    t.p = nullptr;
    return fail(ctx, MC_ERR_NOMEM, std::string(fn) + ": the device cannot hold " + std::to_string(bytes) + " bytes of temporaries");
}

void tiles_of(uint64_t n, uint32_t& tileLen, uint32_t& tiles)
{
    const uint64_t per = (n + kMaxTiles - 1) / kMaxTiles;
    tileLen = (uint32_t)std::max<uint64_t>(kBlock, (per + kBlock - 1) / kBlock * kBlock);
    tiles = (uint32_t)((n + tileLen - 1) / tileLen);
}

// what all three calls ask of the context, after their arguments: a device, a finished table, one part, no shard
int table_of(mc_ctx* ctx, const char* fn, DeviceTable& tab)
{
    const std::string f(fn);
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, f + ": the context has no device (mc_open_metadata)");
    if (ctx->parts.empty() || !ctx->tableReady || !ctx->parts[0].dbuckets) return fail(ctx, MC_ERR_STATE, f + ": the table is not finished (mc_load_end)");
    if (ctx->parts.size() > 1) return fail(ctx, MC_ERR_UNSUPPORTED, f + ": the context holds several parts (a list of their union is not a list of a file): open one part, mc_config.single_part");
    if (ctx->cfg.key_shard_count > 1) return fail(ctx, MC_ERR_UNSUPPORTED, f + ": the context is a key shard");
    if (ctx->cfg.target_shard_count > 1) return fail(ctx, MC_ERR_UNSUPPORTED, f + ": the context is a target-range shard");
    const Part& T = ctx->parts[0];
    tab = DeviceTable{T.dbuckets, T.dvalues, T.nbuckets, 0xFFFFFFFFu, T.maxProbe};
    if (T.compact) {
        tab.values = nullptr; tab.values32 = reinterpret_cast<const uint32_t*>(T.dvalues);
        tab.gwBase = ctx->dGwBase; tab.gwDir = ctx->dGwDir; tab.gwDirShift = ctx->gwDirShift; tab.gwGap = ctx->gwGap; tab.gwTargets = ctx->gwTargets;
    }
    return MC_OK;
}

int too_long(mc_ctx* ctx, const char* fn) { return fail(ctx, MC_ERR_UNSUPPORTED, std::string(fn) + ": the table stores a list of more than 255 locations"); }

}  // namespace

extern "C" {

int mc_table_histogram(mc_ctx* ctx, uint64_t hist[256], uint64_t* dead)
{
    static const char* fn = "mc_table_histogram";
    if (!ctx) return MC_ERR_INVALID;
    if (!hist) return fail(ctx, MC_ERR_INVALID, "mc_table_histogram: no hist");
    DeviceTable tab{};
    int rc = table_of(ctx, fn, tab);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    Tmp dHist;
    if ((rc = take(ctx, fn, dHist, (kBins + 1) * 8)) != MC_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(dHist.p, 0, (kBins + 1) * 8, st));
    {
        ScopedTimer timer(ctx, "table_hist", st);
        const uint32_t blocks = row_blocks(tab.nbuckets, kBlock, 256 * 32);
        if (blocks) hipLaunchKernelGGL(table_hist_kernel, dim3(blocks), dim3(kBlock), 0, st, tab.buckets, tab.nbuckets, dHist.as<unsigned long long>());
    }
    HIP_TRY(ctx, hipGetLastError());
    uint64_t h[kBins + 1];
    HIP_TRY(ctx, hipMemcpyAsync(h, dHist.p, sizeof h, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (h[kBins]) return too_long(ctx, fn);
    uint64_t stored = 0;
    for (uint32_t s = 0; s < kBins; ++s) { hist[s] = h[s]; stored += h[s]; }
    const uint64_t given = ctx->parts[0].keysLoaded;
    if (dead) *dead = given > stored ? given - stored : 0;
    return MC_OK;
}

int mc_table_features(mc_ctx* ctx, uint32_t* keys, uint32_t* sizes, uint64_t capacity, uint64_t* num, int flags)
{
    static const char* fn = "mc_table_features";
    if (!ctx) return MC_ERR_INVALID;
    if (!num) return fail(ctx, MC_ERR_INVALID, "mc_table_features: no num");
    if (flags != 0) return fail(ctx, MC_ERR_INVALID, "mc_table_features: flags is reserved and must be 0");
    if (capacity > 0 && (!keys || !sizes)) return fail(ctx, MC_ERR_INVALID, "mc_table_features: no keys or no sizes");
    DeviceTable tab{};
    int rc = table_of(ctx, fn, tab);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    uint32_t tileLen, tiles;
    tiles_of(tab.nbuckets, tileLen, tiles);
    Tmp dSums, dFlag;
    if ((rc = take(ctx, fn, dSums, ((uint64_t)tiles + 1) * 8)) != MC_OK || (rc = take(ctx, fn, dFlag, 4)) != MC_OK) return rc;
    uint64_t* sums = dSums.as<uint64_t>();
    HIP_TRY(ctx, hipMemsetAsync(dFlag.p, 0, 4, st));
    HIP_TRY(ctx, hipMemsetAsync(sums, 0, ((uint64_t)tiles + 1) * 8, st));
    if (tiles) {
        hipLaunchKernelGGL(table_count_kernel, dim3(tiles), dim3(kBlock), 0, st, tab.buckets, tab.nbuckets, tileLen, sums);
        hipLaunchKernelGGL(tile_scan_kernel<uint64_t>, dim3(1), dim3(kBlock), 0, st, sums, tiles, sums + tiles);
    }
    HIP_TRY(ctx, hipGetLastError());
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, sums + tiles, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    *num = total;
    const uint64_t want = std::min(capacity, total);
    if (want == 0) return MC_OK;
    // the enumeration's temporaries: the words, the sorted words, the sort's own
    size_t sortBytes = 0;
    Tmp dWords, dSorted, dSort;
    uint64_t* words = nullptr; uint64_t* sorted = nullptr;
    HIP_TRY(ctx, rocprim::radix_sort_keys(nullptr, sortBytes, words, sorted, total, 16, 48, st));
    if ((rc = take(ctx, fn, dWords, total * 8)) != MC_OK || (rc = take(ctx, fn, dSorted, total * 8)) != MC_OK || (rc = take(ctx, fn, dSort, sortBytes)) != MC_OK) return rc;
    words = dWords.as<uint64_t>(); sorted = dSorted.as<uint64_t>();
    {
        ScopedTimer timer(ctx, "table_enumerate", st);
        hipLaunchKernelGGL(table_compact_kernel, dim3(tiles), dim3(kBlock), 0, st, tab.buckets, tab.nbuckets, tileLen, sums, words, total, dFlag.as<unsigned int>());
        HIP_TRY(ctx, rocprim::radix_sort_keys(dSort.p, sortBytes, words, sorted, total, 16, 48, st));
    }
    HIP_TRY(ctx, hipGetLastError());
    unsigned int flag = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&flag, dFlag.p, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (flag & kFlagSize) return too_long(ctx, fn);
    std::vector<uint64_t> buf((size_t)std::min(want, kPieceWords));
    for (uint64_t done = 0; done < want; done += kPieceWords) {
        const uint64_t m = std::min(kPieceWords, want - done);
        HIP_TRY(ctx, hipMemcpy(buf.data(), sorted + done, m * 8, hipMemcpyDeviceToHost));
        for (uint64_t k = 0; k < m; ++k) { keys[done + k] = (uint32_t)(buf[k] >> 16); sizes[done + k] = (uint32_t)(buf[k] & 0xFFFFu); }
    }
    return MC_OK;
}

int mc_table_lookup(mc_ctx* ctx, const uint32_t* keys, uint64_t n, uint64_t* offsets, mc_location* locs, uint64_t capacity, int flags)
{
    static const char* fn = "mc_table_lookup";
    if (!ctx) return MC_ERR_INVALID;
    if (!offsets) return fail(ctx, MC_ERR_INVALID, "mc_table_lookup: no offsets");
    if (n > 0 && !keys) return fail(ctx, MC_ERR_INVALID, "mc_table_lookup: no keys");
    if (capacity > 0 && !locs) return fail(ctx, MC_ERR_INVALID, "mc_table_lookup: no locs");
    if (flags != 0) return fail(ctx, MC_ERR_INVALID, "mc_table_lookup: flags is reserved and must be 0");
    DeviceTable tab{};
    int rc = table_of(ctx, fn, tab);
    if (rc) return rc;
    offsets[0] = 0;
    if (n == 0) return MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint32_t piece = (uint32_t)std::min<uint64_t>(n, kPieceKeys);
    const bool single = piece >= n;
    Tmp dKeys, dSizes, dPays, dOff, dSums, dFlag, dOut;
    if ((rc = take(ctx, fn, dKeys, (uint64_t)piece * 4)) != MC_OK || (rc = take(ctx, fn, dSizes, (uint64_t)piece * 4)) != MC_OK ||
        (rc = take(ctx, fn, dPays, (uint64_t)piece * 8)) != MC_OK || (rc = take(ctx, fn, dOff, ((uint64_t)piece + 1) * 8)) != MC_OK ||
        (rc = take(ctx, fn, dSums, (uint64_t)kMaxTiles * 8)) != MC_OK || (rc = take(ctx, fn, dFlag, 4)) != MC_OK) return rc;
    HIP_TRY(ctx, hipMemsetAsync(dFlag.p, 0, 4, st));
    // a piece's keys -> sizes, payloads and offsets on the device (the offsets count from the piece's first list)
    auto stage = [&](uint64_t done, uint32_t m) -> int {
        uint32_t tileLen, tiles;
        tiles_of(m, tileLen, tiles);
        HIP_TRY(ctx, hipMemcpyAsync(dKeys.p, keys + done, (uint64_t)m * 4, hipMemcpyHostToDevice, st));
        ScopedTimer timer(ctx, "table_lookup", st);
        hipLaunchKernelGGL(table_lookup_sizes_kernel, dim3(tiles), dim3(kBlock), 0, st, tab, dKeys.as<uint32_t>(), m, tileLen, dSizes.as<uint32_t>(),
                           dPays.as<uint64_t>(), dSums.as<uint64_t>(), dFlag.as<unsigned int>());
        hipLaunchKernelGGL(tile_scan_kernel<uint64_t>, dim3(1), dim3(kBlock), 0, st, dSums.as<uint64_t>(), tiles, dOff.as<uint64_t>() + m);
        hipLaunchKernelGGL(table_offsets_kernel, dim3(tiles), dim3(kBlock), 0, st, dSizes.as<uint32_t>(), m, tileLen, dSums.as<uint64_t>(), dOff.as<uint64_t>());
        HIP_TRY(ctx, hipGetLastError());
        return MC_OK;
    };
    // no entry of locs may be written unless ALL lists fit, so every piece's offsets come first; a call of one piece -- the common case --
    // keeps its sizes and payloads on the device for the gather, more pieces are staged a second time
    uint64_t all = 0;
    for (uint64_t done = 0; done < n; done += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - done);
        if ((rc = stage(done, m)) != MC_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(offsets + done, dOff.p, ((uint64_t)m + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (uint64_t k = done; k <= done + m; ++k) offsets[k] += all;
        all = offsets[done + m];
    }
    unsigned int flag = 0;
    HIP_TRY(ctx, hipMemcpy(&flag, dFlag.p, 4, hipMemcpyDeviceToHost));
    if (flag & kFlagSize) return too_long(ctx, fn);
    if (all > capacity) return fail(ctx, MC_ERR_NOMEM, "mc_table_lookup: the lists hold " + std::to_string(all) + " locations, locs has room for " + std::to_string(capacity) + " (offsets is complete)");
    if (all == 0) return MC_OK;
    uint64_t maxLocs = 0;
    for (uint64_t done = 0; done < n; done += piece) maxLocs = std::max(maxLocs, offsets[std::min<uint64_t>(done + piece, n)] - offsets[done]);
    const uint64_t outPiece = std::min(maxLocs, kPieceLocs);
    if ((rc = take(ctx, fn, dOut, outPiece * 8)) != MC_OK) return rc;
    const uint64_t storeEntries = ctx->parts[0].valuesStored;
    for (uint64_t done = 0; done < n; done += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - done);
        const uint64_t first = offsets[done], total = offsets[done + m] - first;
        if (total == 0) continue;
        if (!single && (rc = stage(done, m)) != MC_OK) return rc;
        for (uint64_t o0 = 0; o0 < total; o0 += outPiece) {
            const uint64_t o1 = std::min(total, o0 + outPiece);
            {
                ScopedTimer timer(ctx, "table_gather", st);
                hipLaunchKernelGGL(table_gather_kernel, dim3((uint32_t)((o1 - o0 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, tab, dOff.as<uint64_t>(),
                                   dPays.as<uint64_t>(), m, o0, o1, storeEntries, dOut.as<uint64_t>(), dFlag.as<unsigned int>());
            }
            HIP_TRY(ctx, hipGetLastError());
            HIP_TRY(ctx, hipMemcpyAsync(locs + first + o0, dOut.p, (o1 - o0) * 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
        }
    }
    HIP_TRY(ctx, hipMemcpy(&flag, dFlag.p, 4, hipMemcpyDeviceToHost));
    if (flag & kFlagStore) return fail(ctx, MC_ERR_STATE, "mc_table_lookup: a list of the table lies outside its location store");
    return MC_OK;
}

}  // extern "C"
