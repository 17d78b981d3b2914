// metacache_amd/csrc/target_hits.hip -- mc_target_hits_*: the reference's per-target candidate lists of -hits-per-ref
// (matches_per_target::insert / sort, matches_per_target.hpp:104-136; printed by show_matches_per_targets, printing.cpp:385-420) on the
// device: every qualifying candidate becomes one 24-byte record {tgt, beg, end, hits, query} in a LOG in device memory; the log is
// sorted by (tgt, beg, end, query, hits) and cut into one slice per target when it is collected.
//
// target_hits_append_kernel: one lane per read (the shape of coverage_mark_kernel).  A lane counts its qualifying entries, the wave forms
// a prefix sum over its lanes, ONE lane reserves the wave's total with one 64-bit atomicAdd on the log's cursor, the lanes write their
// records behind each other.  Records past the capacity are not written and counted (per lane -> wave -> LDS -> one atomic per block).
// The sort (gw_sort.hip's header says why this project merges instead of running radix passes on wave64): a record is compared as three
// 64-bit words {tgt:beg, end:query.hi, query.lo:hits}, whose lexicographic order is the order of the five fields.
//   target_hits_block_sort_kernel   a block sorts one TILE of kTile records in LDS (three word planes, a bitonic network; the tile's
//                                   tail is padded with all-ones words, which no record equals or exceeds)
//   target_hits_merge_kernel        ceil(log2(tiles)) passes through HBM, ping-pong between the log and a second buffer; a block makes one
//                                   tile of the output: two lanes find where it begins and ends in the two runs (merge path, a binary
//                                   search on the tile's two diagonals in HBM), the two pieces come into LDS, every record finds its place
//                                   by a binary search in the OTHER piece (ties: the left run first), goes there in LDS, and the tile
//                                   leaves in consecutive stores.  A run without a partner is copied by the same code.
// The number of passes decides where the block sort writes, so the result always ends in the log itself.
// target_hits_bounds_kernel: one lane per target, a lower_bound over the sorted log.
// Plain HIP C++; no inline assembly.
#include "rows_common.h"
#include "devcache.h"

#include <algorithm>
#include <cstring>

namespace mcamd {

struct TargetHitsState {                 // what the context keeps on the device for mc_target_hits_*
    uint64_t linVersion = ~0ull;         // ctx->lineageVersion the records belong to
    mc_target_hit* dLog = nullptr;       // [cap]
    uint64_t cap = 0;
    unsigned long long* dCounters = nullptr;   // [2]: the cursor (records asked for, beyond cap too), records dropped
    uint64_t* dOffsets = nullptr;        // [offsetsCap]: what target_hits_bounds_kernel writes
    uint64_t offsetsCap = 0;
    std::atomic<uint64_t> addCalls{0};
    bool sorted = false;                 // the log's first sortedN records are in order (no add since the last collect)
    uint64_t sortedN = 0;
    std::mutex stageMtx;                 // MC_TARGET_HITS_HOST callers take turns at the staging buffers
    DevBuf stageIn, stageIds;
};

}  // namespace mcamd

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kMaxBlocks = 2048;
constexpr uint32_t kTile = 2048, kPerThread = kTile / kBlock;      // records a block sorts or merges at a time: 3 planes x 16 KB of LDS
constexpr uint64_t kPad = ~0ull;                                     // (a record of three such words would need tgt = beg = end = hits = 2^32 - 1 and query = 2^64 - 1 and still compares equal, not greater)
static_assert(sizeof(mc_target_hit) == 24, "mc_target_hit is three 64-bit words");
static_assert((kTile & (kTile - 1)) == 0 && kTile % (2 * kBlock) == 0, "the bitonic network takes a power of two, every thread whole pairs");

struct AppendArgs {
    const mc_candidate* cands;
    const uint64_t* queryIds;            // NULL: firstQueryId + i
    const uint32_t* lin;                 // rank-major lineage planes (classify.hip)
    mc_target_hit* log;
    unsigned long long* counters;        // [2]
    uint64_t cap, firstQueryId;
    uint32_t n, stride, linTargets, hitsMin;
    int lowest;
};

// the rule of mc_coverage_add: hits >= hits_min and a taxon (taxon_of_target)
__device__ __forceinline__ bool qualifies(const AppendArgs& a, const uint4 e)
{
    if (e.y < a.hitsMin || e.x >= a.linTargets) return false;
    int r;
    return taxon_of_target(a.lin, a.linTargets, e.x, a.lowest, r) != 0;
}

// The wave's sums of target_hits_append_kernel in their __shfl form: device_common.h's DPP forms (wave_incl_scan_u32, wave_sum_u32) need
// fewer registers here and no ds_bpermute, but the kernel has not been timed with them.
__device__ __forceinline__ uint32_t wave_incl_scan_shfl(uint32_t v, uint32_t lane)      // inclusive prefix sum over the lanes
{
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t u = (uint32_t)__shfl_up((int)v, off);
        if (lane >= (uint32_t)off) v += u;
    }
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_shfl(uint32_t v)                             // lane 0 holds the sum
{
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_down((int)v, off);
    return v;
}

__global__ __launch_bounds__(kBlock) void target_hits_append_kernel(AppendArgs a)
{
    __shared__ uint32_t blockDropped;
    if (threadIdx.x == 0) blockDropped = 0;
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t dropped = 0;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < a.n; base += step) {      // (the same trips for every lane of a block)
        const uint64_t i = base + threadIdx.x;
        const bool active = i < a.n;
        const uint4* c = reinterpret_cast<const uint4*>(a.cands + (active ? i : 0) * a.stride);   // entry j: {tgt, hits, beg, end}
        uint32_t count = 0;
        unsigned long long mask = 0;                                                      // which of the row's first 64 entries qualify
        if (active)
            for (uint32_t j = 0; j < a.stride; ++j) {
                const uint4 e = c[j];
                if (e.y == 0) break;                                                      // the list ends here
                if (!qualifies(a, e)) continue;                                           // skipped, the walk goes on
                ++count;
                if (j < 64u) mask |= 1ull << j;
            }
        // inclusive prefix sum over the wave's lanes (all 64 are here: blocks are whole waves, kBlock = 256, this loop makes the same trips
        // for every lane of a block, and the lanes that walked a row have joined the others again)
        const uint32_t incl = wave_incl_scan_shfl(count, lane);
        const uint32_t total = (uint32_t)__shfl((int)incl, 63);
        unsigned long long first = 0;
        if (lane == 63u && total != 0) first = atomicAdd(&a.counters[0], (unsigned long long)total);    // ONE atomic per wave
        first = (unsigned long long)__shfl((long long)first, 63);
        if (count != 0) {
            uint64_t at = first + (incl - count);
            const uint64_t query = a.queryIds ? a.queryIds[i] : a.firstQueryId + i;
            for (uint32_t j = 0; j < a.stride; ++j) {
                const uint4 e = c[j];
                if (e.y == 0) break;
                if (!(j < 64u ? ((mask >> j) & 1ull) != 0 : qualifies(a, e))) continue;
                if (at < a.cap) {
                    uint64_t* w = reinterpret_cast<uint64_t*>(a.log + at);                // {tgt, beg}, {end, hits}, query
                    w[0] = (uint64_t)e.x | ((uint64_t)e.z << 32);
                    w[1] = (uint64_t)e.w | ((uint64_t)e.y << 32);
                    w[2] = query;
                } else ++dropped;
                ++at;
            }
        }
    }
    // counted per wave, one atomic per block (all 64 lanes: the row loop is behind every lane of the block)
    dropped = wave_sum_shfl(dropped);
    if (lane == 0 && dropped) atomicAdd(&blockDropped, dropped);
    __syncthreads();
    if (threadIdx.x == 0 && blockDropped) atomicAdd(&a.counters[1], (unsigned long long)blockDropped);
}

// a record as the three words it is compared by
struct Key { uint64_t a, b, c; };
__device__ __forceinline__ bool key_less(const Key& x, const Key& y)
{
    if (x.a != y.a) return x.a < y.a;
    if (x.b != y.b) return x.b < y.b;
    return x.c < y.c;
}
__device__ __forceinline__ Key load_key(const mc_target_hit* p)
{
    const uint64_t* w = reinterpret_cast<const uint64_t*>(p);
    const uint64_t w0 = w[0], w1 = w[1], q = w[2];                                        // {tgt, beg}, {end, hits}, query
    Key k;
    k.a = (w0 << 32) | (w0 >> 32);                                                        // tgt : beg
    k.b = (w1 << 32) | (q >> 32);                                                         // end : query.hi
    k.c = (q << 32) | (w1 >> 32);                                                         // query.lo : hits
    return k;
}
__device__ __forceinline__ void store_key(mc_target_hit* p, const Key& k)
{
    uint64_t* w = reinterpret_cast<uint64_t*>(p);
    w[0] = (k.a >> 32) | (k.a << 32);
    w[1] = (k.b >> 32) | (k.c << 32);
    w[2] = (k.b << 32) | (k.c >> 32);
}

// tile t of in[0 .. n) sorted -> out (may be in itself: a block reads its tile before it writes it)
__global__ __launch_bounds__(kBlock) void target_hits_block_sort_kernel(const mc_target_hit* in, mc_target_hit* out, uint64_t n)
{
    __shared__ uint64_t sa[kTile], sb[kTile], sc[kTile];
    const uint64_t base = (uint64_t)blockIdx.x * kTile;
    const uint32_t len = (uint32_t)min((uint64_t)kTile, n - base);
    for (uint32_t x = threadIdx.x; x < kTile; x += kBlock) {
        Key k{kPad, kPad, kPad};
        if (x < len) k = load_key(in + base + x);
        sa[x] = k.a; sb[x] = k.b; sc[x] = k.c;
    }
    __syncthreads();
    for (uint32_t size = 2; size <= kTile; size <<= 1)
        for (uint32_t dist = size >> 1; dist > 0; dist >>= 1) {
            for (uint32_t p = threadIdx.x; p < kTile / 2; p += kBlock) {
                const uint32_t lo = ((p & ~(dist - 1u)) << 1) | (p & (dist - 1u)), hi = lo | dist;
                const bool up = (lo & size) == 0;                                         // (size == kTile: always ascending)
                const Key x{sa[lo], sb[lo], sc[lo]}, y{sa[hi], sb[hi], sc[hi]};
                if (key_less(y, x) == up && (key_less(y, x) || key_less(x, y))) {
                    sa[lo] = y.a; sb[lo] = y.b; sc[lo] = y.c;
                    sa[hi] = x.a; sb[hi] = x.b; sc[hi] = x.c;
                }
            }
            __syncthreads();
        }
    for (uint32_t x = threadIdx.x; x < len; x += kBlock) store_key(out + base + x, Key{sa[x], sb[x], sc[x]});
}

// merge path in HBM: how many of the first d outputs of merge(A, B) come from A (ties: A first); d <= la + lb
__device__ __forceinline__ uint64_t merge_path(const mc_target_hit* A, uint64_t la, const mc_target_hit* B, uint64_t lb, uint64_t d)
{
    uint64_t lo = d > lb ? d - lb : 0, hi = min(d, la);
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (!key_less(load_key(B + (d - 1 - mid)), load_key(A + mid))) lo = mid + 1; else hi = mid;   // A[mid] <= B[d - 1 - mid]
    }
    return lo;
}

// one pass: the sorted runs of `run` records of in[0 .. n) are merged pairwise into out; block t makes out[t * kTile ..)
__global__ __launch_bounds__(kBlock) void target_hits_merge_kernel(const mc_target_hit* __restrict__ in, mc_target_hit* __restrict__ out, uint64_t n, uint64_t run)
{
    __shared__ uint64_t sa[kTile], sb[kTile], sc[kTile];
    __shared__ uint64_t cut[2];
    const uint64_t o0 = (uint64_t)blockIdx.x * kTile;                                     // (< n by the grid's size)
    const uint64_t pairBase = o0 / (2 * run) * (2 * run);
    const uint64_t la = min(run, n - pairBase), lb = min(run, n - pairBase - la);
    const mc_target_hit* A = in + pairBase;
    const mc_target_hit* B = A + la;
    const uint64_t d0 = o0 - pairBase, d1 = min(d0 + kTile, la + lb);
    if (threadIdx.x < 2) cut[threadIdx.x] = merge_path(A, la, B, lb, threadIdx.x ? d1 : d0);
    __syncthreads();
    const uint64_t a0 = cut[0], a1 = cut[1], b0 = d0 - a0, b1 = d1 - a1;
    const uint32_t na = (uint32_t)(a1 - a0), nb = (uint32_t)(b1 - b0), len = na + nb;   // (len <= kTile)
    for (uint32_t x = threadIdx.x; x < len; x += kBlock) {
        const Key k = load_key(x < na ? A + a0 + x : B + b0 + (x - na));
        sa[x] = k.a; sb[x] = k.b; sc[x] = k.c;
    }
    __syncthreads();
    // every record's place in the merged tile: its own index in its piece + the records of the other piece that go before it
    Key mine[kPerThread];
    uint32_t place[kPerThread];
#pragma unroll
    for (uint32_t u = 0; u < kPerThread; ++u) {
        const uint32_t x = threadIdx.x + u * kBlock;
        place[u] = kTile;
        if (x < len) {
            const Key k{sa[x], sb[x], sc[x]};
            mine[u] = k;
            const bool fromA = x < na;
            uint32_t lo = fromA ? na : 0u, hi = fromA ? len : na;                         // the other piece
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                const Key m{sa[mid], sb[mid], sc[mid]};
                // from A: the B records LESS than k go first; from B: the A records less than OR EQUAL to k
                const bool before = fromA ? key_less(m, k) : !key_less(k, m);
                if (before) lo = mid + 1; else hi = mid;
            }
            place[u] = fromA ? x + (lo - na) : (x - na) + lo;
        }
    }
    __syncthreads();
#pragma unroll
    for (uint32_t u = 0; u < kPerThread; ++u)
        if (place[u] < kTile) { sa[place[u]] = mine[u].a; sb[place[u]] = mine[u].b; sc[place[u]] = mine[u].c; }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < len; x += kBlock) store_key(out + o0 + x, Key{sa[x], sb[x], sc[x]});
}

// offsets[t] = the first record of the sorted log with tgt >= t, for t = 0 .. targets (offsets[targets] = n where no record's tgt is beyond the table)
__global__ __launch_bounds__(kBlock) void target_hits_bounds_kernel(const mc_target_hit* __restrict__ log, uint64_t n, uint32_t targets, uint64_t* __restrict__ offsets)
{
    const uint64_t t = (uint64_t)blockIdx.x * kBlock + threadIdx.x;
    if (t > targets) return;
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)log[mid].tgt < t) lo = mid + 1; else hi = mid;
    }
    offsets[t] = lo;
}

void free_device(TargetHitsState& S)
{
    if (S.dLog) (void)hipFree(S.dLog);
    S.dLog = nullptr; S.cap = 0; S.sorted = false; S.sortedN = 0;
}

// the state object, its two counters, and -- after mc_set_lineages -- an empty log
int ensure_state(mc_ctx* ctx, const char* who, TargetHitsState** out)
{
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, std::string(who) + ": the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::lock_guard<std::mutex> lock(ctx->targetHitsMtx);
    if (!ctx->targetHits) ctx->targetHits = new TargetHitsState;
    TargetHitsState& S = *ctx->targetHits;
    *out = &S;
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, kCounterPairBytes));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, kCounterPairBytes));
        S.linVersion = ctx->lineageVersion;
    }
    if (S.linVersion != ctx->lineageVersion) {                                            // other lineages: what was recorded under the old ones goes
        HIP_TRY(ctx, hipDeviceSynchronize());
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, kCounterPairBytes));
        S.addCalls = 0; S.sorted = false; S.sortedN = 0;
        S.linVersion = ctx->lineageVersion;
    }
    return MC_OK;
}

// the log with room for newCap records, the first `keep` of the old one in it; MC_ERR_NOMEM leaves everything as it was.  Under ctx->targetHitsMtx.
int resize_log(mc_ctx* ctx, TargetHitsState& S, uint64_t newCap, uint64_t keep)
{
    if (newCap == S.cap) return MC_OK;
    mc_target_hit* fresh = nullptr;
    if (newCap) {
        if (dev_malloc((void**)&fresh, newCap * sizeof(mc_target_hit)) != hipSuccess) {
            (void)hipGetLastError();
            return fail(ctx, MC_ERR_NOMEM, "mc_target_hits: the device has no room for a log of " + std::to_string(newCap) + " records");
        }
        if (keep) {
            const hipError_t e = hipMemcpy(fresh, S.dLog, keep * sizeof(mc_target_hit), hipMemcpyDeviceToDevice);
            if (e != hipSuccess) { (void)hipFree(fresh); return fail(ctx, MC_ERR_HIP, std::string("mc_target_hits: copy into the larger log: ") + hipGetErrorString(e)); }
        }
    }
    if (S.dLog) (void)hipFree(S.dLog);
    S.dLog = fresh; S.cap = newCap;
    return MC_OK;
}

void launch_append(const TargetHitsState& S, const ClassifyState& C, const mc_candidate* cands, const uint64_t* ids, uint64_t firstId, uint32_t n, uint32_t stride,
                   uint32_t hitsMin, int lowest, hipStream_t st)
{
    AppendArgs a{};
    a.cands = cands; a.queryIds = ids; a.lin = C.dLin; a.log = S.dLog; a.counters = S.dCounters; a.cap = S.cap; a.firstQueryId = firstId;
    a.n = n; a.stride = stride; a.linTargets = C.numTargets; a.hitsMin = hitsMin; a.lowest = lowest;
    hipLaunchKernelGGL(target_hits_append_kernel, dim3(row_blocks(n, kBlock, kMaxBlocks)), dim3(kBlock), 0, st, a);
}

// the log's first n records in order, in the log itself; `tmp` has room for n records
void launch_sort(mc_target_hit* log, mc_target_hit* tmp, uint64_t n, hipStream_t st)
{
    const uint64_t tiles = (n + kTile - 1) / kTile;
    uint32_t passes = 0;
    for (uint64_t runs = tiles; runs > 1; runs = (runs + 1) / 2) ++passes;
    mc_target_hit* src = (passes & 1u) ? tmp : log;                                       // an odd number of passes ends in the log when it begins in tmp
    hipLaunchKernelGGL(target_hits_block_sort_kernel, dim3((uint32_t)tiles), dim3(kBlock), 0, st, log, src, n);
    uint64_t run = kTile;
    for (uint32_t p = 0; p < passes; ++p, run *= 2) {
        mc_target_hit* dst = src == log ? tmp : log;
        hipLaunchKernelGGL(target_hits_merge_kernel, dim3((uint32_t)tiles), dim3(kBlock), 0, st, src, dst, n, run);
        src = dst;
    }
}

}  // namespace

extern "C" const uint32_t mc_target_hits_tile = kTile;

namespace mcamd {

void free_target_hits_state(mc_ctx* ctx)
{
    if (!ctx->targetHits) return;
    TargetHitsState& S = *ctx->targetHits;
    free_device(S);
    for (void* p : {(void*)S.dCounters, (void*)S.dOffsets, S.stageIn.p, S.stageIds.p}) if (p) (void)hipFree(p);
    delete ctx->targetHits;
    ctx->targetHits = nullptr;
}

}  // namespace mcamd

extern "C" {

int mc_target_hits_reserve(mc_ctx* ctx, uint64_t capacity)
{
    if (!ctx) return MC_ERR_INVALID;
    if (capacity > (1ull << 40)) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_reserve: more than 2^40 records");
    TargetHitsState* S = nullptr;
    const int rc = ensure_state(ctx, "mc_target_hits_reserve", &S);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(ctx->targetHitsMtx);
    HIP_TRY(ctx, hipDeviceSynchronize());                                                 // (appends that still run finish on the old log)
    unsigned long long counters[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(counters, S->dCounters, sizeof counters, hipMemcpyDeviceToHost));
    const uint64_t stored = std::min<uint64_t>(counters[0], S->cap);
    if (capacity == 0) {
        free_device(*S);
        HIP_TRY(ctx, hipMemset(S->dCounters, 0, kCounterPairBytes));
        S->addCalls = 0;
        return MC_OK;
    }
    if (capacity < stored) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_reserve: the log holds " + std::to_string(stored) + " records (collect with reset, or reserve 0, first)");
    return resize_log(ctx, *S, capacity, stored);
}

int mc_target_hits_add(mc_ctx* ctx, const mc_candidate* cands, const uint64_t* queryIds, uint64_t firstQueryId, uint32_t n, uint32_t stride, uint32_t hitsMin,
                       int32_t lowest, int flags, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_TARGET_HITS_HOST) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_add: unknown flag");
    if (stride == 0) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_add: stride must be at least 1");
    if (lowest < 0 || lowest >= MC_NUM_RANKS) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_add: lowest_rank must be 0 .. MC_NUM_RANKS - 1");
    if (n > 0 && !cands) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_add: null array");
    const bool host = (flags & MC_TARGET_HITS_HOST) != 0;
    if (n > 0 && !host && (((uintptr_t)cands & 15u) || ((uintptr_t)queryIds & 7u))) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_add: device arrays must be 16-byte (cands) and 8-byte (query_ids) aligned");
    if (n == 0) return MC_OK;
    // ... then state
    if (ctx->lineages.empty()) return fail(ctx, MC_ERR_STATE, "mc_target_hits_add: the context has no lineages (mc_set_lineages)");
    TargetHitsState* S = nullptr; ClassifyState* Cl = nullptr;
    int rc = ensure_state(ctx, "mc_target_hits_add", &S);
    if (rc) return rc;
    if ((rc = ensure_classify_state(ctx, &Cl)) != MC_OK) return rc;
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (!host) {
        std::lock_guard<std::mutex> state(ctx->targetHitsMtx);                            // (the log is not replaced between the read of its pointer and the launch)
        if (!S->dLog) return fail(ctx, MC_ERR_STATE, "mc_target_hits_add: no log (mc_target_hits_reserve)");
        S->sorted = false;
        ++S->addCalls;
        launch_append(*S, *Cl, cands, queryIds, firstQueryId, n, stride, hitsMin, lowest, st);
        HIP_TRY(ctx, hipGetLastError());
        return MC_OK;
    }
    // host arrays: room for every entry first (all or nothing), then in pieces of at most 64 MB of candidates through the staging buffers
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint32_t piece = staged_piece_rows(n, stride);
    if ((rc = grow(ctx, S->stageIn, staged_piece_bytes(n, stride))) != MC_OK) return rc;      // (here already: both buffers before the log is touched)
    if (queryIds && (rc = grow(ctx, S->stageIds, (uint64_t)piece * 8)) != MC_OK) return rc;
    {
        std::lock_guard<std::mutex> state(ctx->targetHitsMtx);
        HIP_TRY(ctx, hipStreamSynchronize(st));
        unsigned long long counters[2] = {0, 0};
        HIP_TRY(ctx, hipMemcpy(counters, S->dCounters, sizeof counters, hipMemcpyDeviceToHost));
        if (counters[0] > S->cap) return fail(ctx, MC_ERR_STATE, "mc_target_hits_add: the log has dropped records (mc_target_hits_collect with reset first)");
        const uint64_t need = counters[0] + (uint64_t)n * stride;
        if (need > S->cap) {
            const uint64_t most = (uint64_t)ctx->targetHitsMaxMb * (1ull << 20) / sizeof(mc_target_hit);
            if (need > most)
                return fail(ctx, MC_ERR_NOMEM, "mc_target_hits_add: " + std::to_string(need) + " records are more than target_hits_max_mb = " + std::to_string(ctx->targetHitsMaxMb) + " holds");
            HIP_TRY(ctx, hipDeviceSynchronize());
            if ((rc = resize_log(ctx, *S, std::min(most, std::max<uint64_t>({need, 2 * S->cap, 65536})), counters[0])) != MC_OK) return rc;
        }
        S->sorted = false;
        ++S->addCalls;
    }
    return for_each_staged_piece(ctx, st, S->stageIn, cands, n, stride, [&](const mc_candidate* dRows, uint32_t done, uint32_t m) {
        if (queryIds) HIP_TRY(ctx, hipMemcpyAsync(S->stageIds.p, queryIds + done, (uint64_t)m * 8, hipMemcpyHostToDevice, st));
        std::lock_guard<std::mutex> state(ctx->targetHitsMtx);
        launch_append(*S, *Cl, dRows, queryIds ? (const uint64_t*)S->stageIds.p : nullptr, firstQueryId + done, m, stride, hitsMin, lowest, st);
        HIP_TRY(ctx, hipGetLastError());
        return (int)MC_OK;
    });
}

int mc_target_hits_collect(mc_ctx* ctx, uint64_t* offsets, uint64_t capacityTargets, uint64_t* numTargets, mc_target_hit* records, uint64_t capacityRecords,
                           uint64_t* numRecords, uint64_t stats[4], int reset)
{
    if (!ctx) return MC_ERR_INVALID;
    if (ctx->lineages.empty()) return fail(ctx, MC_ERR_STATE, "mc_target_hits_collect: the context has no lineages (mc_set_lineages)");
    TargetHitsState* S = nullptr; ClassifyState* Cl = nullptr;
    int rc = ensure_state(ctx, "mc_target_hits_collect", &S);
    if (rc) return rc;
    if ((rc = ensure_classify_state(ctx, &Cl)) != MC_OK) return rc;
    std::lock_guard<std::mutex> lock(ctx->targetHitsMtx);
    hipStream_t st = ctx->stream;
    if ((rc = drain_query_streams(ctx)) != MC_OK) return rc;
    unsigned long long counters[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpy(counters, S->dCounters, sizeof counters, hipMemcpyDeviceToHost));
    const uint64_t n = std::min<uint64_t>(counters[0], S->cap), nt = Cl->numTargets;
    // the order is needed by whoever asks for the lists or for stats[3]; a call without either (a reset, a count) leaves the log as it is
    std::vector<uint64_t> off;
    if (offsets || records || stats) {
        if (S->offsetsCap < nt + 1) {
            if (S->dOffsets) { (void)hipFree(S->dOffsets); S->dOffsets = nullptr; S->offsetsCap = 0; }
            HIP_TRY(ctx, hipMalloc((void**)&S->dOffsets, (nt + 1) * 8));
            S->offsetsCap = nt + 1;
        }
        if (n > 1 && !(S->sorted && S->sortedN == n)) {
            mc_target_hit* tmp = nullptr;                                                     // the passes' second buffer: from the block cache, back to it
            if (n > kTile && big_malloc((void**)&tmp, n * sizeof(mc_target_hit)) != hipSuccess) {
                (void)hipGetLastError();
                return fail(ctx, MC_ERR_NOMEM, "mc_target_hits_collect: the device has no room for the sort's second buffer (" + std::to_string(n) + " records)");
            }
            { ScopedTimer t(ctx, "target_hits_sort", st); launch_sort(S->dLog, tmp, n, st); }
            const hipError_t e = hipGetLastError();
            const hipError_t e2 = hipStreamSynchronize(st);
            if (tmp) (void)big_free(tmp);
            HIP_TRY(ctx, e);
            HIP_TRY(ctx, e2);
        }
        S->sorted = true; S->sortedN = n;
        { ScopedTimer t(ctx, "target_hits_bounds", st); hipLaunchKernelGGL(target_hits_bounds_kernel, dim3((uint32_t)((nt + 1 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, S->dLog, n, (uint32_t)nt, S->dOffsets); }
        HIP_TRY(ctx, hipGetLastError());
        off.resize(nt + 1);
        HIP_TRY(ctx, hipMemcpyAsync(off.data(), S->dOffsets, (nt + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    if (numTargets) *numTargets = nt;
    if (numRecords) *numRecords = n;
    if (stats) {
        uint64_t filled = 0;
        for (uint64_t t = 0; t < nt; ++t) filled += off[t + 1] > off[t];
        stats[0] = n; stats[1] = counters[1]; stats[2] = S->addCalls; stats[3] = filled;
    }
    if (offsets || records) {
        if (counters[1] > 0) return fail(ctx, MC_ERR_STATE, "mc_target_hits_collect: " + std::to_string(counters[1]) + " records found no room in the log: the lists are not whole");
        if (offsets && capacityTargets < nt) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_collect: capacity_targets is smaller than the number of targets");
        if (records && capacityRecords < n) return fail(ctx, MC_ERR_INVALID, "mc_target_hits_collect: capacity_records is smaller than the number of records");
        if (offsets) std::memcpy(offsets, off.data(), (nt + 1) * 8);
        if (records && n) HIP_TRY(ctx, hipMemcpy(records, S->dLog, n * sizeof(mc_target_hit), hipMemcpyDeviceToHost));
    }
    if (reset) {
        HIP_TRY(ctx, hipMemset(S->dCounters, 0, kCounterPairBytes));
        S->addCalls = 0; S->sorted = false; S->sortedN = 0;
    }
    return MC_OK;
}

}  // extern "C"
