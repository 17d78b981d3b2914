// metacache_amd/csrc/coverage.hip -- mc_coverage_*: the reference's two-pass classification of -cov-percentile (classification.cpp:591-634,
// :660-671, :747-838; matches_per_target.hpp:100-127) on the device: which windows of which targets the reads' qualifying candidates
// cover, the targets' covered-window counts, and the candidate lists without the targets that were dropped.
//
// ONE BITMAP for all targets.  Target t owns the words wordBase[t] .. wordBase[t] + ceil(windows(t) / 32), bit w & 31 of word w >> 5 is
// its window w; no two targets share a word, bits past windows(t) are never set.  A collection's windows number fewer than 2^32: the
// bitmap of the 150 Gbp table takes 168 MB.
// coverage_mark_kernel: one lane per read (the shape of taxon_vote_kernel); a lane walks its row, one 16-byte load per entry, and ORs a
// mask into every word its range touches.  coverage_count_kernel: one wave per target, popcounts.  coverage_drop_kernel: one lane per
// read, the entries of kept targets move to the front of the row.
// Plain HIP C++; no inline assembly.
#include "rows_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <numeric>

namespace mcamd {

struct CoverageState {                   // what the context keeps on the device for mc_coverage_*
    uint64_t winVersion = ~0ull;         // ctx->windowsVersion the layout was made from
    uint64_t linVersion = ~0ull;         // ctx->lineageVersion the marks belong to
    std::vector<uint32_t> hWordBase;     // [targets + 1]: first word of every target, the total at the end
    uint32_t* dWordBase = nullptr;       // [targets + 1]
    uint32_t* dWindows = nullptr;        // [targets]
    uint32_t* dCovered = nullptr;        // [targets]: what coverage_count_kernel writes
    uint32_t* dBits = nullptr;           // [words]
    uint64_t words = 0;
    uint32_t numTargets = 0;
    unsigned long long* dCounters = nullptr;   // [2]: qualifying entries that marked windows, entries out of range
    std::atomic<uint64_t> addCalls{0};
    uint8_t* dKeep = nullptr;            // [keepTargets], absent until mc_coverage_set_keep
    uint64_t keepTargets = 0;
    std::mutex stageMtx;                 // MC_COVERAGE_HOST callers take turns at the staging buffers
    DevBuf stageIn;
};

}  // namespace mcamd

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kMaxBlocks = 2048, kWavesPerBlock = kBlock / 64;

struct MarkArgs {
    const mc_candidate* cands;
    const uint32_t* lin;                 // rank-major lineage planes (classify.hip)
    const uint32_t* wordBase;
    const uint32_t* windows;
    uint32_t* bits;
    unsigned long long* counters;        // [2]
    uint32_t n, stride, linTargets, targets, hitsMin;
    int lowest;
};

// TEST: the word is LOADED first and the atomic is issued only where it would set a bit.  The reads of a sample pile onto a few genomes,
// so after the first moments almost every bit a candidate wants is set already and the kernel is the vote's loads plus one word.
// The load is a plain one and may be served from this XCD's L2 with a line that another XCD's atomics have changed since: bits are only
// ever SET between two resets, so a stale word can only lack bits that are there by now -- it costs an atomic that was not needed, never
// a bit that is missing.  (A reset is a memset on a stream that the caller has ordered against the marking calls; kernels see it.)
template <bool TEST>
__global__ __launch_bounds__(kBlock) void coverage_mark_kernel(MarkArgs a)
{
    __shared__ uint32_t blockCount[2];
    if (threadIdx.x < 2) blockCount[threadIdx.x] = 0;
    __syncthreads();
    uint32_t marked = 0, outside = 0;
    const uint32_t nL = a.linTargets;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < a.n; i += step) {
        const uint4* c = reinterpret_cast<const uint4*>(a.cands + i * a.stride);          // entry j: {tgt, hits, beg, end}
        for (uint32_t j = 0; j < a.stride; ++j) {
            const uint4 e = c[j];
            if (e.y == 0) break;                                                          // the list ends here: every producer of rows (the candidate kernels, mc_coverage_drop,
                                                                                          // mcq's padded rows) puts its empty entries behind the filled ones
            // matches_per_target::insert: an entry that does not qualify is skipped, the walk goes on
            if (e.y < a.hitsMin || e.x >= nL) continue;
            // the target's size and first word are asked for together with its taxon, ahead of the tests that use them: the chain
            // entry -> tables -> word is three memory latencies deep, not five
            const bool known = e.x < a.targets;
            const uint32_t W = known ? a.windows[e.x] : 0u, base = known ? a.wordBase[e.x] : 0u;
            int r;
            if (!taxon_of_target(a.lin, nL, e.x, a.lowest, r)) continue;
            if (!known || e.z > e.w) { ++outside; continue; }
            if (e.z >= W) { ++outside; continue; }
            uint32_t end = e.w;
            if (end >= W) { end = W - 1; ++outside; }                                     // the part inside the target is marked
            ++marked;
            uint32_t* words = a.bits + base;
            const uint32_t w0 = e.z >> 5, w1 = end >> 5;
            for (uint32_t w = w0; w <= w1; ++w) {
                uint32_t mask = 0xFFFFFFFFu;
                if (w == w0) mask &= 0xFFFFFFFFu << (e.z & 31u);
                if (w == w1) mask &= 0xFFFFFFFFu >> (31u - (end & 31u));
                if (TEST && (words[w] & mask) == mask) continue;
                atomicOr(words + w, mask);                                                // (result unused: no value comes back)
            }
        }
    }
    // counted per wave, one atomic per block and counter.  wave_sum_u32 needs all 64 lanes: blocks are whole waves (kBlock = 256) and the
    // lanes, whatever number of rows each has walked, have left the row loop together by here
    marked = wave_sum_u32(marked); outside = wave_sum_u32(outside);
    if ((threadIdx.x & 63u) == 0) {
        if (marked) atomicAdd(&blockCount[0], marked);
        if (outside) atomicAdd(&blockCount[1], outside);
    }
    __syncthreads();
    if (threadIdx.x < 2 && blockCount[threadIdx.x]) atomicAdd(&a.counters[threadIdx.x], (unsigned long long)blockCount[threadIdx.x]);
}

// covered[t] = bits set in target t's words: one wave per target, its lanes stride over the words
__global__ __launch_bounds__(kBlock) void coverage_count_kernel(const uint32_t* __restrict__ bits, const uint32_t* __restrict__ wordBase, uint32_t targets,
                                                                uint32_t* __restrict__ covered)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t t = (uint64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (t >= targets) return;                                                             // (the same for every lane of a wave)
    const uint32_t b = wordBase[t], e = wordBase[t + 1];
    uint32_t sum = 0;
    for (uint32_t w = b + lane; w < e; w += 64) sum += (uint32_t)__popc(bits[w]);
    sum = wave_sum_u32(sum);                                                              // all 64 lanes: a wave has left above as a whole or is here as a whole, the word loop behind it
    if (lane == 0) covered[t] = sum;
}

// update_candidates (classification.cpp:660-671): the entries of kept targets, in their order, at the front of the row; zeros behind them.
// out may be the input itself: a lane owns its row and writes entry k <= j after it has read entry j.
__global__ __launch_bounds__(kBlock) void coverage_drop_kernel(const mc_candidate* in, mc_candidate* out, uint32_t n, uint32_t stride,
                                                               const uint8_t* __restrict__ keep, uint64_t keepTargets)
{
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += step) {
        const uint4* src = reinterpret_cast<const uint4*>(in + i * stride);
        uint4* dst = reinterpret_cast<uint4*>(out + i * stride);
        uint32_t k = 0;
        for (uint32_t j = 0; j < stride; ++j) {
            const uint4 e = src[j];
            if (e.y == 0) break;
            if (e.x < keepTargets && keep[e.x]) dst[k++] = e;
        }
        for (; k < stride; ++k) dst[k] = make_uint4(0, 0, 0, 0);
    }
}

void free_device(CoverageState& S)
{
    for (void* p : {(void*)S.dWordBase, (void*)S.dWindows, (void*)S.dCovered, (void*)S.dBits, (void*)S.dCounters, (void*)S.dKeep})
        if (p) (void)hipFree(p);
    S.dWordBase = S.dWindows = S.dCovered = S.dBits = nullptr; S.dCounters = nullptr; S.dKeep = nullptr;
    S.keepTargets = 0; S.words = 0; S.numTargets = 0;
}

// the layout for the announced window counts: made on first use, made again -- empty, and without a keep mask -- when other window counts
// or other lineages have been announced.  Returns the lineage planes of classify.hip with it (one copy of the table on the device).
int ensure_state(mc_ctx* ctx, const char* who, CoverageState** out, ClassifyState** cls)
{
    if (ctx->targetWindows.empty()) return fail(ctx, MC_ERR_STATE, std::string(who) + ": the context has no window counts (mc_load_target_windows)");
    if (ctx->lineages.empty()) return fail(ctx, MC_ERR_STATE, std::string(who) + ": the context has no lineages (mc_set_lineages)");
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, std::string(who) + ": the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int rc = ensure_classify_state(ctx, cls);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(ctx->coverageMtx);
    if (!ctx->coverage) ctx->coverage = new CoverageState;
    CoverageState& S = *ctx->coverage;
    *out = &S;
    if (S.winVersion == ctx->windowsVersion && S.linVersion == ctx->lineageVersion && S.dBits) return MC_OK;
    if (S.dBits) HIP_TRY(ctx, hipDeviceSynchronize());                                    // (marks that still run finish on the old layout)
    if (S.winVersion != ctx->windowsVersion || !S.dBits) {
        free_device(S);
        const uint64_t nt = ctx->targetWindows.size();
        S.hWordBase.assign(nt + 1, 0);
        uint64_t words = 0;
        for (uint64_t t = 0; t < nt; ++t) { S.hWordBase[t] = (uint32_t)words; words += ((uint64_t)ctx->targetWindows[t] + 31) / 32; }
        if (words >= 0xFFFFFF00ull) return fail(ctx, MC_ERR_UNSUPPORTED, std::string(who) + ": the bitmap would take 2^32 words");
        S.hWordBase[nt] = (uint32_t)words;
        S.words = words; S.numTargets = (uint32_t)nt;
        HIP_TRY(ctx, hipMalloc((void**)&S.dWordBase, (nt + 1) * 4));
        HIP_TRY(ctx, hipMalloc((void**)&S.dWindows, nt * 4));
        HIP_TRY(ctx, hipMalloc((void**)&S.dCovered, nt * 4));
        HIP_TRY(ctx, hipMalloc((void**)&S.dBits, std::max<uint64_t>(words, 1) * 4));
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, kCounterPairBytes));
        HIP_TRY(ctx, hipMemcpy(S.dWordBase, S.hWordBase.data(), (nt + 1) * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(S.dWindows, ctx->targetWindows.data(), nt * 4, hipMemcpyHostToDevice));
    }
    if (S.dKeep) { (void)hipFree(S.dKeep); S.dKeep = nullptr; S.keepTargets = 0; }
    HIP_TRY(ctx, hipMemsetAsync(S.dBits, 0, std::max<uint64_t>(S.words, 1) * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(S.dCounters, 0, kCounterPairBytes, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    S.addCalls = 0;
    S.winVersion = ctx->windowsVersion; S.linVersion = ctx->lineageVersion;
    return MC_OK;
}

// test: the load before the atomic (the shipped form; mc_set_tuning "coverage_load_first" 0 sends every mask out as an atomic, for measurements)
void launch_mark(const CoverageState& S, const ClassifyState& C, const mc_candidate* cands, uint32_t n, uint32_t stride, uint32_t hitsMin, int lowest,
                 bool test, hipStream_t st)
{
    MarkArgs a{};
    a.cands = cands; a.lin = C.dLin; a.wordBase = S.dWordBase; a.windows = S.dWindows; a.bits = S.dBits; a.counters = S.dCounters;
    a.n = n; a.stride = stride; a.linTargets = C.numTargets; a.targets = S.numTargets; a.hitsMin = hitsMin; a.lowest = lowest;
    if (test) hipLaunchKernelGGL(coverage_mark_kernel<true>, dim3(row_blocks(n, kBlock, kMaxBlocks)), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(coverage_mark_kernel<false>, dim3(row_blocks(n, kBlock, kMaxBlocks)), dim3(kBlock), 0, st, a);
}

}  // namespace

namespace mcamd {

void free_coverage_state(mc_ctx* ctx)
{
    if (!ctx->coverage) return;
    CoverageState& S = *ctx->coverage;
    free_device(S);
    if (S.stageIn.p) (void)hipFree(S.stageIn.p);
    delete ctx->coverage;
    ctx->coverage = nullptr;
}

}  // namespace mcamd

extern "C" {

int mc_coverage_add(mc_ctx* ctx, const mc_candidate* cands, uint32_t n, uint32_t stride, uint32_t hitsMin, int32_t lowest, int flags, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_COVERAGE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_coverage_add: unknown flag");
    if (stride == 0) return fail(ctx, MC_ERR_INVALID, "mc_coverage_add: stride must be at least 1");
    if (lowest < 0 || lowest >= MC_NUM_RANKS) return fail(ctx, MC_ERR_INVALID, "mc_coverage_add: lowest_rank must be 0 .. MC_NUM_RANKS - 1");
    if (n > 0 && !cands) return fail(ctx, MC_ERR_INVALID, "mc_coverage_add: null array");
    if (n > 0 && !(flags & MC_COVERAGE_HOST) && ((uintptr_t)cands & 15u)) return fail(ctx, MC_ERR_INVALID, "mc_coverage_add: device arrays must be 16-byte aligned");
    if (n == 0) return MC_OK;
    // ... then state
    CoverageState* S = nullptr; ClassifyState* Cl = nullptr;
    int rc = ensure_state(ctx, "mc_coverage_add", &S, &Cl);
    if (rc) return rc;
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const bool test = ctx->coverageLoadFirst;
    ++S->addCalls;
    if (!(flags & MC_COVERAGE_HOST)) {
        std::lock_guard<std::mutex> state(ctx->coverageMtx);                              // (the bitmap is not laid out again between the read of its pointers and the launch)
        launch_mark(*S, *Cl, cands, n, stride, hitsMin, lowest, test, st);
        HIP_TRY(ctx, hipGetLastError());
        return MC_OK;
    }
    // host arrays: in pieces of at most 64 MB of candidates through the staging buffer, one caller at a time
    std::lock_guard<std::mutex> lock(S->stageMtx);
    return for_each_staged_piece(ctx, st, S->stageIn, cands, n, stride, [&](const mc_candidate* dRows, uint32_t, uint32_t m) {
        std::lock_guard<std::mutex> state(ctx->coverageMtx);
        launch_mark(*S, *Cl, dRows, m, stride, hitsMin, lowest, test, st);
        HIP_TRY(ctx, hipGetLastError());
        return (int)MC_OK;
    });
}

int mc_coverage_counts(mc_ctx* ctx, uint32_t* covered, uint32_t* windows, uint64_t capacity, uint64_t* numTargets, uint64_t stats[4], int reset)
{
    if (!ctx) return MC_ERR_INVALID;
    CoverageState* S = nullptr; ClassifyState* Cl = nullptr;
    const int rc = ensure_state(ctx, "mc_coverage_counts", &S, &Cl);
    if (rc) return rc;
    if (const int drc = drain_query_streams(ctx)) return drc;
    const uint32_t nt = S->numTargets;
    {
        ScopedTimer t(ctx, "coverage_count_kernel", ctx->stream);                         // mc_timing_enable: "coverage_count_kernel" in mc_timing_get
        hipLaunchKernelGGL(coverage_count_kernel, dim3((nt + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, ctx->stream, S->dBits, S->dWordBase, nt, S->dCovered);
    }
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint32_t> all(nt);
    unsigned long long counters[2] = {0, 0};
    HIP_TRY(ctx, hipMemcpyAsync(all.data(), S->dCovered, (uint64_t)nt * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(counters, S->dCounters, sizeof counters, hipMemcpyDeviceToHost, ctx->stream));
    if (reset) {
        HIP_TRY(ctx, hipMemsetAsync(S->dBits, 0, std::max<uint64_t>(S->words, 1) * 4, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(S->dCounters, 0, kCounterPairBytes, ctx->stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint64_t take = std::min<uint64_t>(capacity, nt);
    if (covered && take) std::memcpy(covered, all.data(), take * 4);
    if (windows && take) std::memcpy(windows, ctx->targetWindows.data(), take * 4);
    if (numTargets) *numTargets = nt;
    if (stats) {
        stats[0] = counters[0]; stats[1] = counters[1];
        stats[2] = std::accumulate(all.begin(), all.end(), (uint64_t)0);
        stats[3] = S->addCalls;
    }
    if (reset) S->addCalls = 0;
    return MC_OK;
}

int mc_coverage_keep(const uint32_t* covered, const uint32_t* windows, uint64_t numTargets, const uint32_t* order, uint64_t numOrder, float percentile,
                     uint8_t* keep)
{
    if (!std::isfinite(percentile) || percentile < 0.0f || percentile > 1.0f) return MC_ERR_INVALID;
    if (numTargets > 0 && (!covered || !windows || !keep)) return MC_ERR_INVALID;
    if (!order && numOrder) return MC_ERR_INVALID;
    const uint64_t visits = order ? numOrder : numTargets;
    std::vector<uint8_t> seen(numTargets, 0);
    for (uint64_t i = 0; order && i < visits; ++i) {
        if (order[i] >= numTargets || seen[order[i]]) return MC_ERR_INVALID;
        seen[order[i]] = 1;
    }
    // filter_targets_by_coverage, classification.cpp:591-634
    using CovP = std::pair<uint32_t, float>;
    std::vector<CovP> cov;
    float sum = 0;
    for (uint64_t i = 0; i < visits; ++i) {
        const uint32_t t = order ? order[i] : (uint32_t)i;
        if (covered[t] == 0) continue;
        const float covP = (float)covered[t] / (float)windows[t];
        sum += covP;
        cov.emplace_back(t, covP);
    }
    std::stable_sort(cov.begin(), cov.end(), [](const CovP& a, const CovP& b) { return a.second < b.second; });
    if (numTargets) std::memset(keep, 0, numTargets);
    for (const CovP& c : cov) keep[c.first] = 1;
    const float limit = percentile * sum;
    float part = 0;
    for (const CovP& c : cov) {
        part += c.second;
        if (part > limit) break;
        keep[c.first] = 0;
    }
    return MC_OK;
}

int mc_coverage_set_keep(mc_ctx* ctx, const uint8_t* keep, uint64_t numTargets)
{
    if (!ctx) return MC_ERR_INVALID;
    CoverageState* S = nullptr; ClassifyState* Cl = nullptr;
    const int rc = ensure_state(ctx, "mc_coverage_set_keep", &S, &Cl);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(ctx->coverageMtx);
    HIP_TRY(ctx, hipDeviceSynchronize());                                                  // (drops that still run finish with the old mask)
    if (S->dKeep) { (void)hipFree(S->dKeep); S->dKeep = nullptr; S->keepTargets = 0; }
    if (!keep) return MC_OK;
    HIP_TRY(ctx, hipMalloc((void**)&S->dKeep, std::max<uint64_t>(numTargets, 1)));
    if (numTargets) HIP_TRY(ctx, hipMemcpy(S->dKeep, keep, numTargets, hipMemcpyHostToDevice));
    S->keepTargets = numTargets;
    return MC_OK;
}

int mc_coverage_drop(mc_ctx* ctx, const mc_candidate* in, uint32_t n, uint32_t stride, int flags, mc_candidate* out, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_COVERAGE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_coverage_drop: unknown flag");
    if (stride == 0) return fail(ctx, MC_ERR_INVALID, "mc_coverage_drop: stride must be at least 1");
    if (n > 0) {
        if (!in || !out) return fail(ctx, MC_ERR_INVALID, "mc_coverage_drop: null array");
        const uintptr_t bytes = (uintptr_t)n * stride * sizeof(mc_candidate), i0 = (uintptr_t)in, o0 = (uintptr_t)out;
        if (i0 != o0 && ranges_overlap(i0, i0 + bytes, o0, o0 + bytes)) return fail(ctx, MC_ERR_INVALID, "mc_coverage_drop: out overlaps in without being it");
        if (!(flags & MC_COVERAGE_HOST) && ((i0 | o0) & 15u)) return fail(ctx, MC_ERR_INVALID, "mc_coverage_drop: device arrays must be 16-byte aligned");
    }
    // ... then state
    CoverageState* S = nullptr; ClassifyState* Cl = nullptr;
    int rc = ensure_state(ctx, "mc_coverage_drop", &S, &Cl);
    if (rc) return rc;
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (!(flags & MC_COVERAGE_HOST) || n == 0) {
        std::lock_guard<std::mutex> state(ctx->coverageMtx);                              // (mc_coverage_set_keep frees the mask under this mutex, after the device has drained)
        if (!S->dKeep) return fail(ctx, MC_ERR_STATE, "mc_coverage_drop: no keep mask (mc_coverage_set_keep)");
        if (n == 0) return MC_OK;
        hipLaunchKernelGGL(coverage_drop_kernel, dim3(row_blocks(n, kBlock, kMaxBlocks)), dim3(kBlock), 0, st, in, out, n, stride, S->dKeep, S->keepTargets);
        HIP_TRY(ctx, hipGetLastError());
        return MC_OK;
    }
    std::lock_guard<std::mutex> lock(S->stageMtx);
    return for_each_staged_piece(ctx, st, S->stageIn, in, n, stride, [&](const mc_candidate* dRows, uint32_t done, uint32_t m) {
        mc_candidate* d = const_cast<mc_candidate*>(dRows);                                // (the staging buffer: dropped in place)
        {
            std::lock_guard<std::mutex> state(ctx->coverageMtx);
            if (!S->dKeep) return fail(ctx, MC_ERR_STATE, "mc_coverage_drop: no keep mask (mc_coverage_set_keep)");
            hipLaunchKernelGGL(coverage_drop_kernel, dim3(row_blocks(m, kBlock, kMaxBlocks)), dim3(kBlock), 0, st, d, d, m, stride, S->dKeep, S->keepTargets);
            HIP_TRY(ctx, hipGetLastError());
        }
        HIP_TRY(ctx, hipMemcpyAsync(out + (uint64_t)done * stride, d, (uint64_t)m * stride * sizeof(mc_candidate), hipMemcpyDeviceToHost, st));
        return (int)MC_OK;
    });
}

}  // extern "C"
