// metacache_amd/csrc/classify.hip -- mc_classify_candidates / mc_classify_tally: the reference's ranked-LCA vote over a read's top
// candidates (classification.cpp:146-189, sequence_classification + ranked_lca of taxonomy.hpp; options -hitmin, -hitdiff, -lowest,
// -highest) and its per-rank / per-taxon read counts (classification_statistics, the table behind -abundances), on the device.
//
// ONE LANE PER READ (taxon_vote_kernel).  A lane reads {tgt, hits} of its candidates -- 8 of an entry's 16 bytes -- until the list ends
// or a candidate falls to the threshold, looks the lineages up and stores one 8-byte mc_assignment; consecutive lanes store consecutive
// assignments.  The lineage table lies RANK-MAJOR on the device (lin[rank * targets + target]): most reads have a single voter and need
// one slot of one target, so what the common case touches is one plane of 4 bytes per target (160 kB for 40 000 targets) instead of
// every line of the 84-byte rows (3.4 MB); the walk of a shared lineage takes two words per rank step in either layout.
// The tallies are 64-bit counters in the context.  A wave first adds up the lanes that agree (one add per wave and distinct value); the
// 22 rank bins then go through a histogram in LDS, the taxa through a small hash table in LDS that a block keeps over all its reads --
// the taxa a sample piles onto claim their slots with the block's first reads -- and both reach the global counters once, at the
// block's end.  A taxon that finds no slot goes to its global counter directly (many taxa, few reads each: no contention there).
// Plain HIP C++; no inline assembly.
#include "rows_common.h"

#include <algorithm>
#include <cmath>
#include <cstring>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kBins = MC_NUM_RANKS + 1, kMaxBlocks = 2048;
constexpr int kWaveRounds = 8;           // taxa a wave adds up across its lanes before the rest add their own 1
constexpr uint32_t kTaxonSlots = 512, kTaxonSlotBits = 9, kTaxonProbes = 2;   // a block's taxon table in LDS: slots (a power of two), slots a taxon tries

struct VoteArgs {
    const mc_candidate* cands;
    const uint32_t* lin;
    mc_assignment* out;
    unsigned long long* assigned;        // [kBins]
    unsigned long long* taxonCounts;     // [numCounts]
    uint32_t n, stride, numTargets;
    uint32_t hitsMin;
    float hitsDiff;
    int lowest, highest;
};

template <bool TALLY>
__global__ __launch_bounds__(kBlock) void taxon_vote_kernel(VoteArgs a)
{
    __shared__ uint32_t binCount[kBins];
    __shared__ uint32_t slotTaxon[TALLY ? kTaxonSlots : 1], slotCount[TALLY ? kTaxonSlots : 1];     // slotTaxon 0: free
    if (TALLY) {
        if (threadIdx.x < kBins) binCount[threadIdx.x] = 0;
        for (uint32_t s = threadIdx.x; s < kTaxonSlots; s += kBlock) { slotTaxon[s] = 0; slotCount[s] = 0; }
        __syncthreads();
    }
    const uint32_t nT = a.numTargets;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < a.n; base += step) {      // (the same trips for every lane of a block)
        const uint64_t i = base + threadIdx.x;
        const bool active = i < a.n;
        uint32_t taxon = 0, rank = MC_NUM_RANKS, voters = 0;
        if (active) {
            const uint2* c = reinterpret_cast<const uint2*>(a.cands + i * a.stride);     // entry j: c[2 * j] = {tgt, hits}
            const uint2 top = c[0];
            if (top.y != 0 && top.y >= a.hitsMin && top.x < nT) {
                int r;                                                                   // the rank of tax(cand[0]): where the LCA walk begins
                uint32_t t = taxon_of_target(a.lin, nT, top.x, a.lowest, r);
                if (t) {
                    const float threshold = top.y > a.hitsMin ? (float)(top.y - a.hitsMin) * a.hitsDiff : 0.0f;
                    uint32_t v = 1;
                    for (uint32_t j = 1; j < a.stride; ++j) {
                        const uint2 cj = c[2 * j];
                        if (cj.y == 0 || !((float)cj.y > threshold)) break;
                        ++v;
                        // ranked_lca: the first rank from r up on which both lineages name the same taxon
                        uint32_t l = 0;
                        if (cj.x < nT)
                            for (; r < MC_NUM_RANKS; ++r) {
                                const uint32_t x = a.lin[(uint64_t)r * nT + top.x];
                                if (x && x == a.lin[(uint64_t)r * nT + cj.x]) { l = x; break; }
                            }
                        t = l;
                        if (!t || r > a.highest) { t = 0; break; }
                    }
                    if (t && r <= a.highest) { taxon = t; rank = (uint32_t)r; voters = v < 255u ? v : 255u; }
                }
            }
            *reinterpret_cast<uint2*>(a.out + i) = make_uint2(taxon, rank | (voters << 8));   // {taxon, info}
        }
        if (TALLY) {
            wave_add_by_key(rank, active, (int)kBins, [&](uint32_t k, uint32_t c) { atomicAdd(&binCount[k], c); });
            wave_add_by_key(taxon, active && taxon != 0, kWaveRounds, [&](uint32_t k, uint32_t c) {
                const uint32_t h = (k * 2654435761u) >> (32 - kTaxonSlotBits);
                for (uint32_t probe = 0; probe < kTaxonProbes; ++probe) {
                    const uint32_t s = (h + probe) & (kTaxonSlots - 1);
                    const uint32_t owner = atomicCAS(&slotTaxon[s], 0u, k);
                    if (owner == 0 || owner == k) { atomicAdd(&slotCount[s], c); return; }
                }
                atomicAdd(&a.taxonCounts[k], (unsigned long long)c);
            });
        }
    }
    if (TALLY) {
        __syncthreads();
        if (threadIdx.x < kBins && binCount[threadIdx.x]) atomicAdd(&a.assigned[threadIdx.x], (unsigned long long)binCount[threadIdx.x]);
        for (uint32_t s = threadIdx.x; s < kTaxonSlots; s += kBlock)
            if (slotCount[s]) atomicAdd(&a.taxonCounts[slotTaxon[s]], (unsigned long long)slotCount[s]);
    }
}

}  // namespace

// the device copy of the lineage table and the tallies that are sized by it: made on first use, made again after mc_set_lineages
// (the tallies then start from zero: their taxon indices belonged to the old table)
int mcamd::ensure_classify_state(mc_ctx* ctx, ClassifyState** out)
{
    std::lock_guard<std::mutex> lock(ctx->classifyMtx);
    if (!ctx->classify) ctx->classify = new ClassifyState;
    ClassifyState& S = *ctx->classify;
    *out = &S;
    // a context without lineages that has a taxon table (mc_merge_results_classify): no lineage planes, the tallies sized by the taxon table
    const bool byTaxa = ctx->lineages.empty() && ctx->taxonTableSet;
    if (byTaxa ? (S.byTaxonTable && S.taxonVersion == ctx->taxonTableVersion && S.dTally) : (!S.byTaxonTable && S.version == ctx->lineageVersion && S.dLin)) return MC_OK;
    if (S.dLin) {                                                  // (a new table: votes that still run finish with the old one)
        HIP_TRY(ctx, hipDeviceSynchronize());
        (void)hipFree(S.dLin); S.dLin = nullptr;
    }
    if (S.dTally) { (void)hipFree(S.dTally); S.dTally = nullptr; }
    S.byTaxonTable = byTaxa;
    if (byTaxa) {
        S.numTargets = 0;
        S.numCounts = (uint64_t)ctx->taxonRank.size() + 1;
        HIP_TRY(ctx, hipMalloc((void**)&S.dTally, (kBins + S.numCounts) * 8));
        HIP_TRY(ctx, hipMemset(S.dTally, 0, (kBins + S.numCounts) * 8));
        S.taxonVersion = ctx->taxonTableVersion;
        S.version = ~0ull;
        return MC_OK;
    }
    const uint64_t nt = ctx->lineages.size() / MC_NUM_RANKS;
    if (nt > 0xFFFFFFFFull) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_classify: more than 2^32 targets");
    std::vector<uint32_t> planes(nt * MC_NUM_RANKS);
    uint32_t largest = 0;
    for (uint64_t t = 0; t < nt; ++t)
        for (uint32_t r = 0; r < MC_NUM_RANKS; ++r) {
            const uint32_t x = ctx->lineages[t * MC_NUM_RANKS + r];
            planes[(uint64_t)r * nt + t] = x;
            largest = std::max(largest, x);
        }
    S.numTargets = (uint32_t)nt;
    S.numCounts = (uint64_t)largest + 1;
    HIP_TRY(ctx, hipMalloc((void**)&S.dLin, planes.size() * 4));
    HIP_TRY(ctx, hipMalloc((void**)&S.dTally, (kBins + S.numCounts) * 8));
    HIP_TRY(ctx, hipMemcpy(S.dLin, planes.data(), planes.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(S.dTally, 0, (kBins + S.numCounts) * 8));
    S.version = ctx->lineageVersion;
    return MC_OK;
}

namespace {

void launch_vote(const ClassifyState& S, const mc_classify_options& o, const mc_candidate* cands, uint32_t n, uint32_t stride, bool tally,
                 mc_assignment* out, hipStream_t st)
{
    VoteArgs a{};
    a.cands = cands; a.lin = S.dLin; a.out = out; a.assigned = S.dTally; a.taxonCounts = S.dTally + kBins;
    a.n = n; a.stride = stride; a.numTargets = S.numTargets;
    a.hitsMin = o.hits_min; a.hitsDiff = o.hits_diff; a.lowest = o.lowest_rank; a.highest = o.highest_rank;
    const uint32_t blocks = row_blocks(n, kBlock, kMaxBlocks);
    if (tally) hipLaunchKernelGGL(taxon_vote_kernel<true>, dim3(blocks), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(taxon_vote_kernel<false>, dim3(blocks), dim3(kBlock), 0, st, a);
}

}  // namespace

namespace mcamd {

void free_classify_state(mc_ctx* ctx)
{
    if (!ctx->classify) return;
    ClassifyState& S = *ctx->classify;
    if (S.dLin) (void)hipFree(S.dLin);
    if (S.dTally) (void)hipFree(S.dTally);
    if (S.stageIn.p) (void)hipFree(S.stageIn.p);
    if (S.stageOut.p) (void)hipFree(S.stageOut.p);
    delete ctx->classify;
    ctx->classify = nullptr;
}

}  // namespace mcamd

extern "C" {

void mc_classify_options_default(mc_classify_options* o)
{
    if (!o) return;
    o->hits_min = 0; o->hits_diff = 1.0f; o->lowest_rank = 0; o->highest_rank = MC_NUM_RANKS - 1;
}

int mc_classify_candidates(mc_ctx* ctx, const mc_classify_options* o, const mc_candidate* cands, uint32_t n, uint32_t stride, int flags,
                           mc_assignment* out, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!o) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: no options");
    if (flags & ~(MC_CLASSIFY_HOST | MC_CLASSIFY_TALLY)) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: unknown flag");
    if (stride == 0) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: stride must be at least 1");
    if (o->lowest_rank < 0 || o->lowest_rank >= MC_NUM_RANKS || o->highest_rank < 0 || o->highest_rank >= MC_NUM_RANKS)
        return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: ranks must be 0 .. MC_NUM_RANKS - 1");
    if (o->lowest_rank > o->highest_rank) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: lowest_rank above highest_rank");
    if (!std::isfinite(o->hits_diff) || o->hits_diff < 0.0f) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: hits_diff must be finite and not negative");
    if (n > 0) {
        if (!cands || !out) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: null array");
        const uintptr_t c0 = (uintptr_t)cands, c1 = c0 + (uintptr_t)n * stride * sizeof(mc_candidate), o0 = (uintptr_t)out, o1 = o0 + (uintptr_t)n * sizeof(mc_assignment);
        if (ranges_overlap(c0, c1, o0, o1)) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: out overlaps cands");
        if (!(flags & MC_CLASSIFY_HOST) && ((c0 | o0) & 7u)) return fail(ctx, MC_ERR_INVALID, "mc_classify_candidates: device arrays must be 8-byte aligned");
    }
    if (n == 0) return MC_OK;
    // ... then state
    if (ctx->lineages.empty()) return fail(ctx, MC_ERR_STATE, "mc_classify_candidates: the context has no lineages (mc_set_lineages)");
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_classify_candidates: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ClassifyState* S = nullptr;
    int rc = ensure_classify_state(ctx, &S);
    if (rc) return rc;
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const bool tally = (flags & MC_CLASSIFY_TALLY) != 0;
    if (!(flags & MC_CLASSIFY_HOST)) {
        launch_vote(*S, *o, cands, n, stride, tally, out, st);
        HIP_TRY(ctx, hipGetLastError());
        return MC_OK;
    }
    // host arrays: in pieces of at most 64 MB of candidates through the staging buffers, one caller at a time
    std::lock_guard<std::mutex> lock(S->stageMtx);
    if ((rc = grow(ctx, S->stageIn, staged_piece_bytes(n, stride))) != MC_OK || (rc = grow(ctx, S->stageOut, (uint64_t)staged_piece_rows(n, stride) * sizeof(mc_assignment))) != MC_OK) return rc;
    return for_each_staged_piece(ctx, st, S->stageIn, cands, n, stride, [&](const mc_candidate* dRows, uint32_t done, uint32_t m) {
        launch_vote(*S, *o, dRows, m, stride, tally, (mc_assignment*)S->stageOut.p, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(out + done, S->stageOut.p, (uint64_t)m * sizeof(mc_assignment), hipMemcpyDeviceToHost, st));
        return (int)MC_OK;
    });
}

int mc_classify_tally(mc_ctx* ctx, uint64_t assigned[MC_NUM_RANKS + 1], uint64_t* taxonCounts, uint64_t capacity, uint64_t* numCounts, int reset)
{
    if (!ctx) return MC_ERR_INVALID;
    if (capacity > 0 && !taxonCounts) return fail(ctx, MC_ERR_INVALID, "mc_classify_tally: capacity without an array");
    if (ctx->lineages.empty() && !ctx->taxonTableSet) return fail(ctx, MC_ERR_STATE, "mc_classify_tally: the context has no lineages (mc_set_lineages)");
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_classify_tally: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    ClassifyState* S = nullptr;
    const int rc = ensure_classify_state(ctx, &S);
    if (rc) return rc;
    if (const int drc = drain_query_streams(ctx)) return drc;
    const uint64_t take = std::min(capacity, S->numCounts);
    if (assigned) HIP_TRY(ctx, hipMemcpyAsync(assigned, S->dTally, kBins * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (take) HIP_TRY(ctx, hipMemcpyAsync(taxonCounts, S->dTally + kBins, take * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (reset) HIP_TRY(ctx, hipMemsetAsync(S->dTally, 0, (kBins + S->numCounts) * 8, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (numCounts) *numCounts = S->numCounts;
    return MC_OK;
}

}  // extern "C"
