// metacache_amd/csrc/evaluate.hip -- mc_evaluate_assignments / mc_evaluate_tally: the ground-truth block of the reference's query summary
// (classification.cpp:237-295 update_coverage_statistics + evaluate_classification, classification_statistics.hpp:87-107
// assign_known_correct; options -precision, -taxon-coverage) on the device.  The rule, step by step: include/metacache_amd.h.
//
// ONE LANE PER READ (taxon_evaluate_kernel).  A lane reads its assignment (8 bytes) and its truth (4), loads the two taxa's rows into
// registers, compares their ranked lineages and stores one 4-byte verdict; consecutive lanes read and store consecutive entries.
// The taxon table lies on the device as ROWS PADDED TO 128 BYTES, one per taxon: the 21 lineage slots, then in the spare
// words the taxon's own rank and covered flag, a mask of its filled slots, a mask of the slots whose taxon is covered and the 21 ranks
// of the slots' taxa.  Unlike the vote, whose common case is ONE slot of one target (rank-major planes, classify.hip), the common case
// here is a walk over two lineages, and the coverage pass reads the truth's whole row: with rows a read touches two lines -- its two
// taxa's -- however long the walk, and never a third taxon's (the rank and the covered flag of a slot's taxon are in the row).
// The tallies are 64-bit counters in the context.  A block keeps all of them as 32-bit counters in LDS; a wave first adds up the lanes
// that agree (wave_add_by_key: one LDS add per wave and distinct bin) and the block sends what is not zero to the global counters once,
// at its end.  Plain HIP C++; no inline assembly.
#include "rows_common.h"

#include <algorithm>
#include <cstring>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kBins = MC_NUM_RANKS + 1, kMaxBlocks = 2048;
// a row of the device table, in 32-bit words
constexpr uint32_t kRowWords = 32;
constexpr uint32_t kWordMeta = MC_NUM_RANKS;           // own rank | covered << 8
constexpr uint32_t kWordMask = MC_NUM_RANKS + 1;       // bit r: slot r is filled
constexpr uint32_t kWordCovered = MC_NUM_RANKS + 2;    // bit r: slot r's taxon is covered
constexpr uint32_t kWordSlotRanks = MC_NUM_RANKS + 3;  // byte r of these 6 words: the rank of slot r's taxon
static_assert(kWordSlotRanks + (MC_NUM_RANKS + 3) / 4 <= kRowWords, "a row holds its slots and the spare words");
// the counters, in the order of mc_evaluation
constexpr uint32_t kAssigned = 0, kKnown = kBins, kCorrect = 2 * kBins, kWrong = 3 * kBins, kCoverage = 4 * kBins, kReads = 8 * kBins,
                   kOutOfTable = kReads + 1, kCounters = kReads + 2;
static_assert(sizeof(mc_evaluation) == kCounters * 8, "the device counters are an mc_evaluation");
static_assert(sizeof(mc_verdict) == 4 && sizeof(mc_assignment) == 8, "ABI sizes");

struct EvalArgs {
    const mc_assignment* assigned;
    const uint32_t* truth;
    uint32_t* verdicts;                  // mc_verdict as one word: known | correct << 8 | flags << 16; may be null
    const uint32_t* rows;                // [numTaxa][kRowWords]
    unsigned long long* tally;           // [kCounters]
    uint32_t n, numTaxa;
};

// a row in registers: the whole line comes as eight 16-byte loads that are in flight together (a slot-by-slot walk would wait for
// memory once per step, and the coverage pass would find its line gone from the L1 of a CU whose 2 048 lanes hold a line each)
struct Row { uint32_t w[kRowWords]; };

__device__ __forceinline__ void load_row(Row& R, const uint32_t* rows, uint32_t taxon)      // taxon != 0, within the table
{
    const uint4* p = reinterpret_cast<const uint4*>(rows + (uint64_t)(taxon - 1) * kRowWords);
#pragma unroll
    for (uint32_t q = 0; q < kRowWords / 4; ++q) {
        const uint4 v = p[q];
        R.w[4 * q] = v.x; R.w[4 * q + 1] = v.y; R.w[4 * q + 2] = v.z; R.w[4 * q + 3] = v.w;
    }
}

// byte r of the row's slot ranks; r is a run-time value, the words are registers: a select per word, no indexed access
__device__ __forceinline__ uint32_t slot_rank(const Row& R, uint32_t r)
{
    uint32_t word = 0;
#pragma unroll
    for (uint32_t q = 0; q < (MC_NUM_RANKS + 3) / 4; ++q) word = (r >> 2) == q ? R.w[kWordSlotRanks + q] : word;
    return (word >> ((r & 3u) * 8u)) & 0xFFu;
}

template <bool TALLY, bool COVERAGE>
__global__ __launch_bounds__(kBlock) void taxon_evaluate_kernel(EvalArgs e)
{
    __shared__ uint32_t bins[TALLY ? kCounters : 1];
    if (TALLY) {
        for (uint32_t s = threadIdx.x; s < kCounters; s += kBlock) bins[s] = 0;
        __syncthreads();
    }
    const uint32_t none = MC_NUM_RANKS;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < e.n; base += step) {      // (the same trips for every lane of a block)
        const uint64_t i = base + threadIdx.x;
        const bool active = i < e.n;
        uint32_t a = 0, t = 0, beyond = 0;
        if (active) {
            a = reinterpret_cast<const uint2*>(e.assigned)[i].x;                         // {taxon, info}: info is not looked at
            t = e.truth[i];
            if (a > e.numTaxa) { a = 0; ++beyond; }
            if (t > e.numTaxa) { t = 0; ++beyond; }
        }
        Row A, T;
#pragma unroll
        for (uint32_t q = 0; q < kRowWords; ++q) { A.w[q] = 0; T.w[q] = 0; }
        if (a) load_row(A, e.rows, a);
        if (t) load_row(T, e.rows, t);
        const uint32_t ar = a ? (A.w[kWordMeta] & 0xFFu) : none, kr = t ? (T.w[kWordMeta] & 0xFFu) : none, maskT = T.w[kWordMask];
        // ranked_lca: the first slot that both lineages fill with the same taxon; its taxon's rank
        uint32_t same = 0;
#pragma unroll
        for (uint32_t r = 0; r < MC_NUM_RANKS; ++r) same |= (A.w[r] != 0 && A.w[r] == T.w[r]) ? 1u << r : 0u;
        uint32_t cr = same ? slot_rank(A, (uint32_t)__ffs((int)same) - 1u) : none;
        cr = max(cr, max(ar, kr));
        const bool wrong = kr != none && cr > kr && cr > ar;
        if (active && e.verdicts) e.verdicts[i] = kr | (cr << 8) | ((wrong ? 1u : 0u) << 16);
        if (TALLY) {
            wave_add_by_key(ar, active, (int)kBins, [&](uint32_t k, uint32_t c) { atomicAdd(&bins[kAssigned + k], c); });
            wave_add_by_key(kr, active, (int)kBins, [&](uint32_t k, uint32_t c) { atomicAdd(&bins[kKnown + k], c); });
            wave_add_by_key(cr, active && kr != none, (int)kBins, [&](uint32_t k, uint32_t c) { atomicAdd(&bins[kCorrect + k], c); });
            wave_add_by_key(cr - 1u, active && wrong, (int)kBins, [&](uint32_t k, uint32_t c) { atomicAdd(&bins[kWrong + k], c); });   // (wrong: cr >= 1)
            const uint32_t reads = (uint32_t)__popcll(__ballot(active));
            const uint32_t out = (uint32_t)(__popcll(__ballot(beyond >= 1)) + __popcll(__ballot(beyond == 2)));
            if ((threadIdx.x & 63u) == 0) {
                atomicAdd(&bins[kReads], reads);
                if (out) atomicAdd(&bins[kOutOfTable], out);
            }
            if (COVERAGE) {
                // update_coverage_statistics: every taxon of the truth's lineage is a hit on it (the read was assigned at its rank or below)
                // or not, and covered or not.  A slot is the same for the whole wave, its taxon's rank nearly always: one or two classes per slot.
                const uint32_t covT = T.w[kWordCovered];
#pragma unroll
                for (uint32_t r = 0; r < MC_NUM_RANKS; ++r) {
                    const bool has = (maskT >> r) & 1u;
                    if (!__ballot(has)) continue;
                    const uint32_t rr = has ? ((T.w[kWordSlotRanks + (r >> 2)] >> ((r & 3u) * 8u)) & 0xFFu) : none;
                    const bool on = a != 0 && rr >= ar, covered = (covT >> r) & 1u;
                    const uint32_t cls = covered ? (on ? 0u : 3u) : (on ? 1u : 2u);          // true_pos, false_pos, true_neg, false_neg
                    wave_add_by_key(rr * 4u + cls, has, (int)(4 * kBins), [&](uint32_t k, uint32_t c) { atomicAdd(&bins[kCoverage + k], c); });
                }
            }
        }
    }
    if (TALLY) {
        __syncthreads();
        for (uint32_t s = threadIdx.x; s < kCounters; s += kBlock)
            if (bins[s]) atomicAdd(&e.tally[s], (unsigned long long)bins[s]);
    }
}

}  // namespace

namespace mcamd {

struct EvaluateState {                   // what the context keeps on the device for mc_evaluate_*
    uint64_t version = ~0ull;            // ctx->taxonTableVersion the device copy was made from
    uint32_t* dRows = nullptr;           // [numTaxa][kRowWords]
    uint32_t numTaxa = 0;
    bool hasCovered = false;
    unsigned long long* dTally = nullptr;   // [kCounters], an mc_evaluation
    std::mutex stageMtx;                 // MC_EVALUATE_HOST callers take turns at the staging buffers
    DevBuf stageAssigned, stageTruth, stageVerdicts;
};

void free_evaluate_state(mc_ctx* ctx)
{
    if (!ctx->evaluate) return;
    EvaluateState& S = *ctx->evaluate;
    if (S.dRows) (void)hipFree(S.dRows);
    if (S.dTally) (void)hipFree(S.dTally);
    for (DevBuf* b : {&S.stageAssigned, &S.stageTruth, &S.stageVerdicts}) if (b->p) (void)hipFree(b->p);
    delete ctx->evaluate;
    ctx->evaluate = nullptr;
}

}  // namespace mcamd

namespace {

// the device copy of the taxon table and the tallies: made on first use, made again after mc_set_taxon_table (the tallies then start
// from zero: their reads were judged by the old table)
int ensure_evaluate_state(mc_ctx* ctx, EvaluateState** out)
{
    std::lock_guard<std::mutex> lock(ctx->evaluateMtx);
    if (!ctx->evaluate) ctx->evaluate = new EvaluateState;
    EvaluateState& S = *ctx->evaluate;
    *out = &S;
    if (S.version == ctx->taxonTableVersion && S.dRows) return MC_OK;
    if (S.dRows) {                                                 // (a new table: evaluations that still run finish with the old one)
        HIP_TRY(ctx, hipDeviceSynchronize());
        (void)hipFree(S.dRows); S.dRows = nullptr;
    }
    const uint64_t nt = ctx->taxonRank.size();
    const bool cov = ctx->taxonCoveredSet;
    std::vector<uint32_t> rows(std::max<uint64_t>(nt, 1) * kRowWords, 0u);
    for (uint64_t x = 0; x < nt; ++x) {
        uint32_t* R = &rows[x * kRowWords];
        R[kWordMeta] = ctx->taxonRank[x] | ((cov && ctx->taxonCovered[x]) ? 0x100u : 0u);
        for (uint32_t r = 0; r < MC_NUM_RANKS; ++r) {
            const uint32_t y = ctx->taxonLin[x * MC_NUM_RANKS + r];              // (mc_set_taxon_table: y <= nt)
            if (!y) continue;
            R[r] = y;
            R[kWordMask] |= 1u << r;
            if (cov && ctx->taxonCovered[y - 1]) R[kWordCovered] |= 1u << r;
            R[kWordSlotRanks + (r >> 2)] |= (uint32_t)ctx->taxonRank[y - 1] << ((r & 3u) * 8u);   // (<= MC_NUM_RANKS: mc_set_taxon_table)
        }
    }
    S.numTaxa = (uint32_t)nt;
    S.hasCovered = cov;
    HIP_TRY(ctx, hipMalloc((void**)&S.dRows, rows.size() * 4));
    if (!S.dTally) HIP_TRY(ctx, hipMalloc((void**)&S.dTally, kCounters * 8));
    HIP_TRY(ctx, hipMemcpy(S.dRows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(S.dTally, 0, kCounters * 8));
    S.version = ctx->taxonTableVersion;
    return MC_OK;
}

void launch_evaluate(mc_ctx* ctx, const EvaluateState& S, const mc_assignment* assigned, const uint32_t* truth, uint32_t n, int flags,
                     mc_verdict* verdicts, hipStream_t st)
{
    EvalArgs e{};
    e.assigned = assigned; e.truth = truth; e.verdicts = reinterpret_cast<uint32_t*>(verdicts); e.rows = S.dRows; e.tally = S.dTally;
    e.n = n; e.numTaxa = S.numTaxa;
    const uint32_t blocks = row_blocks(n, kBlock, kMaxBlocks);
    ScopedTimer timer(ctx, "taxon_evaluate", st);
    if (flags & MC_EVALUATE_COVERAGE) hipLaunchKernelGGL((taxon_evaluate_kernel<true, true>), dim3(blocks), dim3(kBlock), 0, st, e);
    else if (flags & MC_EVALUATE_TALLY) hipLaunchKernelGGL((taxon_evaluate_kernel<true, false>), dim3(blocks), dim3(kBlock), 0, st, e);
    else hipLaunchKernelGGL((taxon_evaluate_kernel<false, false>), dim3(blocks), dim3(kBlock), 0, st, e);
}

}  // namespace

extern "C" {

int mc_evaluate_assignments(mc_ctx* ctx, const mc_assignment* assigned, const uint32_t* truth, uint32_t n, int flags, mc_verdict* verdicts,
                            void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~(MC_EVALUATE_HOST | MC_EVALUATE_TALLY | MC_EVALUATE_COVERAGE)) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_assignments: unknown flag");
    if (n > 0 && (!assigned || !truth)) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_assignments: null array");
    if (!verdicts && !(flags & MC_EVALUATE_TALLY)) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_assignments: neither verdicts nor MC_EVALUATE_TALLY: nothing to do");
    if ((flags & MC_EVALUATE_COVERAGE) && !(flags & MC_EVALUATE_TALLY)) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_assignments: MC_EVALUATE_COVERAGE needs MC_EVALUATE_TALLY");
    if (n > 0) {
        const uintptr_t a0 = (uintptr_t)assigned, a1 = a0 + (uintptr_t)n * sizeof(mc_assignment), t0 = (uintptr_t)truth, t1 = t0 + (uintptr_t)n * 4,
                        v0 = (uintptr_t)verdicts, v1 = v0 + (uintptr_t)n * sizeof(mc_verdict);
        if (!(flags & MC_EVALUATE_HOST) && ((a0 & 7u) || ((t0 | v0) & 3u))) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_assignments: device arrays must be aligned (assigned: 8 bytes, truth and verdicts: 4)");
        if (verdicts && (ranges_overlap(a0, a1, v0, v1) || ranges_overlap(t0, t1, v0, v1))) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_assignments: verdicts overlaps an input");
    }
    if (n == 0) return MC_OK;
    // ... then state
    if (!ctx->taxonTableSet) return fail(ctx, MC_ERR_STATE, "mc_evaluate_assignments: the context has no taxon table (mc_set_taxon_table)");
    if ((flags & MC_EVALUATE_COVERAGE) && !ctx->taxonCoveredSet) return fail(ctx, MC_ERR_STATE, "mc_evaluate_assignments: MC_EVALUATE_COVERAGE needs a taxon table with a covered array");
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_evaluate_assignments: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EvaluateState* S = nullptr;
    int rc = ensure_evaluate_state(ctx, &S);
    if (rc) return rc;
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (!(flags & MC_EVALUATE_HOST)) {
        launch_evaluate(ctx, *S, assigned, truth, n, flags, verdicts, st);
        HIP_TRY(ctx, hipGetLastError());
        return MC_OK;
    }
    // host arrays: in pieces of at most 64 MB of pairs (or "evaluate_stage_rows" reads) through the staging buffers, one caller at a time
    // (a call that fails after its first piece HAS counted the pieces before: the tallies of a failed call are undefined)
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint32_t most = ctx->evaluateStageRows ? ctx->evaluateStageRows : (uint32_t)(kStagePieceBytes / (sizeof(mc_assignment) + 8));
    const uint32_t piece = std::min(n, most);
    if ((rc = grow(ctx, S->stageAssigned, (uint64_t)piece * sizeof(mc_assignment))) != MC_OK || (rc = grow(ctx, S->stageTruth, (uint64_t)piece * 4)) != MC_OK ||
        (verdicts && (rc = grow(ctx, S->stageVerdicts, (uint64_t)piece * sizeof(mc_verdict))) != MC_OK)) return rc;
    for (uint64_t done = 0; done < n; done += piece) {                  // (64 bits: n may lie within one piece of 2^32)
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - done);
        HIP_TRY(ctx, hipMemcpyAsync(S->stageAssigned.p, assigned + done, (uint64_t)m * sizeof(mc_assignment), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(S->stageTruth.p, truth + done, (uint64_t)m * 4, hipMemcpyHostToDevice, st));
        launch_evaluate(ctx, *S, (const mc_assignment*)S->stageAssigned.p, (const uint32_t*)S->stageTruth.p, m, flags,
                        verdicts ? (mc_verdict*)S->stageVerdicts.p : nullptr, st);
        HIP_TRY(ctx, hipGetLastError());
        if (verdicts) HIP_TRY(ctx, hipMemcpyAsync(verdicts + done, S->stageVerdicts.p, (uint64_t)m * sizeof(mc_verdict), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return MC_OK;
}

int mc_evaluate_tally(mc_ctx* ctx, mc_evaluation* out, int reset)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!out) return fail(ctx, MC_ERR_INVALID, "mc_evaluate_tally: no place for the counters");
    if (!ctx->taxonTableSet) return fail(ctx, MC_ERR_STATE, "mc_evaluate_tally: the context has no taxon table (mc_set_taxon_table)");
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_evaluate_tally: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EvaluateState* S = nullptr;
    const int rc = ensure_evaluate_state(ctx, &S);
    if (rc) return rc;
    if (const int drc = drain_query_streams(ctx)) return drc;
    HIP_TRY(ctx, hipMemcpyAsync(out, S->dTally, kCounters * 8, hipMemcpyDeviceToHost, ctx->stream));
    if (reset) HIP_TRY(ctx, hipMemsetAsync(S->dTally, 0, kCounters * 8, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MC_OK;
}

}  // extern "C"
