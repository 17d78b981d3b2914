// metacache_amd/csrc/merge_results.hip -- mc_merge_results_*: the result lines of per-part query outputs cut and folded into one
// candidate list per query on the device, and the vote over those lists.  The rules are those of include/metacache_amd.h
// (read_results / insert_taxon_candidate / classify of mcq_main.cpp, after mode_merge.cpp:158-238, candidate_generation.hpp:172-231 and
// classification.cpp:146-189); a line this file cannot decide inside its rule makes the range IRREGULAR and nothing is changed.
//
// A result line names its query itself, so nothing has to be summed in front of a line: a tile is kTile consecutive bytes, a block owns
// a tile, a thread 16 consecutive bytes of it (one 16-byte load) and every line that STARTS in them.  A lane that owns a line walks it
// byte by byte to its end, wherever that lies.  The passes of one mc_merge_results_add, enqueued back to back and never waited for:
//   1. merge_validate_kernel  per tile: lines counted, every result line judged, the largest query, owner[q] claimed by the smallest
//                             line start (atomicMin: the result does not depend on the order)
//   2. merge_dups_kernel      per tile: a result line whose query is owned by another line, or -- MC_MERGE_CONTINUE -- was folded by an
//                             earlier piece of the same file, is an offence
//   3. merge_verdict_kernel   one thread: verdict, the new number of lists, status
//   4. merge_cut_kernel       the file rule: the lists and header places from the file's line count up to the old number are emptied
//   5. merge_fold_kernel      per tile: each result line again: header place, taxid -> taxon entry by binary search, the insert rule on
//                             the query's list in place; owner[q] is given back (with any verdict)
// Passes 4 and 5 read the verdict from device memory.  A query has ONE line per call (pass 2), so one lane alone works on a list: no
// atomic decides a value of the lists, the header places or status.  This is built to be right, not yet to be fast (7i).
// merge_vote_kernel (mc_merge_results_classify) is one lane per query over the store, the taxon table rank-major as classify.hip reads
// the lineages.  Plain HIP C++; no inline assembly.
#include "parse_scan.h"

#include <atomic>
#include <cmath>
#include <cstring>
#include <numeric>

using namespace mcamd;
using namespace mcamd::parsek;

namespace {

constexpr uint32_t kMaxBlocks = 2048;
constexpr uint32_t kMaxCandidates = 32, kBins = MC_NUM_RANKS + 1;
constexpr uint64_t kMaxCapacity = 0xFFFFFFFFull;         // a query is id - 1 with id <= 2^32 - 1
constexpr uint64_t kScratchBytes = 256;
// the call's workspace, in 32-bit words (zeroed in front of pass 1)
enum { wLines = 0, wComments, wOffenceInv /* kNone - offence; 0: none */, wMaxQ1, wVerdict, wBaseLo, wBaseHi, wOldLo, wOldHi };
// the context's device counters
enum { cLines = 0, cEntries, cUnknown, cRefused, cCounters };

struct MergeArgs {
    const uint8_t* B;
    uint32_t* ws;
    uint64_t* status;
    unsigned long long* counters;
    unsigned long long* count;               // the number of lists (the store's)
    uint2* lists; uint32_t* hdr; uint32_t* owner; uint32_t* epoch;
    const int64_t* ids; const uint32_t* rows;    // the taxids ascending, and the taxon entry of each
    uint64_t capacity, fileLines;
    uint32_t n, numIds, tophitsColumn, maxCand, cont, fileSeq, callNo;
    int32_t mergeBelow;
};

// clause 1 of the line rule: the digits at the line start -> the query
__device__ __forceinline__ bool parse_id(const MergeArgs& a, uint32_t& p, uint32_t& q)
{
    uint64_t id = 0;
    uint32_t digits = 0;
    for (uint32_t c; is_digit(c = byte_at(a.B, a.n, p)); ++p) { id = min(id * 10 + (c - '0'), 1ull << 40); ++digits; }
    if (!digits || id > 0xFFFFFFFFull) return false;
    q = id ? (uint32_t)id - 1 : 0u;
    return true;
}

// moves p behind the next `stop` of the line; false where the line ends first or holds a refused byte on the way
__device__ __forceinline__ bool skip_past(const MergeArgs& a, uint32_t& p, uint32_t stop)
{
    for (;; ++p) {
        const uint32_t c = byte_at(a.B, a.n, p);
        if (c == stop) { ++p; return true; }
        if (c == '\n' || is_refused(c)) return false;
    }
}

// clauses 1-4: the query, the header token and the place of the list's first byte
__device__ __forceinline__ bool parse_head(const MergeArgs& a, uint32_t s, uint32_t& q, uint32_t& hdrOff, uint32_t& hdrLen, uint32_t& listAt)
{
    uint32_t p = s;
    if (!parse_id(a, p, q)) return false;
    if (!skip_past(a, p, '|')) return false;
    uint32_t c;
    while ((c = byte_at(a.B, a.n, p)) == ' ' || c == '\t') ++p;
    hdrOff = p;
    for (; (c = byte_at(a.B, a.n, p)) != ' ' && c != '\t' && c != '\n'; ++p) if (c == '|' || is_refused(c)) return false;
    hdrLen = p - hdrOff;
    if (!hdrLen) return false;
    for (uint32_t k = 1; k < a.tophitsColumn; ++k) if (!skip_past(a, p, '|')) return false;
    if (!skip_past(a, p, '\t')) return false;
    listAt = p;
    return true;
}

// clause 5 and the rest of the line: every entry goes to sink(taxid, hits)
template <class Sink>
__device__ __forceinline__ bool parse_list(const MergeArgs& a, uint32_t p, Sink&& sink)
{
    uint32_t c = byte_at(a.B, a.n, p);
    if (c != '\t' && c != '\n') {
        for (;;) {
            const bool neg = c == '-';
            if (neg) ++p;
            int64_t taxid = 0;
            uint32_t digits = 0;
            for (; is_digit(c = byte_at(a.B, a.n, p)); ++p) { if (++digits > 18) return false; taxid = taxid * 10 + (int64_t)(c - '0'); }
            if (!digits || c != ':') return false;
            ++p;
            uint64_t hits = 0;
            digits = 0;
            for (; is_digit(c = byte_at(a.B, a.n, p)); ++p) { if (++digits > 10) return false; hits = hits * 10 + (c - '0'); }
            if (!digits || hits == 0 || hits > 0xFFFFFFFFull) return false;
            sink(neg ? -taxid : taxid, (uint32_t)hits);
            if (c == '\t' || c == '\n') break;
            if (c != ',') return false;
            c = byte_at(a.B, a.n, ++p);
        }
    }
    for (; (c = byte_at(a.B, a.n, p)) != '\n'; ++p) if (is_refused(c)) return false;
    return true;
}

// the taxon entry of a taxid (0: not in the table)
__device__ __forceinline__ uint32_t taxon_of_id(const MergeArgs& a, int64_t id)
{
    uint32_t lo = 0, hi = a.numIds;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.ids[mid] < id) lo = mid + 1; else hi = mid;
    }
    return (lo < a.numIds && a.ids[lo] == id) ? a.rows[lo] : 0u;
}

// the insert rule (insert_taxon_candidate) on a list of K pairs {taxon entry, hits} that ends at the first pair with hits == 0
__device__ __forceinline__ void insert_candidate(uint2* L, uint32_t K, uint2 c, int32_t mergeBelow)
{
    uint32_t size = 0;
    while (size < K && L[size].y != 0) ++size;
    if (size == K && L[K - 1].y >= c.y) return;
    if (mergeBelow != 0) {
        uint32_t i = 0;
        while (i < size && L[i].x != c.x) ++i;
        if (i < size) {
            if (c.y > L[i].y) {
                L[i] = c;
                for (uint32_t j = i; j > 0 && L[j].y > L[j - 1].y; --j) { const uint2 t = L[j]; L[j] = L[j - 1]; L[j - 1] = t; }
            }
            return;
        }
    }
    uint32_t j = 0;
    while (j < size && L[j].y >= c.y) ++j;                     // behind every entry with as many hits: ties keep the earlier one in front
    if (j == size && size == K) return;
    for (uint32_t k = min(size, K - 1); k > j; --k) L[k] = L[k - 1];
    L[j] = c;
}

// ---- the byte passes ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void merge_validate_kernel(MergeArgs a)
{
    const uint32_t p0 = blockIdx.x * kTile + threadIdx.x * 16u;
    uint32_t lines = 0, comments = 0, offenceInv = 0, maxQ1 = 0;
    for_each_line_start(a.B, a.n, p0, [&](uint32_t s) {
        if (a.B[s] == '#') { ++comments; return; }
        ++lines;
        uint32_t q = 0, hdrOff, hdrLen, listAt;
        const bool ok = parse_head(a, s, q, hdrOff, hdrLen, listAt) && parse_list(a, listAt, [](int64_t, uint32_t) {});
        if (!ok) { offenceInv = max(offenceInv, kNone - s); return; }
        maxQ1 = max(maxQ1, q + 1);
        if (q < a.capacity) atomicMin(&a.owner[q], s);
    });
    lines = wave_sum_u32(lines); comments = wave_sum_u32(comments); offenceInv = wave_max_u32(offenceInv); maxQ1 = wave_max_u32(maxQ1);
    if ((threadIdx.x & 63u) == 0) {                            // (sums and maxima: the same whatever the order)
        if (lines) atomicAdd(&a.ws[wLines], lines);
        if (comments) atomicAdd(&a.ws[wComments], comments);
        if (offenceInv) atomicMax(&a.ws[wOffenceInv], offenceInv);
        if (maxQ1) atomicMax(&a.ws[wMaxQ1], maxQ1);
    }
}

__global__ __launch_bounds__(kBlock) void merge_dups_kernel(MergeArgs a)
{
    const uint32_t p0 = blockIdx.x * kTile + threadIdx.x * 16u;
    uint32_t offenceInv = 0;
    for_each_line_start(a.B, a.n, p0, [&](uint32_t s) {
        if (a.B[s] == '#') return;
        uint32_t p = s, q = 0;
        if (!parse_id(a, p, q) || q >= a.capacity) return;
        if (a.owner[q] != s || (a.cont && a.epoch[q] == a.fileSeq)) offenceInv = max(offenceInv, kNone - s);
    });
    offenceInv = wave_max_u32(offenceInv);
    if ((threadIdx.x & 63u) == 0 && offenceInv) atomicMax(&a.ws[wOffenceInv], offenceInv);
}

__global__ void merge_verdict_kernel(MergeArgs a)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint64_t lines = a.ws[wLines], old = *a.count;
    const uint32_t inv = a.ws[wOffenceInv];
    const uint64_t base = a.cont ? old : (a.fileLines ? a.fileLines : lines);
    const uint64_t need = max(base, (uint64_t)a.ws[wMaxQ1]);
    const uint32_t verdict = inv ? MC_MERGE_IRREGULAR : need > a.capacity ? MC_MERGE_OVERFLOW : MC_MERGE_OK;
    a.ws[wVerdict] = verdict;
    a.ws[wBaseLo] = (uint32_t)base; a.ws[wBaseHi] = (uint32_t)(base >> 32);
    a.ws[wOldLo] = (uint32_t)old; a.ws[wOldHi] = (uint32_t)(old >> 32);
    if (verdict == MC_MERGE_OK) { *a.count = need; atomicAdd(&a.counters[cLines], (unsigned long long)lines); }
    else atomicAdd(&a.counters[cRefused], 1ull);
    a.status[0] = lines; a.status[1] = a.ws[wComments]; a.status[2] = verdict == MC_MERGE_OK ? need : old;
    a.status[3] = 0; a.status[4] = 0; a.status[5] = verdict; a.status[6] = inv ? kNone - inv : 0;
    a.status[7] = inv ? 0 : need;
}

__global__ __launch_bounds__(kBlock) void merge_cut_kernel(MergeArgs a)
{
    if (a.ws[wVerdict] != MC_MERGE_OK || a.cont) return;
    const uint64_t base = (uint64_t)a.ws[wBaseLo] | ((uint64_t)a.ws[wBaseHi] << 32), old = (uint64_t)a.ws[wOldLo] | ((uint64_t)a.ws[wOldHi] << 32);
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t q = base + (uint64_t)blockIdx.x * kBlock + threadIdx.x; q < old; q += step) {   // (old <= capacity)
        for (uint32_t k = 0; k < a.maxCand; ++k) a.lists[q * a.maxCand + k] = make_uint2(0u, 0u);
        a.hdr[3 * q] = 0; a.hdr[3 * q + 1] = 0; a.hdr[3 * q + 2] = 0;
    }
}

__global__ __launch_bounds__(kBlock) void merge_fold_kernel(MergeArgs a)
{
    const uint32_t p0 = blockIdx.x * kTile + threadIdx.x * 16u;
    const bool fold = a.ws[wVerdict] == MC_MERGE_OK;
    uint32_t entries = 0, unknown = 0;
    for_each_line_start(a.B, a.n, p0, [&](uint32_t s) {
        if (a.B[s] == '#') return;
        uint32_t q = 0;
        if (!fold) {                                           // nothing changes but the claims of pass 1 are given back
            uint32_t p = s;
            if (parse_id(a, p, q) && q < a.capacity) a.owner[q] = kNone;
            return;
        }
        uint32_t hdrOff = 0, hdrLen = 0, listAt = 0;
        if (!parse_head(a, s, q, hdrOff, hdrLen, listAt) || q >= a.capacity) return;     // (cannot happen with the verdict OK)
        a.owner[q] = kNone;
        a.epoch[q] = a.fileSeq;
        uint32_t* h = a.hdr + 3ull * q;
        if (h[2] == 0) { h[0] = a.callNo; h[1] = hdrOff; h[2] = hdrLen; }
        uint2* L = a.lists + (uint64_t)q * a.maxCand;
        parse_list(a, listAt, [&](int64_t taxid, uint32_t hits) {
            const uint32_t x = taxon_of_id(a, taxid);
            if (!x) { ++unknown; return; }
            ++entries;
            insert_candidate(L, a.maxCand, make_uint2(x, hits), a.mergeBelow);
        });
    });
    entries = wave_sum_u32(entries); unknown = wave_sum_u32(unknown);
    if ((threadIdx.x & 63u) == 0) {                            // (sums: the same whatever the order)
        if (entries) { atomicAdd((unsigned long long*)&a.status[3], (unsigned long long)entries); atomicAdd(&a.counters[cEntries], (unsigned long long)entries); }
        if (unknown) { atomicAdd((unsigned long long*)&a.status[4], (unsigned long long)unknown); atomicAdd(&a.counters[cUnknown], (unsigned long long)unknown); }
    }
}

// ---- the vote: classify for candidates that carry a taxon (the lineage of a candidate is its taxon's row) --------------------------
struct MergeVoteArgs {
    const uint2* lists;                      // the store's row `first` and on
    const uint32_t* lin; const uint8_t* rank;    // the taxon table: lin[rank * numTaxa + row], the rank of each row
    mc_assignment* out;
    unsigned long long* assigned;            // MC_CLASSIFY_TALLY: the context's tallies (classify.hip): [kBins] reads per result rank
    unsigned long long* taxonCounts;         // ... and [numCounts] reads per taxon entry
    uint64_t n, numCounts;
    uint32_t maxCand, numTaxa, hitsMin;
    float hitsDiff;
    int highest;
};

template <bool TALLY>
__global__ __launch_bounds__(kBlock) void merge_vote_kernel(MergeVoteArgs a)
{
    __shared__ uint32_t binCount[kBins];
    if (TALLY) {
        if (threadIdx.x < kBins) binCount[threadIdx.x] = 0;
        __syncthreads();
    }
    const uint32_t nT = a.numTaxa;
    const uint64_t step = (uint64_t)gridDim.x * kBlock;
    for (uint64_t base = (uint64_t)blockIdx.x * kBlock; base < a.n; base += step) {      // (the same trips for every lane of a block)
        const uint64_t i = base + threadIdx.x;
        const bool active = i < a.n;
        const uint2* c = a.lists + (active ? i : 0) * a.maxCand;
        const uint2 top = active ? c[0] : make_uint2(0u, 0u);
        uint32_t taxon = 0, rank = MC_NUM_RANKS, voters = 0;
        if (top.y != 0 && top.y >= a.hitsMin && top.x != 0 && top.x <= nT) {
            int r = a.rank[top.x - 1];                                           // MC_NUM_RANKS: a taxon without a rank
            uint32_t t = top.x, v = 1;
            const float threshold = top.y > a.hitsMin ? (float)(top.y - a.hitsMin) * a.hitsDiff : 0.0f;
            for (uint32_t j = 1; j < a.maxCand; ++j) {
                const uint2 cj = c[j];
                if (cj.y == 0 || !((float)cj.y > threshold)) break;
                ++v;
                uint32_t l = 0;
                if (cj.x != 0 && cj.x <= nT)
                    for (; r < MC_NUM_RANKS; ++r) {
                        const uint32_t x = a.lin[(uint64_t)r * nT + (top.x - 1)];
                        if (x && x == a.lin[(uint64_t)r * nT + (cj.x - 1)]) { l = x; break; }
                    }
                t = l;
                if (!t || r > a.highest) { t = 0; break; }
            }
            if (t && r <= a.highest) { taxon = t; rank = (uint32_t)r; voters = v < 255u ? v : 255u; }
        }
        if (active) *reinterpret_cast<uint2*>(a.out + i) = make_uint2(taxon, rank | (voters << 8));
        if (TALLY) {                                                              // (sums: the same whatever the order)
            wave_add_by_key(rank, active, (int)kBins, [&](uint32_t k, uint32_t n) { atomicAdd(&binCount[k], n); });
            wave_add_by_key(taxon, active && taxon != 0 && taxon < a.numCounts, 8, [&](uint32_t k, uint32_t n) { atomicAdd(&a.taxonCounts[k], (unsigned long long)n); });
        }
    }
    if (TALLY) {
        __syncthreads();
        if (threadIdx.x < kBins && binCount[threadIdx.x]) atomicAdd(&a.assigned[threadIdx.x], (unsigned long long)binCount[threadIdx.x]);
    }
}

}  // namespace

namespace mcamd {

struct MergeResultsState {               // what the context keeps for mc_merge_results_*
    // mc_merge_results_set_taxids: the sorted ids with their taxon entries, and the taxon table rank-major
    int64_t* dIds = nullptr; uint32_t* dRows = nullptr; uint32_t* dLin = nullptr; uint8_t* dRank = nullptr;
    uint32_t numIds = 0;
    uint64_t tableVersion = ~0ull;       // ctx->taxonTableVersion the copies were made from
    // the store (mc_merge_results_begin / _reserve)
    uint2* dLists = nullptr; uint32_t* dHdr = nullptr; uint32_t* dOwner = nullptr; uint32_t* dEpoch = nullptr;
    unsigned long long* dCount = nullptr;
    uint64_t capacity = 0;
    uint32_t maxCand = 0, fileSeq = 0, callNo = 0;
    int32_t mergeBelow = 0;
    bool begun = false;
    unsigned long long* dCounters = nullptr;
    uint64_t calls = 0, bytes = 0;
    DevBuf stageIn, stageWs, stageOut;
    StatusStage status;                  // [8]
};

void free_merge_results_state(mc_ctx* ctx)
{
    if (!ctx->mergeResults) return;
    MergeResultsState& S = *ctx->mergeResults;
    for (void* p : {(void*)S.dIds, (void*)S.dRows, (void*)S.dLin, (void*)S.dRank, (void*)S.dLists, (void*)S.dHdr, (void*)S.dOwner, (void*)S.dEpoch, (void*)S.dCount,
                    (void*)S.dCounters, S.stageIn.p, S.stageWs.p, S.stageOut.p})
        if (p) (void)hipFree(p);
    free_status_stage(S.status);
    delete ctx->mergeResults;
    ctx->mergeResults = nullptr;
}

}  // namespace mcamd

namespace {

int ensure_merge_state(mc_ctx* ctx, MergeResultsState** out)
{
    if (!ctx->mergeResults) ctx->mergeResults = new MergeResultsState;
    MergeResultsState& S = *ctx->mergeResults;
    *out = &S;
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, cCounters * 8));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, cCounters * 8));
    }
    if (!S.dCount) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCount, 8));
        HIP_TRY(ctx, hipMemset(S.dCount, 0, 8));
    }
    return make_status_stage(ctx, S.status, 8);
}

void free_store(MergeResultsState& S)
{
    for (void* p : {(void*)S.dLists, (void*)S.dHdr, (void*)S.dOwner, (void*)S.dEpoch}) if (p) (void)hipFree(p);
    S.dLists = nullptr; S.dHdr = nullptr; S.dOwner = nullptr; S.dEpoch = nullptr;
    S.capacity = 0;
}

// a store of `capacity` queries that holds the first `keep` queries of the present one
int make_store(mc_ctx* ctx, MergeResultsState& S, uint64_t capacity, uint64_t keep)
{
    const uint64_t rows = std::max<uint64_t>(capacity, 1);
    uint2* lists = nullptr; uint32_t* hdr = nullptr; uint32_t* owner = nullptr; uint32_t* epoch = nullptr;
    auto release = [&] { for (void* p : {(void*)lists, (void*)hdr, (void*)owner, (void*)epoch}) if (p) (void)hipFree(p); };
    if (hipMalloc((void**)&lists, rows * S.maxCand * 8) != hipSuccess || hipMalloc((void**)&hdr, rows * 12) != hipSuccess ||
        hipMalloc((void**)&owner, rows * 4) != hipSuccess || hipMalloc((void**)&epoch, rows * 4) != hipSuccess) {
        (void)hipGetLastError();
        release();
        return fail(ctx, MC_ERR_NOMEM, "mc_merge_results: no device memory for " + std::to_string(rows * (S.maxCand * 8ull + 20)) + " bytes of lists");
    }
    hipError_t e = hipMemset(lists, 0, rows * S.maxCand * 8);
    if (e == hipSuccess) e = hipMemset(hdr, 0, rows * 12);
    if (e == hipSuccess) e = hipMemset(owner, 0xFF, rows * 4);
    if (e == hipSuccess) e = hipMemset(epoch, 0, rows * 4);
    if (e == hipSuccess && keep) e = hipMemcpy(lists, S.dLists, keep * S.maxCand * 8, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && keep) e = hipMemcpy(hdr, S.dHdr, keep * 12, hipMemcpyDeviceToDevice);
    if (e == hipSuccess && keep) e = hipMemcpy(epoch, S.dEpoch, keep * 4, hipMemcpyDeviceToDevice);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) { release(); return fail(ctx, MC_ERR_HIP, std::string("mc_merge_results: ") + hipGetErrorString(e)); }
    free_store(S);
    S.dLists = lists; S.dHdr = hdr; S.dOwner = owner; S.dEpoch = epoch; S.capacity = capacity;
    return MC_OK;
}

// the five passes of one range, nothing waited for
int enqueue_add(mc_ctx* ctx, MergeResultsState& S, const uint8_t* dBytes, uint32_t n, uint32_t tophitsColumn, uint64_t fileLines, bool cont,
                uint64_t* dStatus, void* ws, hipStream_t st)
{
    MergeArgs a{};
    a.B = dBytes; a.ws = (uint32_t*)ws; a.status = dStatus; a.counters = S.dCounters; a.count = S.dCount;
    a.lists = S.dLists; a.hdr = S.dHdr; a.owner = S.dOwner; a.epoch = S.dEpoch; a.ids = S.dIds; a.rows = S.dRows;
    a.capacity = S.capacity; a.fileLines = cont ? 0 : fileLines;
    a.n = n; a.numIds = S.numIds; a.tophitsColumn = tophitsColumn; a.maxCand = S.maxCand; a.cont = cont ? 1u : 0u;
    if (!cont) ++S.fileSeq;
    a.fileSeq = S.fileSeq; a.callNo = S.callNo++;
    a.mergeBelow = S.mergeBelow;
    const uint32_t tiles = tiles_of(n);
    HIP_TRY(ctx, hipMemsetAsync(ws, 0, kScratchBytes, st));
    {
        ScopedTimer timer(ctx, "merge_results_validate", st);
        hipLaunchKernelGGL(merge_validate_kernel, dim3(tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(merge_dups_kernel, dim3(tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(merge_verdict_kernel, dim3(1), dim3(64), 0, st, a);
    }
    {
        ScopedTimer timer(ctx, "merge_results_fold", st);
        hipLaunchKernelGGL(merge_cut_kernel, dim3(row_blocks(std::max<uint64_t>(S.capacity, 1), kBlock, kMaxBlocks)), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(merge_fold_kernel, dim3(tiles), dim3(kBlock), 0, st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    ++S.calls; S.bytes += n;
    return MC_OK;
}

// what every call needs of the context, after its own argument checks
int merge_state(mc_ctx* ctx, const char* who, bool needBegin, MergeResultsState** out)
{
    const std::string name = who;
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, name + ": the context has no device (mc_open_metadata)");
    if (!ctx->taxonTableSet) return fail(ctx, MC_ERR_STATE, name + ": the context has no taxon table (mc_set_taxon_table)");
    MergeResultsState* S = ctx->mergeResults;
    if (!S || !S->dIds || S->tableVersion != ctx->taxonTableVersion) return fail(ctx, MC_ERR_STATE, name + ": no taxids for the present taxon table (mc_merge_results_set_taxids)");
    if (needBegin && !S->begun) return fail(ctx, MC_ERR_STATE, name + ": no store (mc_merge_results_begin)");
    *out = S;
    return MC_OK;
}

}  // namespace

extern "C" {

const uint32_t mc_merge_results_tile = kTile;
const uint32_t mc_merge_results_max_candidates = kMaxCandidates;

uint64_t mc_merge_results_scratch_bytes(uint64_t nbytes) { (void)nbytes; return kScratchBytes; }

int mc_merge_results_set_taxids(mc_ctx* ctx, const int64_t* idOfRow, uint64_t numTaxa)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!idOfRow && numTaxa) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_set_taxids: no ids");
    if (!ctx->taxonTableSet) return fail(ctx, MC_ERR_STATE, "mc_merge_results_set_taxids: the context has no taxon table (mc_set_taxon_table)");
    if (numTaxa != ctx->taxonRank.size()) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_set_taxids: one id per row of the taxon table");
    std::vector<uint32_t> order((size_t)numTaxa);
    std::iota(order.begin(), order.end(), 0u);
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return idOfRow[x] < idOfRow[y]; });
    std::vector<int64_t> ids((size_t)numTaxa);
    std::vector<uint32_t> rows((size_t)numTaxa);
    for (size_t i = 0; i < order.size(); ++i) {
        ids[i] = idOfRow[order[i]]; rows[i] = order[i] + 1;
        if (i && ids[i] == ids[i - 1]) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_set_taxids: taxid " + std::to_string(ids[i]) + " names two rows");
    }
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_merge_results_set_taxids: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    MergeResultsState* S = nullptr;
    if (const int rc = ensure_merge_state(ctx, &S)) return rc;
    HIP_TRY(ctx, hipDeviceSynchronize());                       // (merges that still run finish with the old tables)
    for (void* p : {(void*)S->dIds, (void*)S->dRows, (void*)S->dLin, (void*)S->dRank}) if (p) (void)hipFree(p);
    S->dIds = nullptr; S->dRows = nullptr; S->dLin = nullptr; S->dRank = nullptr;
    const uint64_t nt = numTaxa, rowsAlloc = std::max<uint64_t>(nt, 1);
    std::vector<uint32_t> planes(rowsAlloc * MC_NUM_RANKS, 0u);
    for (uint64_t t = 0; t < nt; ++t)
        for (uint32_t r = 0; r < MC_NUM_RANKS; ++r) planes[(uint64_t)r * nt + t] = ctx->taxonLin[t * MC_NUM_RANKS + r];
    HIP_TRY(ctx, hipMalloc((void**)&S->dIds, rowsAlloc * 8));
    HIP_TRY(ctx, hipMalloc((void**)&S->dRows, rowsAlloc * 4));
    HIP_TRY(ctx, hipMalloc((void**)&S->dLin, planes.size() * 4));
    HIP_TRY(ctx, hipMalloc((void**)&S->dRank, rowsAlloc));
    if (nt) {
        HIP_TRY(ctx, hipMemcpy(S->dIds, ids.data(), nt * 8, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(S->dRows, rows.data(), nt * 4, hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(S->dRank, ctx->taxonRank.data(), nt, hipMemcpyHostToDevice));
    }
    HIP_TRY(ctx, hipMemcpy(S->dLin, planes.data(), planes.size() * 4, hipMemcpyHostToDevice));
    S->numIds = (uint32_t)nt;
    S->tableVersion = ctx->taxonTableVersion;
    return MC_OK;
}

int mc_merge_results_begin(mc_ctx* ctx, uint64_t capacityQueries, uint32_t maxCandidates, int32_t mergeBelow)
{
    if (!ctx) return MC_ERR_INVALID;
    if (maxCandidates == 0) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_begin: max_candidates must be at least 1");
    if (capacityQueries > kMaxCapacity) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_begin: more than 2^32 - 1 queries");
    if (maxCandidates > kMaxCandidates) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_merge_results_begin: more than " + std::to_string(kMaxCandidates) + " candidates per query");
    MergeResultsState* S = nullptr;
    if (const int rc = merge_state(ctx, "mc_merge_results_begin", false, &S)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    S->begun = false;
    S->maxCand = maxCandidates; S->mergeBelow = mergeBelow;
    if (const int rc = make_store(ctx, *S, capacityQueries, 0)) return rc;
    HIP_TRY(ctx, hipMemset(S->dCount, 0, 8));
    S->fileSeq = 0; S->callNo = 0;
    S->begun = true;
    return MC_OK;
}

int mc_merge_results_reserve(mc_ctx* ctx, uint64_t capacityQueries)
{
    if (!ctx) return MC_ERR_INVALID;
    if (capacityQueries > kMaxCapacity) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_reserve: more than 2^32 - 1 queries");
    MergeResultsState* S = nullptr;
    if (const int rc = merge_state(ctx, "mc_merge_results_reserve", true, &S)) return rc;
    if (capacityQueries <= S->capacity) return MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipDeviceSynchronize());
    return make_store(ctx, *S, capacityQueries, S->capacity);
}

int mc_merge_results_add(mc_ctx* ctx, const char* bytes, uint64_t nbytes, uint32_t tophitsColumn, uint64_t fileLines, int flags, uint64_t status[8],
                         void* workspace, uint64_t workspaceBytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~(MC_MERGE_HOST | MC_MERGE_CONTINUE)) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: unknown flag");
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: no bytes");
    if (nbytes > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: more than 2^31 bytes in one range");
    if (tophitsColumn == 0) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: tophits_column counts from 1");
    if (!status) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: no status");
    const bool host = (flags & MC_MERGE_HOST) != 0, cont = (flags & MC_MERGE_CONTINUE) != 0;
    if (!host) {
        if (!workspace || workspaceBytes < kScratchBytes) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: the workspace is smaller than mc_merge_results_scratch_bytes");
        if (((uintptr_t)bytes | (uintptr_t)workspace) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: device arrays must be aligned (bytes, workspace: 16 bytes)");
        if ((uintptr_t)status & 7u) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_add: device arrays must be aligned (status: 8 bytes)");
    }
    // ... then state
    MergeResultsState* S = nullptr;
    int rc = merge_state(ctx, "mc_merge_results_add", true, &S);
    if (rc) return rc;
    if (cont && S->fileSeq == 0) return fail(ctx, MC_ERR_STATE, "mc_merge_results_add: MC_MERGE_CONTINUE without a file to continue");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (!host) return enqueue_add(ctx, *S, (const uint8_t*)bytes, (uint32_t)nbytes, tophitsColumn, fileLines, cont, status, workspace, st);
    if ((rc = grow(ctx, S->stageWs, kScratchBytes)) != MC_OK || (rc = stage_bytes(ctx, S->stageIn, bytes, nbytes, st)) != MC_OK) return rc;
    if ((rc = enqueue_add(ctx, *S, (const uint8_t*)S->stageIn.p, (uint32_t)nbytes, tophitsColumn, fileLines, cont, (uint64_t*)S->status.dev.p, S->stageWs.p, st)) != MC_OK) return rc;
    return read_status(ctx, S->status, 8, status, st);
}

int mc_merge_results_lists(mc_ctx* ctx, uint64_t first, uint64_t count, int flags, mc_taxon_candidate* lists, uint32_t* headerPlace, uint64_t* numQueries, void* streamv)
{
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_MERGE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_lists: unknown flag");
    if (count > 0 && !lists && !headerPlace) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_lists: null arrays");
    const bool host = (flags & MC_MERGE_HOST) != 0;
    if (!host && (((uintptr_t)lists | (uintptr_t)numQueries) & 7u)) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_lists: device arrays must be aligned (lists, num_queries: 8 bytes)");
    if (!host && ((uintptr_t)headerPlace & 3u)) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_lists: device arrays must be aligned (header_place: 4 bytes)");
    MergeResultsState* S = nullptr;
    if (const int rc = merge_state(ctx, "mc_merge_results_lists", true, &S)) return rc;
    if (first > S->capacity || count > S->capacity - first) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_lists: first + count beyond the store's capacity");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    if (count && lists) HIP_TRY(ctx, hipMemcpyAsync(lists, S->dLists + first * S->maxCand, count * S->maxCand * 8, kind, st));
    if (count && headerPlace) HIP_TRY(ctx, hipMemcpyAsync(headerPlace, S->dHdr + 3 * first, count * 12, kind, st));
    if (numQueries) HIP_TRY(ctx, hipMemcpyAsync(numQueries, S->dCount, 8, kind, st));
    if (host) HIP_TRY(ctx, hipStreamSynchronize(st));
    return MC_OK;
}

int mc_merge_results_classify(mc_ctx* ctx, const mc_classify_options* o, int flags, uint64_t first, uint64_t count, mc_assignment* out, void* streamv)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!o) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: no options");
    if (flags & ~(MC_CLASSIFY_HOST | MC_CLASSIFY_TALLY)) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: unknown flag");
    if (o->lowest_rank < 0 || o->lowest_rank >= MC_NUM_RANKS || o->highest_rank < 0 || o->highest_rank >= MC_NUM_RANKS)
        return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: ranks must be 0 .. MC_NUM_RANKS - 1");
    if (o->lowest_rank > o->highest_rank) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: lowest_rank above highest_rank");
    if (!std::isfinite(o->hits_diff) || o->hits_diff < 0.0f) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: hits_diff must be finite and not negative");
    if (count > 0 && !out) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: null array");
    const bool host = (flags & MC_CLASSIFY_HOST) != 0;
    if (!host && ((uintptr_t)out & 7u)) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: device arrays must be 8-byte aligned");
    MergeResultsState* S = nullptr;
    int rc = merge_state(ctx, "mc_merge_results_classify", true, &S);
    if (rc) return rc;
    if (first > S->capacity || count > S->capacity - first) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_classify: first + count beyond the store's capacity");
    if (count == 0) return MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (host && (rc = grow(ctx, S->stageOut, count * sizeof(mc_assignment))) != MC_OK) return rc;
    MergeVoteArgs a{};
    const bool tally = (flags & MC_CLASSIFY_TALLY) != 0;
    if (tally) {                                                                // the counters mc_classify_tally reads
        ClassifyState* C = nullptr;
        if ((rc = ensure_classify_state(ctx, &C)) != MC_OK) return rc;
        if (C->numCounts < (uint64_t)S->numIds + 1) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_merge_results_classify: the tallies are sized by the lineage table, which names fewer taxa than the taxon table");
        a.assigned = C->dTally; a.taxonCounts = C->dTally + kBins; a.numCounts = C->numCounts;
    }
    a.lists = S->dLists + first * S->maxCand; a.lin = S->dLin; a.rank = S->dRank;
    a.out = host ? (mc_assignment*)S->stageOut.p : out;
    a.n = count; a.maxCand = S->maxCand; a.numTaxa = S->numIds; a.hitsMin = o->hits_min; a.hitsDiff = o->hits_diff; a.highest = o->highest_rank;
    {
        ScopedTimer timer(ctx, "merge_results_vote", st);
        const dim3 grid(row_blocks(count, kBlock, kMaxBlocks));
        if (tally) hipLaunchKernelGGL(merge_vote_kernel<true>, grid, dim3(kBlock), 0, st, a);
        else hipLaunchKernelGGL(merge_vote_kernel<false>, grid, dim3(kBlock), 0, st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    if (host) {
        HIP_TRY(ctx, hipMemcpyAsync(out, S->stageOut.p, count * sizeof(mc_assignment), hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return MC_OK;
}

int mc_merge_results_stats(mc_ctx* ctx, uint64_t stats[6])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_merge_results_stats: no place for the counters");
    for (int i = 0; i < 6; ++i) stats[i] = 0;
    MergeResultsState* S = ctx->mergeResults;
    if (!S) return MC_OK;
    stats[0] = S->calls; stats[1] = S->bytes;
    if (S->dCounters) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        unsigned long long c[cCounters];
        HIP_TRY(ctx, hipMemcpy(c, S->dCounters, sizeof c, hipMemcpyDeviceToHost));
        stats[2] = c[cLines]; stats[3] = c[cEntries]; stats[4] = c[cUnknown]; stats[5] = c[cRefused];
    }
    return MC_OK;
}

void mc_merge_results_end(mc_ctx* ctx)
{
    if (!ctx || !ctx->mergeResults) return;
    MergeResultsState& S = *ctx->mergeResults;
    if (ctx->stream) { (void)hipSetDevice(ctx->device); (void)hipDeviceSynchronize(); }
    free_store(S);
    S.begun = false;
}

}  // extern "C"
