// metacache_amd/csrc/rows_common.h -- what the consumers of candidate rows (classify.hip, coverage.hip, target_hits.hip) and of their
// assignments (evaluate.hip) share with each other and with context.cpp: the staging of host arrays, the drain before a readback, the
// kernel timer, and -- on the device -- the taxon-of-a-target rule and the per-key wave sum of the tallies.  The wave reductions they use are
// device_common.h's.  The MC_*_HOST forms of the byte passes and of inflate.hip take the staged input bytes (stage_bytes) and the staged
// status (StatusStage, read_status) from here.  Internal.
#pragma once

#include "context.h"

#include <algorithm>
#include <cstring>

#ifdef __HIPCC__
#include "device_common.h"
#endif

namespace mcamd {

// ---- host ------------------------------------------------------------------------------------------
constexpr uint64_t kStagePieceBytes = (64ull << 20);            // MC_*_HOST arrays go to the device in pieces of at most this many bytes of candidates
constexpr size_t kCounterPairBytes = 2 * sizeof(unsigned long long);   // the two 64-bit device counters of mc_coverage_* and of mc_target_hits_*

inline uint32_t row_blocks(uint64_t n, uint32_t block, uint32_t maxBlocks) { return (uint32_t)std::min<uint64_t>((n + block - 1) / block, maxBlocks); }
inline bool ranges_overlap(uintptr_t a0, uintptr_t a1, uintptr_t b0, uintptr_t b1) { return a0 < b1 && b0 < a1; }

// exact size, grow-only: a staging buffer is as large as the largest piece it has held
inline int grow(mc_ctx* ctx, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return MC_OK;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    HIP_TRY(ctx, hipMalloc(&b.p, bytes));
    b.cap = bytes;
    return MC_OK;
}

// ---- the MC_*_HOST forms: the input bytes up, the status words back.  The caller holds whatever mutex guards its staging buffers -----------
// the status of a call as its kernels write it (dev) and the pinned words the host reads it through
struct StatusStage { DevBuf dev; uint64_t* pinned = nullptr; };

// made once, for the largest status the owner reads (`words` 64-bit words); a second call changes nothing
inline int make_status_stage(mc_ctx* ctx, StatusStage& s, size_t words)
{
    if (const int rc = grow(ctx, s.dev, words * 8)) return rc;
    if (!s.pinned) HIP_TRY(ctx, hipHostMalloc((void**)&s.pinned, words * 8));
    return MC_OK;
}
inline void free_status_stage(StatusStage& s)
{
    if (s.dev.p) (void)hipFree(s.dev.p);
    if (s.pinned) (void)hipHostFree(s.pinned);
    s = StatusStage{};
}

// what has been enqueued on st is waited for and `words` status words are left in out; from: where they lie on the device (null: s.dev)
inline int read_status(mc_ctx* ctx, StatusStage& s, size_t words, uint64_t* out, hipStream_t st, const uint64_t* from = nullptr)
{
    HIP_TRY(ctx, hipMemcpyAsync(s.pinned, from ? from : s.dev.p, words * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    std::memcpy(out, s.pinned, words * 8);
    return MC_OK;
}

// n host bytes into stageIn, which is grown to whole 16-byte loads; the copy is enqueued on st
inline int stage_bytes(mc_ctx* ctx, DevBuf& stageIn, const void* bytes, uint64_t n, hipStream_t st)
{
    if (const int rc = grow(ctx, stageIn, (n + 15) / 16 * 16)) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(stageIn.p, bytes, n, hipMemcpyHostToDevice, st));
    return MC_OK;
}

// rows of the largest piece of n rows of `stride` entries (what a caller sizes its own staging buffers by)
inline uint32_t staged_piece_rows(uint32_t n, uint32_t stride)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(n, kStagePieceBytes / ((uint64_t)stride * sizeof(mc_candidate))));
}
// ... and its bytes: the size of stageIn
inline uint64_t staged_piece_bytes(uint32_t n, uint32_t stride) { return (uint64_t)staged_piece_rows(n, stride) * stride * sizeof(mc_candidate); }

// the host array rows[n * stride] through stageIn, piece by piece: the copy of a piece is enqueued on st, body(dRows, done, m) enqueues
// what is to happen to the m rows that begin at row `done` and now lie at dRows, st is drained.  body returns an MC_* code; the first
// that is not MC_OK ends the loop.  The caller holds the mutex of its staging buffers.
template <class Fn>
int for_each_staged_piece(mc_ctx* ctx, hipStream_t st, DevBuf& stageIn, const mc_candidate* rows, uint32_t n, uint32_t stride, Fn&& body)
{
    const uint64_t perRow = (uint64_t)stride * sizeof(mc_candidate);
    const uint32_t piece = staged_piece_rows(n, stride);
    if (const int rc = grow(ctx, stageIn, staged_piece_bytes(n, stride))) return rc;      // (nothing to do where the caller has grown it ahead of its own buffers)
    for (uint32_t done = 0; done < n; done += piece) {
        const uint32_t m = std::min(piece, n - done);
        HIP_TRY(ctx, hipMemcpyAsync(stageIn.p, rows + (uint64_t)done * stride, m * perRow, hipMemcpyHostToDevice, st));
        if (const int rc = body((const mc_candidate*)stageIn.p, done, m)) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(st));
    }
    return MC_OK;
}

// what the query entry points have enqueued on the context's own streams is through (before a readback of what their kernels add to)
inline int drain_query_streams(mc_ctx* ctx)
{
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->pipe1.stream) HIP_TRY(ctx, hipStreamSynchronize(ctx->pipe1.stream));
    return MC_OK;
}

// ---- timing (mc_timing_enable): a kernel sequence between two events of the context's pool, read by mc_timing_get under `name` -----
inline hipEvent_t get_event(mc_ctx* ctx)          // under ctx->timerMtx
{
    if (!ctx->eventPool.empty()) { hipEvent_t e = ctx->eventPool.back(); ctx->eventPool.pop_back(); return e; }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

struct ScopedTimer {
    mc_ctx* ctx; const char* name; hipStream_t st; hipEvent_t a = nullptr, b = nullptr;
    ScopedTimer(mc_ctx* c, const char* n, hipStream_t s) : ctx(c), name(n), st(s)
    {
        if (ctx->timing) { std::lock_guard<std::mutex> l(ctx->timerMtx); a = get_event(ctx); b = get_event(ctx); (void)hipEventRecord(a, st); }
    }
    ~ScopedTimer()
    {
        if (a) { std::lock_guard<std::mutex> l(ctx->timerMtx); (void)hipEventRecord(b, st); ctx->timers[name].pending.emplace_back(a, b); }
    }
};

// ---- device ----------------------------------------------------------------------------------------
#ifdef __HIPCC__

// tax(target) of the reference (classification.cpp:146-189, matches_per_target::insert): the lineage slot `lowest` itself for sequence
// level (rank 0), else the first slot that is filled from `lowest` upwards.  lin: the rank-major lineage planes of classify.hip.
// Returns the taxon (0: none) and leaves the rank the walk stopped on in `rank`.
__device__ __forceinline__ uint32_t taxon_of_target(const uint32_t* lin, uint32_t linTargets, uint32_t tgt, int lowest, int& rank)
{
    int r = lowest;
    uint32_t t = lin[(uint64_t)r * linTargets + tgt];
    if (lowest > 0) while (!t && ++r < MC_NUM_RANKS) t = lin[(uint64_t)r * linTargets + tgt];
    rank = r;
    return t;
}

// adds, for every distinct key among the wave's active lanes, the number of lanes that hold it: `rounds` keys are counted across the
// wave (one add each, by the first lane that holds the key), the lanes left after that add 1 each.  All lanes of the wave call this.
template <class Add>
__device__ __forceinline__ void wave_add_by_key(uint32_t key, bool active, int rounds, Add add)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long todo = __ballot(active);
    for (int r = 0; r < rounds && todo; ++r) {
        const int leader = __ffsll(todo) - 1;
        const uint32_t k = (uint32_t)__shfl((int)key, leader);
        const unsigned long long same = __ballot(active && key == k);
        if (lane == (uint32_t)leader) add(k, (uint32_t)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) add(key, 1u);
}

#endif  // __HIPCC__

}  // namespace mcamd
