// metacache_amd/csrc/inflate.hip -- mc_bgzf_index / mc_inflate_blocks / mc_inflate_stats: the members of a BGZF file inflated on the
// device.  The member rule and the block rule are those of include/metacache_amd.h; the host walk is bgzf_rules.h.
//
// A deflate stream is a chain -- where a symbol starts depends on the one before it -- so the unit of parallelism is the BGZF member:
// ONE WAVE PER MEMBER, kWaves members per workgroup.  Inside a wave
//   * the bit reader (Bits) and everything the chain decides are wave-uniform: every lane runs the same decode, the values go through
//     readfirstlane and so live in scalar registers;
//   * the 64 lanes share the parallel work: the canonical tables of a code set (build_code: one ballot per length and 64 symbols, the
//     fast table by 64 lanes), runs of code lengths, stored copies, match copies (a copy with distance < length repeats its period:
//     out[pos + i] = out[pos - d + i % d]; distance 1 is a fill) and the CRC-32;
//   * literals wait in one register per lane (position p in lane p % 64) and leave as one 64-byte store; a match or a stored block
//     flushes them first, and then reads what the wave itself wrote to `out` (a wave's memory operations are performed in order; the
//     wavefront fence keeps the compiler from moving them).
// The tables live in LDS per wave (WaveTables, 3 584 bytes); nothing per lane is indexed at run time, so there is no scratch.
// EVERY LOOP IS BOUNDED by what is left of the input bits or of the output slice: Bits::left counts the payload's unread bits and every
// consume checks it; every store is checked against the row's out_len before it is made.  A hostile stream ends with a reason.
// The CRC is a pass of its own behind the decode: lane i folds the i-th of 64 equal chunks (the data padded IN FRONT, where a zero
// register stays zero) through a 256-entry table in LDS, and the lanes' registers are joined with the shift operator x^(8 * chunk) mod P.
// The verdict: every bad row sends (row << 8 | reason) into an atomic minimum in status[1], inflate_verdict_kernel behind the blocks turns
// it into the four words.  A minimum does not depend on the order of its operands: the same input gives the same status.
// The decoder itself -- Bits, build_code, inflate_stream, wave_crc32, the fence -- is inflate_wave.h, which inflate_streams.hip (whole gzip
// files, 7n) includes too; this file keeps the BGZF rows, their kernel and the call.
// Plain HIP C++; no inline assembly.
#include "inflate_wave.h"
#include "bgzf_rules.h"

#include <atomic>
#include <cstring>
#include <vector>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kWaves = kBlock / 64;
constexpr unsigned long long kNoKey = ~0ull;
constexpr uint32_t kOverflowCode = 255;                            // the "reason" of a row that does not fit out_capacity
constexpr uint64_t kDefaultStageBytes = 64ull << 20;

struct InflateArgs {
    const uint8_t* B; uint64_t nbytes;
    const mc_bgzf_block* blocks; uint64_t numBlocks;
    uint8_t* out; uint64_t outCap;
    unsigned long long* status;
    unsigned long long* counters;     // the context's: bytes out of accepted calls, calls refused
};

__global__ void inflate_begin_kernel(InflateArgs a)
{
    a.status[0] = 0; a.status[1] = kNoKey; a.status[2] = 0; a.status[3] = 0;
}

__global__ __launch_bounds__(kBlock) void inflate_blocks_kernel(InflateArgs a)
{
    __shared__ uint32_t crcTab[256];
    __shared__ WaveTables tabs[kWaves];
    {
        uint32_t c = threadIdx.x;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        crcTab[threadIdx.x] = c;
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wave = uni(threadIdx.x >> 6);
    const uint64_t blk = (uint64_t)blockIdx.x * kWaves + wave;
    if (blk >= a.numBlocks) return;
    const mc_bgzf_block* row = a.blocks + blk;
    const uint64_t inOff = uni64(row->in_off), outOff = uni64(row->out_off);
    const uint32_t inLen = uni(row->in_len), outLen = uni(row->out_len);
    uint32_t code = 0;
    if (outOff > a.outCap || a.outCap - outOff < outLen) code = kOverflowCode;            // writes nothing
    else if (inOff > a.nbytes || a.nbytes - inOff < inLen || inLen < 20u) code = MC_INFLATE_R_INPUT;   // loads nothing
    else {
        const uint8_t* M = a.B + inOff;
        const uint32_t xlen = uni((uint32_t)M[10] | ((uint32_t)M[11] << 8));
        if (inLen < 12u + xlen + 8u) code = MC_INFLATE_R_INPUT;
        else {
            const uint32_t crcWant = uni(load_u32(M + inLen - 8u)), isize = uni(load_u32(M + inLen - 4u));
            Out o{a.out + outOff, 0u, 0u, outLen, 0u};
            code = inflate_stream(a.B, inOff + 12u + xlen, inLen - 20u - xlen, inOff + inLen, o, tabs[wave], lane);
            if (!code && o.pos != isize) code = o.pos < isize ? MC_INFLATE_R_SHORT : MC_INFLATE_R_OVER;
            if (!code) {
                wave_order();
                if (wave_crc32(o.dst, o.pos, crcTab, lane) != crcWant) code = MC_INFLATE_R_CRC;
            }
        }
    }
    if (lane == 0) {
        if (code != kOverflowCode) atomicMax(&a.status[3], (unsigned long long)(outOff + outLen));
        if (code) atomicMin(&a.status[1], (unsigned long long)((blk << 8) | code));
    }
}

__global__ void inflate_verdict_kernel(InflateArgs a)
{
    const unsigned long long key = a.status[1], covered = a.status[3];
    if (key == kNoKey) {
        a.status[0] = MC_INFLATE_OK; a.status[1] = 0; a.status[2] = 0;
        atomicAdd(&a.counters[0], covered);                  // (statistics, no position)
    } else {
        const uint32_t code = (uint32_t)(key & 255u);
        a.status[0] = code == kOverflowCode ? MC_INFLATE_OVERFLOW : MC_INFLATE_CORRUPT;
        a.status[1] = key >> 8;
        a.status[2] = code == kOverflowCode ? 0u : code;
        atomicAdd(&a.counters[1], 1ull);
    }
}

}  // namespace

namespace mcamd {

void free_inflate_state(mc_ctx* ctx)
{
    if (!ctx->inflate) return;
    InflateState& S = *ctx->inflate;
    if (S.dCounters) (void)hipFree(S.dCounters);
    free_status_stage(S.status);
    for (DevBuf* b : {&S.stageIn, &S.stageRows, &S.stageOut, &S.stageResults})
        if (b->p) (void)hipFree(b->p);
    delete ctx->inflate;
    ctx->inflate = nullptr;
}

}  // namespace mcamd

namespace {

// the device form: three launches, nothing waited for
int enqueue_inflate(mc_ctx* ctx, InflateState& S, const uint8_t* dBytes, uint64_t nbytes, const mc_bgzf_block* dBlocks, uint64_t numBlocks,
                    uint8_t* dOut, uint64_t outCap, uint64_t* dStatus, hipStream_t st)
{
    InflateArgs a{dBytes, nbytes, dBlocks, numBlocks, dOut, outCap, (unsigned long long*)dStatus, S.dCounters};
    ScopedTimer timer(ctx, "inflate_blocks", st);
    hipLaunchKernelGGL(inflate_begin_kernel, dim3(1), dim3(1), 0, st, a);
    if (numBlocks) hipLaunchKernelGGL(inflate_blocks_kernel, dim3((uint32_t)((numBlocks + kWaves - 1) / kWaves)), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(inflate_verdict_kernel, dim3(1), dim3(1), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

}  // namespace

extern "C" {

int mc_bgzf_index(const uint8_t* bytes, uint64_t nbytes, mc_bgzf_block* blocks, uint64_t capacity, uint64_t info[4])
{
    if (!info) return fail(nullptr, MC_ERR_INVALID, "mc_bgzf_index: no place for info");
    if (!bytes && nbytes > 0) return fail(nullptr, MC_ERR_INVALID, "mc_bgzf_index: no bytes");
    bgzf_index(bytes, nbytes, blocks, capacity, info);
    return MC_OK;
}

int mc_inflate_blocks(mc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, const mc_bgzf_block* blocks, uint64_t num_blocks, int flags,
                      uint8_t* out, uint64_t out_capacity, uint64_t status[4], void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_INFLATE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: unknown flag");
    if (!status) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: no status");
    if (num_blocks > 0 && (!bytes || !blocks)) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: null array");
    if (num_blocks > (1ull << 33)) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: more than 2^33 rows in one call");
    if (out_capacity > 0 && !out) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: a capacity without its array");
    const bool host = (flags & MC_INFLATE_HOST) != 0;
    if (bytes && out && ranges_overlap((uintptr_t)bytes, (uintptr_t)bytes + nbytes, (uintptr_t)out, (uintptr_t)out + out_capacity))
        return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: out overlaps bytes");
    if (host) {
        if (!bgzf_rows_ok(blocks, num_blocks, nbytes)) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: the rows are not non-decreasing, non-overlapping slices inside nbytes of at most 65536 bytes out");
    } else {
        if (((uintptr_t)bytes | (uintptr_t)out) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: device arrays must be aligned (bytes, out: 16 bytes)");
        if (((uintptr_t)blocks | (uintptr_t)status) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_inflate_blocks: device arrays must be aligned (blocks, status: 8 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_inflate_blocks: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    InflateState* S = nullptr;
    int rc = ensure_inflate_state(ctx, &S);
    if (rc) return rc;
    ++S->calls; S->bytesIn += nbytes;
    if (!host) return enqueue_inflate(ctx, *S, bytes, nbytes, blocks, num_blocks, out, out_capacity, status, st);
    // host arrays: pieces of whole members through the staging buffers, one caller at a time.  A piece's rows are moved to the piece's
    // own origin (in_off from a multiple of 16, out_off from its first slice); its out leaves the device only with MC_INFLATE_OK
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t pieceIn = ctx->inflateStageBytes ? ctx->inflateStageBytes : kDefaultStageBytes, pieceOut = 4 * pieceIn;
    std::vector<mc_bgzf_block> rows;
    uint64_t covered = 0, piece[4];                                              // piece: the status of one piece
    for (uint64_t i = 0; i < num_blocks;) {
        const uint64_t inBase = blocks[i].in_off & ~15ull, outBase = blocks[i].out_off;
        uint64_t j = i, inEnd = inBase, outEnd = outBase;
        rows.clear();
        for (; j < num_blocks; ++j) {
            const mc_bgzf_block& r = blocks[j];
            if (j > i && (r.in_off + r.in_len - inBase > pieceIn || r.out_off + r.out_len - outBase > pieceOut)) break;
            inEnd = r.in_off + r.in_len; outEnd = r.out_off + r.out_len;
            rows.push_back({r.in_off - inBase, r.out_off - outBase, r.in_len, r.out_len});
        }
        const uint64_t inSpan = inEnd - inBase, outSpan = outEnd - outBase;
        const uint64_t cap = out_capacity > outBase ? std::min(out_capacity - outBase, outSpan) : 0;
        if ((rc = grow(ctx, S->stageIn, std::max<uint64_t>((inSpan + 15) / 16 * 16, 16))) != MC_OK || (rc = grow(ctx, S->stageOut, std::max<uint64_t>(outSpan, 16))) != MC_OK ||
            (rc = grow(ctx, S->stageRows, rows.size() * sizeof(mc_bgzf_block))) != MC_OK) return rc;
        if (inSpan) HIP_TRY(ctx, hipMemcpyAsync(S->stageIn.p, bytes + inBase, inSpan, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(S->stageRows.p, rows.data(), rows.size() * sizeof(mc_bgzf_block), hipMemcpyHostToDevice, st));
        if ((rc = enqueue_inflate(ctx, *S, (const uint8_t*)S->stageIn.p, inSpan, (const mc_bgzf_block*)S->stageRows.p, rows.size(), (uint8_t*)S->stageOut.p, cap,
                                  (uint64_t*)S->status.dev.p, st)) != MC_OK) return rc;
        if ((rc = read_status(ctx, S->status, 4, piece, st)) != MC_OK) return rc;
        covered = std::max(covered, outBase + piece[3]);
        if (piece[0] != MC_INFLATE_OK) {
            status[0] = piece[0]; status[1] = i + piece[1]; status[2] = piece[2]; status[3] = covered;
            return MC_OK;
        }
        // back: one copy per run of slices that touch (an indexed file is one run)
        for (size_t a = 0; a < rows.size();) {
            size_t e = a + 1;
            while (e < rows.size() && rows[e].out_off == rows[e - 1].out_off + rows[e - 1].out_len) ++e;
            const uint64_t from = rows[a].out_off, len = rows[e - 1].out_off + rows[e - 1].out_len - from;
            if (len) HIP_TRY(ctx, hipMemcpyAsync(out + outBase + from, (const uint8_t*)S->stageOut.p + from, len, hipMemcpyDeviceToHost, st));
            a = e;
        }
        HIP_TRY(ctx, hipStreamSynchronize(st));
        i = j;
    }
    status[0] = MC_INFLATE_OK; status[1] = 0; status[2] = 0; status[3] = covered;
    return MC_OK;
}

int mc_inflate_stats(mc_ctx* ctx, uint64_t stats[4])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_inflate_stats: no place for the counters");
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    InflateState* S = nullptr;
    { std::lock_guard<std::mutex> lock(ctx->inflateMtx); S = ctx->inflate; }
    if (!S) return MC_OK;
    stats[0] = S->calls; stats[1] = S->bytesIn;
    if (S->dCounters) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        unsigned long long c[2];
        HIP_TRY(ctx, hipMemcpy(c, S->dCounters, sizeof c, hipMemcpyDeviceToHost));
        stats[2] = c[0]; stats[3] = c[1];
    }
    return MC_OK;
}

}  // extern "C"
