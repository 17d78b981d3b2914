// metacache_amd/csrc/inflate_streams.hip -- mc_gzip_hint / mc_inflate_streams / mc_inflate_streams_stats: whole gzip files inflated on the
// device.  The stream rule is that of include/metacache_amd.h; the host header walk is gzip_rules.h; the decoder is
// inflate_wave.h, shared with inflate.hip.
//
// One deflate stream is a chain, so the unit of parallelism is the FILE: ONE WAVE PER ROW, and ONE WAVE PER WORKGROUP.  A row may be
// megabytes long; a workgroup of four waves would live as long as its longest row and hold the LDS of the three that are done.
// What this file adds to the decoder:
//   * the header walk (gzip_header_wave): wave-uniform, every byte access checked against the row's end first; FNAME and FCOMMENT are a
//     search for a zero byte, 64 bytes per round with one ballot;
//   * the chain: a member's input is bounded by the row's end minus 8, the stream says where it ends, the trailer is read at the next
//     byte behind it and the next member, if bytes remain, starts behind the trailer;
//   * per-MEMBER state: every member gets an Out of its own that begins at the member's first output byte, so the decoder's
//     "distance > produced" check is against the member's own count -- a second member starts with an empty history -- and the CRC and
//     ISIZE are the member's;
//   * the CRC-32 in SEGMENTS of kCrcSegment = 16 KiB (wave_crc32_segments): lane i folds the i-th 256 bytes of the segment, the lanes
//     are joined with the shift operator, and the joined register starts lane 0 of the next segment.  The wave so walks 16 KiB of
//     adjoining memory at a time -- two 128-byte lines per lane -- instead of 64 places megabytes apart, and pays one multiplication
//     mod P per 256 table steps.  The rest behind the last whole segment is folded as 7j folds a member.
// EVERY LOOP IS BOUNDED, the bound beside it.  A hostile row ends with a reason.  Every store is the decoder's and is checked against the
// row's out_cap first; a row whose slice is not inside out_capacity never reaches the decoder.
// The verdict: lane 0 writes results[row]; a refused row sends (row << 8 | reason) into an atomic minimum, an accepted one counts itself;
// streams_verdict_kernel behind the rows turns that into the four words.
// Plain HIP C++; no inline assembly.
#include "inflate_wave.h"
#include "gzip_rules.h"

#include <cstring>
#include <vector>

using namespace mcamd;

namespace {

constexpr uint32_t kStreamBlock = 64;                              // one wave
constexpr uint32_t kCrcSegment = 16384, kCrcPerLane = kCrcSegment / 64;
constexpr unsigned long long kNoStreamKey = ~0ull;
constexpr uint64_t kDefaultStreamStageBytes = 64ull << 20;
constexpr uint64_t kMaxStreamRows = 1ull << 30;

struct StreamArgs {
    const uint8_t* B; uint64_t nbytes;
    const mc_gzip_stream* rows; uint64_t numRows;
    uint8_t* out; uint64_t outCap;
    mc_gzip_result* results;
    unsigned long long* status;
    unsigned long long* counters;     // the context's [2], [3]: bytes out of accepted rows, rows refused
};

// the header of the member at M[p], p < n = the row's length: 0 and the offset of its deflate stream in `pay`, or the reason.  The checks
// and their order are gzip_rules.h's gzip_header.  Wave-uniform
__device__ uint32_t gzip_header_wave(const uint8_t* M, uint32_t n, uint32_t p, bool first, uint32_t lane, uint32_t& pay)
{
    if (n - p < 2u || uni(M[p]) != 0x1fu || uni(M[p + 1u]) != 0x8bu) return first ? MC_INFLATE_R_HEADER : MC_INFLATE_R_TRAILING;
    if (n - p < 10u) return MC_INFLATE_R_HEADER;
    if (uni(M[p + 2u]) != 8u) return MC_INFLATE_R_HEADER;
    const uint32_t flg = uni(M[p + 3u]);
    if (flg & 0xE2u) return MC_INFLATE_R_HEADER;
    uint32_t at = p + 10u;
    if (flg & 4u) {
        if (n - at < 2u) return MC_INFLATE_R_HEADER;
        const uint32_t xlen = uni((uint32_t)M[at] | ((uint32_t)M[at + 1u] << 8));
        if (n - at - 2u < xlen) return MC_INFLATE_R_HEADER;
        at += 2u + xlen;
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1)
        if (flg & bit) {
            bool found = false;
            while (at < n) {                                        // 64 bytes per round: at most (n - at) / 64 + 1 rounds
                const uint32_t i = at + lane;                       // (n <= 2^28: no wrap)
                const unsigned long long zero = __ballot(i < n && M[i] == 0);
                if (zero) { at += (uint32_t)__ffsll((long long)zero); found = true; break; }   // behind the zero byte
                at += 64u;
            }
            if (!found) return MC_INFLATE_R_HEADER;
        }
    pay = at;
    return 0u;
}

// the CRC-32 of dst[0, n), by the wave, in segments of kCrcSegment; all lanes get it
__device__ uint32_t wave_crc32_segments(const uint8_t* dst, uint32_t n, const uint32_t* tab, uint32_t lane)
{
    if (n == 0) return 0u;
    uint32_t reg0 = 0xFFFFFFFFu;                                     // the register in front of the bytes not yet folded (wave-uniform)
    uint32_t done = 0;
    if (n >= kCrcSegment) {
        // lane i's register is followed by (63 - i) * kCrcPerLane bytes of its segment
        const uint32_t op = crc_pow(crc_pow(0x00800000u /* x^8 */, kCrcPerLane), 63u - lane);
        for (; n - done >= kCrcSegment; done += kCrcSegment) {      // n / kCrcSegment rounds
            const uint8_t* s = dst + done + lane * kCrcPerLane;
            uint32_t reg = lane == 0 ? reg0 : 0u;
            for (uint32_t k = 0; k < kCrcPerLane; ++k) reg = tab[(reg ^ s[k]) & 255u] ^ (reg >> 8);
            uint32_t x = crc_mul(op, reg);
            for (int m = 1; m < 64; m <<= 1) x ^= (uint32_t)__shfl_xor((int)x, m);
            reg0 = x;
        }
    }
    const uint32_t rem = n - done;
    if (rem) {                                                       // as wave_crc32: 64 chunks of L, the zeros in front
        const uint8_t* s = dst + done;
        const uint32_t L = (rem + 63u) / 64u, pad = 64u * L - rem;
        const int64_t a0 = (int64_t)lane * L - pad, b0 = a0 + L;
        uint32_t reg = 0;
        if (b0 > 0) {
            if (a0 <= 0) reg = reg0;                                 // the chunk that holds the first byte
            for (uint32_t p = (uint32_t)max(a0, (int64_t)0); p < (uint32_t)b0; ++p) reg = tab[(reg ^ s[p]) & 255u] ^ (reg >> 8);   // L <= 256 rounds
        }
        const uint32_t op = crc_pow(0x00800000u, L);
        uint32_t x = crc_mul(crc_pow(op, 63u - lane), reg);
        for (int m = 1; m < 64; m <<= 1) x ^= (uint32_t)__shfl_xor((int)x, m);
        reg0 = x;
    }
    return ~reg0;
}

__global__ void streams_begin_kernel(StreamArgs a)
{
    a.status[0] = 0; a.status[1] = kNoStreamKey; a.status[2] = 0; a.status[3] = 0;
}

__global__ __launch_bounds__(kStreamBlock) void inflate_streams_kernel(StreamArgs a)
{
    __shared__ uint32_t crcTab[256];
    __shared__ WaveTables tab;
    const uint32_t lane = threadIdx.x;
#pragma unroll
    for (uint32_t j = 0; j < 4u; ++j) {
        uint32_t c = j * 64u + lane;
#pragma unroll
        for (int k = 0; k < 8; ++k) c = (c & 1u) ? (c >> 1) ^ kCrcPoly : c >> 1;
        crcTab[j * 64u + lane] = c;
    }
    __syncthreads();
    const uint64_t r = blockIdx.x;
    const mc_gzip_stream* row = a.rows + r;
    const uint64_t inOff = uni64(row->in_off), inLen = uni64(row->in_len), outOff = uni64(row->out_off), outCap = uni64(row->out_cap);
    uint32_t reason = 0, members = 0, total = 0;
    if (outOff > a.outCap || a.outCap - outOff < outCap) reason = MC_INFLATE_R_OVER;                       // writes nothing
    else if (inLen < kGzipMinRow || inLen > kGzipMaxRowIn || outCap > kGzipMaxRowOut || inOff > a.nbytes || a.nbytes - inOff < inLen)
        reason = MC_INFLATE_R_INPUT;                                                                         // loads nothing
    else {
        const uint8_t* M = a.B + inOff;
        uint8_t* dst = a.out + outOff;
        const uint32_t n = (uint32_t)inLen, cap = (uint32_t)outCap;    // (cap == 2^31 fits)
        uint32_t p = 0;
        for (;;) {                                                   // a member per round: each takes at least 18 of the n bytes
            uint32_t pay = 0;
            reason = gzip_header_wave(M, n, p, members == 0u, lane, pay);
            if (reason) break;
            if (n - pay < 8u) { reason = MC_INFLATE_R_INPUT; break; }
            Out o{dst + total, 0u, 0u, cap - total, 0u};              // this member's: matches reach back to o.dst and no further
            Bits b;
            reason = inflate_deflate(a.B, inOff + pay, n - 8u - pay, inOff + n, o, tab, lane, b);
            if (reason) break;
            bits_drop(b, b.left & 7u);                                // to the next byte (fewer than 8 bits)
            const uint32_t trailer = n - 8u - (b.left >> 3);          // <= n - 8
            const uint32_t crcWant = uni(load_u32(M + trailer)), isize = uni(load_u32(M + trailer + 4u));
            if (o.pos != isize) { reason = o.pos < isize ? MC_INFLATE_R_SHORT : MC_INFLATE_R_OVER; break; }
            wave_order();
            if (wave_crc32_segments(o.dst, o.pos, crcTab, lane) != crcWant) { reason = MC_INFLATE_R_CRC; break; }
            total += o.pos; ++members;
            p = trailer + 8u;
            if (p == n) break;
        }
    }
    if (lane == 0) {
        mc_gzip_result res;
        res.produced = reason ? 0ull : (unsigned long long)total; res.members = members; res.reason = reason;
        a.results[r] = res;
        if (reason) {
            atomicMin(&a.status[1], (unsigned long long)((r << 8) | reason));
            atomicAdd(&a.counters[3], 1ull);
        } else {
            atomicAdd(&a.status[3], 1ull);
            atomicAdd(&a.counters[2], (unsigned long long)total);
        }
    }
}

__global__ void streams_verdict_kernel(StreamArgs a)
{
    const unsigned long long key = a.status[1];
    if (key == kNoStreamKey) { a.status[0] = MC_INFLATE_OK; a.status[1] = 0; a.status[2] = 0; return; }
    const uint32_t reason = (uint32_t)(key & 255u);
    a.status[0] = reason == MC_INFLATE_R_OVER ? MC_INFLATE_OVERFLOW : MC_INFLATE_CORRUPT;
    a.status[1] = key >> 8;
    a.status[2] = reason;
}

// the device form: three launches, nothing waited for
int enqueue_streams(mc_ctx* ctx, InflateState& S, const uint8_t* dBytes, uint64_t nbytes, const mc_gzip_stream* dRows, uint64_t numRows,
                    uint8_t* dOut, uint64_t outCap, mc_gzip_result* dResults, uint64_t* dStatus, hipStream_t st)
{
    StreamArgs a{dBytes, nbytes, dRows, numRows, dOut, outCap, dResults, (unsigned long long*)dStatus, S.dCounters};
    ScopedTimer timer(ctx, "inflate_streams", st);
    hipLaunchKernelGGL(streams_begin_kernel, dim3(1), dim3(1), 0, st, a);
    if (numRows) hipLaunchKernelGGL(inflate_streams_kernel, dim3((uint32_t)numRows), dim3(kStreamBlock), 0, st, a);
    hipLaunchKernelGGL(streams_verdict_kernel, dim3(1), dim3(1), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

}  // namespace

extern "C" {

int mc_gzip_hint(const uint8_t* bytes, uint64_t nbytes, uint64_t info[4])
{
    if (!info) return fail(nullptr, MC_ERR_INVALID, "mc_gzip_hint: no place for info");
    if (!bytes && nbytes > 0) return fail(nullptr, MC_ERR_INVALID, "mc_gzip_hint: no bytes");
    gzip_hint(bytes, nbytes, info);
    return MC_OK;
}

int mc_inflate_streams(mc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, const mc_gzip_stream* rows, uint64_t num_rows, int flags,
                       uint8_t* out, uint64_t out_capacity, mc_gzip_result* results, uint64_t status[4], void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_INFLATE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: unknown flag");
    if (!status) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: no status");
    if (num_rows > 0 && (!bytes || !rows || !results)) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: null array");
    if (num_rows > kMaxStreamRows) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: more than 2^30 rows in one call");
    if (out_capacity > 0 && !out) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: a capacity without its array");
    const bool host = (flags & MC_INFLATE_HOST) != 0;
    if (bytes && out && ranges_overlap((uintptr_t)bytes, (uintptr_t)bytes + nbytes, (uintptr_t)out, (uintptr_t)out + out_capacity))
        return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: out overlaps bytes");
    if (host) {
        if (!gzip_rows_ok(rows, num_rows, nbytes))
            return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: a row is not 18 .. 2^28 bytes inside nbytes with at most 2^31 bytes out, or two out slices overlap");
    } else {
        if (((uintptr_t)bytes | (uintptr_t)out) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: device arrays must be aligned (bytes, out: 16 bytes)");
        if (((uintptr_t)rows | (uintptr_t)results | (uintptr_t)status) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams: device arrays must be aligned (rows, results, status: 8 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_inflate_streams: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    InflateState* S = nullptr;
    int rc = ensure_inflate_state(ctx, &S);
    if (rc) return rc;
    ++S->streamCalls; S->streamBytesIn += nbytes;
    if (!host) return enqueue_streams(ctx, *S, bytes, nbytes, rows, num_rows, out, out_capacity, results, status, st);
    // host arrays: pieces of whole, consecutive rows through the staging buffers, one caller at a time.  A piece covers the span of its
    // rows' bytes (from a multiple of 16) and the span of their slices; its rows are moved to those origins.  A row's bytes leave the
    // device only where the row is accepted.  A row whose slice is not inside out_capacity is refused here, as the kernel would
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t pieceIn = ctx->inflateStageBytes ? ctx->inflateStageBytes : kDefaultStreamStageBytes, pieceOut = 4 * pieceIn;
    std::vector<mc_gzip_stream> piece;
    std::vector<uint64_t> index;                                                  // the piece's rows in the caller's numbering
    std::vector<mc_gzip_result> res;
    std::vector<uint8_t> back;
    uint64_t accepted = 0, lowest = ~0ull, lowestReason = 0, pst[4];
    auto refuse = [&](uint64_t i, uint32_t members, uint32_t reason) {
        results[i].produced = 0; results[i].members = members; results[i].reason = reason;
        if (i < lowest) { lowest = i; lowestReason = reason; }
    };
    for (uint64_t i = 0; i < num_rows;) {
        uint64_t j = i, inLo = ~0ull, inHi = 0, outLo = ~0ull, outHi = 0;
        piece.clear(); index.clear();
        for (; j < num_rows; ++j) {
            const mc_gzip_stream& r = rows[j];
            if (r.out_off > out_capacity || out_capacity - r.out_off < r.out_cap) { refuse(j, 0, MC_INFLATE_R_OVER); ++S->streamRefusedHost; continue; }
            const uint64_t a = std::min<uint64_t>(inLo, r.in_off & ~15ull), b = std::max<uint64_t>(inHi, r.in_off + r.in_len);
            const uint64_t c = std::min<uint64_t>(outLo, r.out_off), d = std::max<uint64_t>(outHi, r.out_off + r.out_cap);
            if (!piece.empty() && (b - a > pieceIn || d - c > pieceOut)) break;
            inLo = a; inHi = b; outLo = c; outHi = d;
            piece.push_back(r); index.push_back(j);
        }
        i = j;
        if (piece.empty()) continue;
        for (mc_gzip_stream& r : piece) { r.in_off -= inLo; r.out_off -= outLo; }
        const uint64_t inSpan = inHi - inLo, outSpan = outHi - outLo, m = piece.size();
        if ((rc = grow(ctx, S->stageIn, (inSpan + 15) / 16 * 16)) != MC_OK || (rc = grow(ctx, S->stageOut, std::max<uint64_t>(outSpan, 16))) != MC_OK ||
            (rc = grow(ctx, S->stageRows, m * sizeof(mc_gzip_stream))) != MC_OK || (rc = grow(ctx, S->stageResults, m * sizeof(mc_gzip_result))) != MC_OK) return rc;
        HIP_TRY(ctx, hipMemcpyAsync(S->stageIn.p, bytes + inLo, inSpan, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(S->stageRows.p, piece.data(), m * sizeof(mc_gzip_stream), hipMemcpyHostToDevice, st));
        if ((rc = enqueue_streams(ctx, *S, (const uint8_t*)S->stageIn.p, inSpan, (const mc_gzip_stream*)S->stageRows.p, m, (uint8_t*)S->stageOut.p, outSpan,
                                  (mc_gzip_result*)S->stageResults.p, (uint64_t*)S->status.dev.p, st)) != MC_OK) return rc;
        res.resize(m); back.resize(outSpan);
        HIP_TRY(ctx, hipMemcpyAsync(res.data(), S->stageResults.p, m * sizeof(mc_gzip_result), hipMemcpyDeviceToHost, st));
        if (outSpan) HIP_TRY(ctx, hipMemcpyAsync(back.data(), S->stageOut.p, outSpan, hipMemcpyDeviceToHost, st));
        if ((rc = read_status(ctx, S->status, 4, pst, st)) != MC_OK) return rc;      // (waits for the copies in front of it too)
        accepted += pst[3];
        for (uint64_t k = 0; k < m; ++k) {
            if (res[k].reason) { refuse(index[k], res[k].members, res[k].reason); continue; }
            results[index[k]] = res[k];
            if (res[k].produced) std::memcpy(out + rows[index[k]].out_off, back.data() + piece[k].out_off, res[k].produced);
        }
    }
    if (lowest == ~0ull) { status[0] = MC_INFLATE_OK; status[1] = 0; status[2] = 0; }
    else { status[0] = lowestReason == MC_INFLATE_R_OVER ? MC_INFLATE_OVERFLOW : MC_INFLATE_CORRUPT; status[1] = lowest; status[2] = lowestReason; }
    status[3] = accepted;
    return MC_OK;
}

int mc_inflate_streams_stats(mc_ctx* ctx, uint64_t stats[4])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_inflate_streams_stats: no place for the counters");
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    InflateState* S = nullptr;
    { std::lock_guard<std::mutex> lock(ctx->inflateMtx); S = ctx->inflate; }
    if (!S) return MC_OK;
    stats[0] = S->streamCalls; stats[1] = S->streamBytesIn; stats[3] = S->streamRefusedHost;
    if (S->dCounters) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        unsigned long long c[4];
        HIP_TRY(ctx, hipMemcpy(c, S->dCounters, sizeof c, hipMemcpyDeviceToHost));
        stats[2] = c[2]; stats[3] += c[3];
    }
    return MC_OK;
}

}  // extern "C"
