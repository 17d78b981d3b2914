// metacache_amd/csrc/parse_cut.hip -- mc_parse_cut / mc_parse_headers: a range of FASTA or FASTQ bytes cut into batches of whole records on
// the device, and the headers of a parsed range packed back to back.  The cut rule is the one of include/metacache_amd.h:
// line starts, record starts and offences are those of the record rule (parse.hip); this file adds where the range is taken to end.
//
// mc_parse_cut is layered as parse.hip is: a tile is kTile bytes, a block owns a tile, a thread one 16-byte load of it.
//   1. cut_lines_kernel    per tile: line starts                                                    -> cut_scan_kernel<1>
//   2. cut_classify_kernel per tile: record starts, first offence, the last two record starts       -> cut_scan_kernel<2>: whole, consumed,
//                                                                                                      the offences in front of consumed, verdict, nb, status
//   3. cut_select_kernel   per tile: record start k with k mod R = 0 and k < whole -> cuts[k / R]; one thread: cuts[nb]
//   4. cut_spans_kernel    per kSpan cuts: the largest cuts[i + 1] - cuts[i]                         -> cut_longest_kernel: status[6]
// cut_scan_kernel and cut_longest_kernel are ONE block each; every loop is bounded by the tile count (the span blocks' for the last).
// No look-back, no flag another block waits for, no atomic: the same bytes give the same outputs.
// The range may begin at ANY address: the 16-byte loads are done from the aligned address below it (A = bytes - shift), a tile is kTile
// bytes of A, and the bytes in front of the range are masked.  Position p of the range is A[p + shift].
// mc_parse_headers is a layer per RECORD, built as the mates layer of parse.hip: sums per kQBlock records, ONE block that scans them,
// the places, then a copy with a wave per record.  Plain HIP C++; no inline assembly.
#include "parse_scan.h"

#include <cstring>

using namespace mcamd;
using namespace mcamd::parsek;

namespace {

constexpr int kCutFlags = MC_PARSE_HOST | MC_PARSE_PAIRS | MC_CUT_OPEN;
// the workspace, in 32-bit words: kHead words, kArrays arrays of one word per tile, one word per kSpan cuts
constexpr uint32_t kHead = 32, kArrays = 5, kSpan = kBlock * 16;
enum { hLines = 0, hRecs, hWhole, hNb, hConsumed, hVerdict };
enum { aLines = 0, aRecs, aOffence, aLast, aSecond };

struct CutArgs {
    const uint8_t* A;                        // the aligned address at or below the range
    uint32_t* ws;
    uint64_t* cuts; uint64_t* status;
    uint64_t capacity;
    uint32_t n, shift, tiles, R, pairs, open, spanBlocks;
};

__host__ __device__ __forceinline__ uint32_t span_blocks_of(uint64_t cuts) { return (uint32_t)((cuts + kSpan - 1) / kSpan); }
__device__ __forceinline__ uint32_t* arr(const CutArgs& a, uint32_t which) { return a.ws + kHead + (uint64_t)which * a.tiles; }
__device__ __forceinline__ uint32_t* spans(const CutArgs& a) { return a.ws + kHead + (uint64_t)kArrays * a.tiles; }

// ---- a thread's 16 bytes of A: the Chunk of parse_scan.h with the range's shift ------------------------------------------------------------
__device__ __forceinline__ uint32_t chunk_line_starts(const CutArgs& a, const Chunk& c)
{
    uint32_t lines = 0, prev = c.prev;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k < c.lo || k >= c.hi) continue;
        if (c.g + k == a.shift || prev == '\n') ++lines;
        prev = CHUNK_BYTE(c, k);
    }
    return lines;
}

struct CutTally { uint32_t recs, offence, last, second; };                       // last, second: position + 1 of the last two record starts (0: none)

// the one walk over a thread's bytes: the line starts and record starts of the record rule and, with JUDGE, its offences (a range whose
// verdict is known needs none).  lines: line starts in front.
template <bool JUDGE, class OnRecord>
__device__ __forceinline__ void walk_cut(const CutArgs& a, const Chunk& c, bool fastq, uint32_t lines, CutTally& t, OnRecord on_record)
{
    uint32_t prev = c.prev;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k < c.lo || k >= c.hi) continue;
        const uint32_t p = c.g + k - a.shift, ch = CHUNK_BYTE(c, k);
        const uint32_t nx = k == 15 ? c.next : (k + 1 < c.hi ? CHUNK_BYTE(c, (k + 1) & 15u) : (uint32_t)'\n');
        if (p == 0 || prev == '\n') {
            bool rec, bad;
            if (fastq) {
                const uint32_t ph = lines & 3u;
                rec = ph == 0;
                bad = JUDGE && (ph == 0 ? ch != '@' : ph == 1 ? (ch == '+' || ch == '>' || ch == '\n' || ch == '\r') : ph == 2 ? ch != '+' : false);
            } else { rec = ch == '>'; bad = JUDGE && ch == '+'; }
            ++lines;
            if (bad) t.offence = min(t.offence, p);
            if (rec) { on_record(t.recs, p); ++t.recs; t.second = t.last; t.last = p + 1; }
        }
        if (JUDGE && ch == '\r' && nx != '\n') t.offence = min(t.offence, p);   // a '\r' that does not end its line: refused, as parse.hip refuses it
        prev = ch;
    }
}
struct NoRecord { __device__ __forceinline__ void operator()(uint32_t, uint32_t) const {} };

// line starts in front of the thread (the tile's own come from cut_scan_kernel<1>)
__device__ __forceinline__ uint32_t lines_in_front(const CutArgs& a, const Chunk& c, uint32_t* lds)
{
    uint32_t sv[1] = {chunk_line_starts(a, c)}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    return arr(a, aLines)[blockIdx.x] + sv[0];
}

__global__ __launch_bounds__(kBlock) void cut_lines_kernel(CutArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const Chunk c = load_chunk(a.A, a.n, a.shift, blockIdx.x * kTile + threadIdx.x * 16u);
    uint32_t sv[1] = {chunk_line_starts(a, c)}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    if (threadIdx.x == 0) arr(a, aLines)[blockIdx.x] = st[0];
}

__global__ __launch_bounds__(kBlock) void cut_classify_kernel(CutArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const bool fastq = a.A[a.shift] == '@';
    const Chunk c = load_chunk(a.A, a.n, a.shift, blockIdx.x * kTile + threadIdx.x * 16u);
    const uint32_t lines = lines_in_front(a, c, lds);
    CutTally t{0, kNone, 0, 0};
    walk_cut<true>(a, c, fastq, lines, t, NoRecord{});
    uint32_t sv[1] = {t.recs}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    const uint32_t offence = block_min(t.offence, lds);
    // the tile's last two record starts: positions differ, so the second is the largest below the last
    const uint32_t last = block_max(t.last, lds), second = block_max(t.last < last ? t.last : t.second, lds);
    if (threadIdx.x == 0) { arr(a, aRecs)[blockIdx.x] = st[0]; arr(a, aOffence)[blockIdx.x] = offence; arr(a, aLast)[blockIdx.x] = last; arr(a, aSecond)[blockIdx.x] = second; }
}

// ONE block: the tiles' values become what lies in front of each tile.  STAGE 1: the line starts.  STAGE 2: the record starts, where the
// range is taken to end (whole, consumed), the first offence in front of that end, the verdict, nb, status.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void cut_scan_kernel(CutArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const uint32_t t = threadIdx.x;
    if (STAGE == 1) {
        uint32_t lines = 0;
        for (uint32_t base = 0; base < a.tiles; base += kBlock) {                // (the same trips for every thread)
            const uint32_t j = base + t;
            const bool in = j < a.tiles;
            uint32_t sv[1] = {in ? arr(a, aLines)[j] : 0u}, m0[1] = {0}, st[1], mt[1];
            block_excl_scan<1, 1>(sv, m0, st, mt, lds);
            if (in) arr(a, aLines)[j] = lines + sv[0];
            lines += st[0];
        }
        if (t == 0) a.ws[hLines] = lines;
    }
    if (STAGE == 2) {
        uint32_t recs = 0, last = 0, second = 0;                                 // last, second: of this thread's tiles (tiles in order: a later tile's are larger)
        for (uint32_t base = 0; base < a.tiles; base += kBlock) {
            const uint32_t j = base + t;
            const bool in = j < a.tiles;
            uint32_t sv[1] = {in ? arr(a, aRecs)[j] : 0u}, m0[1] = {0}, st[1], mt[1];
            block_excl_scan<1, 1>(sv, m0, st, mt, lds);
            if (in) {
                arr(a, aRecs)[j] = recs + sv[0];
                const uint32_t l = arr(a, aLast)[j], s = arr(a, aSecond)[j];
                if (l) { second = s ? s : last; last = l; }
            }
            recs += st[0];
        }
        const uint32_t m1 = block_max(last, lds), m2 = block_max(last < m1 ? last : second, lds);
        // where the range is taken to end (every thread works it out: all of them need consumed)
        const uint32_t first = a.A[a.shift], lines = a.ws[hLines];
        const bool fastq = first == '@';
        uint32_t whole = recs, consumed = a.n;
        if (a.open) {
            if (fastq) whole = (lines - (a.A[a.shift + a.n - 1] != '\n' ? 1u : 0u)) / 4u;   // groups whose four lines end in a '\n' of the range
            else whole = recs ? recs - 1 : 0u;
            if (a.pairs) whole &= ~1u;
            const uint32_t behind = recs - whole;                                // record starts at or behind the end: 0, 1 or 2
            consumed = behind == 0 ? (recs ? a.n : 0u) : behind == 1 ? m1 - 1 : m2 - 1;
        }
        uint32_t offence = kNone;
        for (uint32_t base = 0; base < a.tiles; base += kBlock) {
            const uint32_t j = base + t;
            if (j < a.tiles) { const uint32_t o = arr(a, aOffence)[j]; if (o < consumed) offence = min(offence, o); }   // (kNone is not below consumed)
        }
        offence = block_min(offence, lds);
        if (t == 0) {
            if (!a.open && fastq && (lines & 3u)) offence = min(offence, a.n);   // an incomplete last group
            if (first != '@' && first != '>') offence = 0;
            const uint64_t nb = ((uint64_t)whole + a.R - 1) / a.R;
            uint32_t verdict = MC_PARSE_OK;
            if (offence != kNone) verdict = MC_PARSE_IRREGULAR;
            else if (nb + 1 > a.capacity) verdict = MC_PARSE_OVERFLOW;
            a.ws[hRecs] = recs; a.ws[hWhole] = whole; a.ws[hNb] = (uint32_t)nb; a.ws[hConsumed] = consumed; a.ws[hVerdict] = verdict;
            a.status[0] = whole; a.status[1] = nb; a.status[2] = consumed; a.status[3] = recs;
            a.status[4] = verdict; a.status[5] = offence == kNone ? 0 : offence; a.status[6] = 0;
            a.status[7] = (!a.open && a.pairs && (whole & 1u)) ? 1 : 0;
        }
    }
}

struct SelectRecord {
    const CutArgs& a; uint32_t inFront, whole;
    __device__ __forceinline__ void operator()(uint32_t local, uint32_t p) const
    {
        const uint32_t k = inFront + local;
        if (k < whole && k % a.R == 0) a.cuts[k / a.R] = p;
    }
};

__global__ __launch_bounds__(kBlock) void cut_select_kernel(CutArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const bool fastq = a.A[a.shift] == '@';
    const Chunk c = load_chunk(a.A, a.n, a.shift, blockIdx.x * kTile + threadIdx.x * 16u);
    const uint32_t lines = lines_in_front(a, c, lds);
    CutTally t{0, kNone, 0, 0};
    walk_cut<false>(a, c, fastq, lines, t, NoRecord{});                     // (the verdict is MC_PARSE_OK: only the record starts are counted)
    uint32_t sv[1] = {t.recs}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    CutTally t2{0, kNone, 0, 0};
    walk_cut<false>(a, c, fastq, lines, t2, SelectRecord{a, arr(a, aRecs)[blockIdx.x] + sv[0], a.ws[hWhole]});
    if (blockIdx.x == 0 && threadIdx.x == 0) a.cuts[a.ws[hNb]] = a.ws[hConsumed];
}

// the largest batch of kSpan batches: a thread looks at 16 of them, kBlock apart
__global__ __launch_bounds__(kBlock) void cut_spans_kernel(CutArgs a)
{
    __shared__ uint32_t lds[kWaves];
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const uint32_t nb = a.ws[hNb];
    if ((uint64_t)blockIdx.x * kSpan >= nb) return;
    uint32_t longest = 0;
#pragma unroll 4
    for (uint32_t k = 0; k < 16; ++k) {
        const uint64_t i = (uint64_t)blockIdx.x * kSpan + k * kBlock + threadIdx.x;
        if (i < nb) longest = max(longest, (uint32_t)(a.cuts[i + 1] - a.cuts[i]));
    }
    longest = block_max(longest, lds);
    if (threadIdx.x == 0) spans(a)[blockIdx.x] = longest;
}

// ONE block: status[6]
__global__ __launch_bounds__(kBlock) void cut_longest_kernel(CutArgs a)
{
    __shared__ uint32_t lds[kWaves];
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const uint32_t blocks = min(span_blocks_of(a.ws[hNb]), a.spanBlocks);
    uint32_t longest = 0;
    for (uint32_t j = threadIdx.x; j < blocks; j += kBlock) longest = max(longest, spans(a)[j]);
    longest = block_max(longest, lds);
    if (threadIdx.x == 0) a.status[6] = longest;
}

// batches a range of nbytes can be cut into at the most: a record takes two bytes at least
uint64_t most_batches(uint64_t nbytes) { return nbytes / 2 + 1; }

// ---- mc_parse_headers: a layer per RECORD ------------------------------------------------------------------------------------------------
constexpr uint32_t kQBlock = kBlock, kHHead = 32;
enum { gVerdict = 0, gRecs, gTotal };

struct HeadersArgs {
    const uint8_t* B; const uint32_t* hdr; const uint64_t* parseStatus;
    uint32_t* ws;                            // kHHead words, one word per kQBlock records
    uint8_t* out; uint64_t* outOff; uint64_t* status;
    uint64_t outCap;
    uint32_t n, maxRecords;                  // n: bytes of the range
};

__host__ __device__ __forceinline__ uint32_t qblocks_of(uint32_t records) { return (records + kQBlock - 1) / kQBlock; }
__device__ __forceinline__ uint32_t* hblk(const HeadersArgs& a) { return a.ws + kHHead; }
// the records the tables have room for (0 where the parse refused the range or left more records than max_records)
__device__ __forceinline__ uint32_t header_records(const HeadersArgs& a)
{
    const uint64_t recs = a.parseStatus[0];
    return (a.parseStatus[4] == MC_PARSE_OK && recs <= a.maxRecords) ? (uint32_t)recs : 0u;
}

__global__ __launch_bounds__(kQBlock) void headers_sums_kernel(HeadersArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const uint32_t recs = header_records(a);
    if (blockIdx.x * kQBlock >= recs) return;
    const uint32_t r = blockIdx.x * kQBlock + threadIdx.x;
    uint32_t sv[1] = {r < recs ? a.hdr[2ull * r + 1] : 0u}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    if (threadIdx.x == 0) hblk(a)[blockIdx.x] = st[0];
}

// ONE block: the blocks' sums turned into what lies in front of each (a trip: kBlock * kQBlock records), the verdict, status
__global__ __launch_bounds__(kBlock) void headers_scan_kernel(HeadersArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const uint32_t t = threadIdx.x, recs = header_records(a), nb = qblocks_of(recs);
    uint32_t inFront = 0;
    for (uint32_t base = 0; base < nb; base += kBlock) {                          // (the same trips for every thread)
        const uint32_t j = base + t;
        const bool in = j < nb;
        uint32_t sv[1] = {in ? hblk(a)[j] : 0u}, m0[1] = {0}, st[1], mt[1];
        block_excl_scan<1, 1>(sv, m0, st, mt, lds);
        if (in) hblk(a)[j] = inFront + sv[0];
        inFront += st[0];
    }
    if (t == 0) {
        const uint64_t parsed = a.parseStatus[4], all = a.parseStatus[0];
        uint32_t verdict = (uint32_t)parsed;
        if (parsed == MC_PARSE_OK && (all > a.maxRecords || inFront > a.outCap)) verdict = MC_PARSE_OVERFLOW;
        a.ws[gVerdict] = verdict; a.ws[gRecs] = recs; a.ws[gTotal] = inFront;
        a.status[0] = parsed == MC_PARSE_OK ? all : 0; a.status[1] = inFront; a.status[2] = verdict; a.status[3] = 0;
    }
}

__global__ __launch_bounds__(kQBlock) void headers_place_kernel(HeadersArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    if (a.ws[gVerdict] != MC_PARSE_OK) return;
    const uint32_t recs = a.ws[gRecs];
    const uint32_t r = blockIdx.x * kQBlock + threadIdx.x;
    if (r == 0) a.outOff[recs] = a.ws[gTotal];
    if (blockIdx.x * kQBlock >= recs) return;
    uint32_t sv[1] = {r < recs ? a.hdr[2ull * r + 1] : 0u}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    if (r < recs) a.outOff[r] = hblk(a)[blockIdx.x] + sv[0];
}

// a wave per record: headers are tens of bytes
__global__ __launch_bounds__(kBlock) void headers_copy_kernel(HeadersArgs a)
{
    if (a.ws[gVerdict] != MC_PARSE_OK) return;
    const uint32_t r = blockIdx.x * kWaves + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (r >= a.ws[gRecs]) return;
    const uint32_t off = a.hdr[2ull * r], len = a.hdr[2ull * r + 1];
    const uint64_t at = a.outOff[r];
    const uint32_t inside = off < a.n ? min(len, a.n - off) : 0u;                // (hdr rows that are not this range's read nothing outside it)
    for (uint32_t k = lane; k < inside; k += 64u) a.out[at + k] = a.B[off + k];
}

}  // namespace

namespace mcamd {

struct CutState {                        // what the context keeps for the MC_PARSE_HOST forms of mc_parse_cut and mc_parse_headers
    std::mutex stageMtx;                 // callers take turns at the staging buffers
    DevBuf stageIn, stageWs, stageCuts, stageHdr, stageOut, stageOff;
    StatusStage status;                  // [16]: mc_parse_cut reads 8 words; mc_parse_headers keeps the parse's 8 in front of its own 4
};

void free_cut_state(mc_ctx* ctx)
{
    if (!ctx->cut) return;
    CutState& S = *ctx->cut;
    free_status_stage(S.status);
    for (DevBuf* b : {&S.stageIn, &S.stageWs, &S.stageCuts, &S.stageHdr, &S.stageOut, &S.stageOff})
        if (b->p) (void)hipFree(b->p);
    delete ctx->cut;
    ctx->cut = nullptr;
}

}  // namespace mcamd

namespace {

int ensure_cut_state(mc_ctx* ctx, CutState** out)
{
    std::lock_guard<std::mutex> lock(ctx->cutMtx);
    if (!ctx->cut) ctx->cut = new CutState;
    CutState& S = *ctx->cut;
    *out = &S;
    return make_status_stage(ctx, S.status, 16);
}

// the device form: two byte passes and their scans, the selection, the spans; nothing waited for
int enqueue_cut(mc_ctx* ctx, const uint8_t* dBytes, uint32_t n, uint32_t R, int flags, uint64_t* cuts, uint64_t capacity, uint64_t* status, void* ws, hipStream_t st)
{
    CutArgs a{};
    a.shift = (uint32_t)((uintptr_t)dBytes & 15u);
    a.A = dBytes - a.shift; a.ws = (uint32_t*)ws; a.cuts = cuts; a.status = status; a.capacity = capacity;
    a.n = n; a.tiles = tiles_of((uint64_t)n + a.shift); a.R = R;
    a.pairs = (flags & MC_PARSE_PAIRS) ? 1u : 0u; a.open = (flags & MC_CUT_OPEN) ? 1u : 0u;
    a.spanBlocks = span_blocks_of(std::min<uint64_t>(capacity ? capacity - 1 : 0, most_batches(n)));
    ScopedTimer timer(ctx, "parse_cut", st);
    hipLaunchKernelGGL(cut_lines_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(cut_scan_kernel<1>, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(cut_classify_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(cut_scan_kernel<2>, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(cut_select_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
    if (a.spanBlocks) hipLaunchKernelGGL(cut_spans_kernel, dim3(a.spanBlocks), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(cut_longest_kernel, dim3(1), dim3(kBlock), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

uint64_t headers_words(uint32_t maxRecords) { return (uint64_t)kHHead + qblocks_of(maxRecords); }

}  // namespace

namespace mcamd {

// mc_parse_headers' device form, for the call itself and for the slots (raw_parse, context.cpp): four launches, nothing waited for
int enqueue_parse_headers(mc_ctx* ctx, const uint8_t* dBytes, uint32_t nbytes, const uint32_t* hdr, const uint64_t* parseStatus, uint32_t maxRecords, uint8_t* out, uint64_t outCap,
                          uint64_t* outOff, uint64_t* status, void* ws, hipStream_t st)
{
    HeadersArgs a{};
    a.B = dBytes; a.hdr = hdr; a.parseStatus = parseStatus; a.ws = (uint32_t*)ws; a.out = out; a.outOff = outOff; a.status = status; a.outCap = outCap; a.n = nbytes; a.maxRecords = maxRecords;
    ScopedTimer timer(ctx, "parse_headers", st);
    if (maxRecords) hipLaunchKernelGGL(headers_sums_kernel, dim3(qblocks_of(maxRecords)), dim3(kQBlock), 0, st, a);
    hipLaunchKernelGGL(headers_scan_kernel, dim3(1), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(headers_place_kernel, dim3(std::max(1u, qblocks_of(maxRecords))), dim3(kQBlock), 0, st, a);
    if (maxRecords) hipLaunchKernelGGL(headers_copy_kernel, dim3((maxRecords + kWaves - 1) / kWaves), dim3(kBlock), 0, st, a);
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

}  // namespace mcamd

extern "C" {

uint64_t mc_parse_cut_scratch_bytes(uint64_t nbytes)
{
    const uint64_t words = (uint64_t)kHead + (uint64_t)kArrays * tiles_of(nbytes + 15) + span_blocks_of(most_batches(nbytes));
    return (words * 4 + 255) / 256 * 256;
}

int mc_parse_cut(mc_ctx* ctx, const char* bytes, uint64_t nbytes, uint32_t records_per_batch, int flags, uint64_t* cuts, uint64_t capacity, uint64_t status[8],
                 void* workspace, uint64_t workspace_bytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~kCutFlags) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: unknown flag");
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: no bytes");
    if (nbytes > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: more than 2^31 bytes in one range");
    if (records_per_batch == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: no records per batch");
    if ((flags & MC_PARSE_PAIRS) && (records_per_batch & 1u)) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: MC_PARSE_PAIRS with an odd number of records per batch");
    if (!cuts || !status) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: no cuts or no status");
    const bool host = (flags & MC_PARSE_HOST) != 0;
    if (!host) {
        if (!workspace || workspace_bytes < mc_parse_cut_scratch_bytes(nbytes)) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: the workspace is smaller than mc_parse_cut_scratch_bytes");
        if ((uintptr_t)workspace & 15u) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: device arrays must be aligned (workspace: 16 bytes)");
        if (((uintptr_t)cuts | (uintptr_t)status) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_parse_cut: device arrays must be aligned (cuts, status: 8 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_parse_cut: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const uint32_t n = (uint32_t)nbytes;
    if (!host) return enqueue_cut(ctx, (const uint8_t*)bytes, n, records_per_batch, flags, cuts, capacity, status, workspace, st);
    // host arrays: through the staging buffers, one caller at a time; the cuts leave the device only with the verdict MC_PARSE_OK
    CutState* S = nullptr;
    int rc = ensure_cut_state(ctx, &S);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t room = std::min<uint64_t>(capacity, most_batches(nbytes) + 1);   // (no range needs more)
    if ((rc = grow(ctx, S->stageWs, mc_parse_cut_scratch_bytes(nbytes))) != MC_OK || (rc = grow(ctx, S->stageCuts, std::max<uint64_t>(room * 8, 16))) != MC_OK ||
        (rc = stage_bytes(ctx, S->stageIn, bytes, nbytes, st)) != MC_OK) return rc;
    if ((rc = enqueue_cut(ctx, (const uint8_t*)S->stageIn.p, n, records_per_batch, flags & ~MC_PARSE_HOST, (uint64_t*)S->stageCuts.p, room, (uint64_t*)S->status.dev.p, S->stageWs.p, st)) != MC_OK) return rc;
    if ((rc = read_status(ctx, S->status, 8, status, st)) != MC_OK) return rc;
    if (status[4] != MC_PARSE_OK) return MC_OK;
    HIP_TRY(ctx, hipMemcpyAsync(cuts, S->stageCuts.p, (status[1] + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MC_OK;
}

uint64_t mc_parse_headers_scratch_bytes(uint32_t max_records)
{
    return (headers_words(max_records) * 4 + 255) / 256 * 256;
}

int mc_parse_headers(mc_ctx* ctx, const char* bytes, uint64_t nbytes, const uint32_t* hdr, const uint64_t* parse_status, uint32_t max_records, int flags,
                     char* out, uint64_t out_capacity, uint64_t* out_off, uint64_t status[4], void* workspace, uint64_t workspace_bytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_PARSE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: flags other than MC_PARSE_HOST");
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: no bytes");
    if (nbytes > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: more than 2^31 bytes in one range");
    if (!parse_status || !status || !out_off) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: no parse status, no status or no out_off");
    if (max_records > 0 && !hdr) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: null array");
    if (out_capacity > 0 && !out) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: a capacity without its array");
    const bool host = (flags & MC_PARSE_HOST) != 0;
    if (!host) {
        if (!workspace || workspace_bytes < mc_parse_headers_scratch_bytes(max_records)) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: the workspace is smaller than mc_parse_headers_scratch_bytes");
        if ((uintptr_t)workspace & 15u) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: device arrays must be aligned (workspace: 16 bytes)");
        if (((uintptr_t)parse_status | (uintptr_t)out_off | (uintptr_t)status) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: device arrays must be aligned (parse_status, out_off, status: 8 bytes)");
        if ((uintptr_t)hdr & 3u) return fail(ctx, MC_ERR_INVALID, "mc_parse_headers: device arrays must be aligned (hdr: 4 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_parse_headers: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (!host) return enqueue_parse_headers(ctx, (const uint8_t*)bytes, (uint32_t)nbytes, hdr, parse_status, max_records, (uint8_t*)out, out_capacity, out_off, status, workspace, st);
    // host arrays: through the staging buffers, one caller at a time; out and out_off leave the device only with the verdict MC_PARSE_OK
    CutState* S = nullptr;
    int rc = ensure_cut_state(ctx, &S);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t outRoom = std::min<uint64_t>(out_capacity, nbytes);           // (the headers are bytes of the range)
    if ((rc = grow(ctx, S->stageIn, nbytes)) != MC_OK || (rc = grow(ctx, S->stageWs, mc_parse_headers_scratch_bytes(max_records))) != MC_OK ||
        (rc = grow(ctx, S->stageHdr, std::max<uint64_t>((uint64_t)max_records * 8, 16))) != MC_OK || (rc = grow(ctx, S->stageOut, std::max<uint64_t>(outRoom, 16))) != MC_OK ||
        (rc = grow(ctx, S->stageOff, ((uint64_t)max_records + 1) * 8)) != MC_OK) return rc;
    uint64_t* dParse = (uint64_t*)S->status.dev.p;                                // [8] the parse's status, [8] this call's
    HIP_TRY(ctx, hipMemcpyAsync(S->stageIn.p, bytes, nbytes, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(dParse, parse_status, 64, hipMemcpyHostToDevice, st));
    const uint64_t rows = (parse_status[4] == MC_PARSE_OK) ? std::min<uint64_t>(parse_status[0], max_records) : 0;
    if (rows) HIP_TRY(ctx, hipMemcpyAsync(S->stageHdr.p, hdr, rows * 8, hipMemcpyHostToDevice, st));
    if ((rc = enqueue_parse_headers(ctx, (const uint8_t*)S->stageIn.p, (uint32_t)nbytes, (const uint32_t*)S->stageHdr.p, dParse, max_records, (uint8_t*)S->stageOut.p, outRoom,
                              (uint64_t*)S->stageOff.p, dParse + 8, S->stageWs.p, st)) != MC_OK) return rc;
    if ((rc = read_status(ctx, S->status, 4, status, st, dParse + 8)) != MC_OK) return rc;
    if (status[2] != MC_PARSE_OK) return MC_OK;
    HIP_TRY(ctx, hipMemcpyAsync(out_off, S->stageOff.p, (status[0] + 1) * 8, hipMemcpyDeviceToHost, st));
    if (status[1]) HIP_TRY(ctx, hipMemcpyAsync(out, S->stageOut.p, status[1], hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MC_OK;
}

}  // extern "C"
