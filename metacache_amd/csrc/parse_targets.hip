// metacache_amd/csrc/parse_targets.hip -- mc_parse_targets / mc_parse_targets_scratch_bytes: a byte range that holds MANY FASTA files back
// to back cut into the targets of a build on the device.  The target rule is the one of include/metacache_amd.h: every file
// of the range is judged by the FASTA record rule (parse.hip) ON ITS OWN -- a file's first byte is a line start whatever precedes it, a
// file need not end in '\n', and every file begins with '>'.  Whatever this file cannot decide inside its rule it REFUSES.
//
// The layering is the PER-RECORD one of parse.hip's mates path, not a padding pass over the bytes: a target needs its length, its file and
// its number inside that file, all of which belong to a record and none to a byte; with the lengths in a table by record number the places
// are one scan over the records of pad4(len), and index = r - (the number of the record that starts at file_off[file]) costs nothing.  A
// padding pass would read the bytes once more to learn the same places and would still need the record table for file and index.
//   0. targets_table_kernel    per row of file_off: the first row that breaks the table's rule                 -> targets_scan_kernel<1>
//   1. targets_lines_kernel    per tile: the last line start                                                   -> targets_scan_kernel<1>
//   2. targets_classify_kernel per tile: record starts, sequence bytes kept (S), S at the last record start,
//                                        the first offence                                                     -> targets_scan_kernel<2> (+ the offence's file)
//   3. targets_lengths_kernel  per tile: len[r], file[r], firstRec[file]; padding, records with bytes, longest -> targets_sums_kernel per kQBlock
//                                        records: the sum of pad4(len)                                         -> targets_scan_kernel<3> (+ verdict, status)
//   4. targets_place_kernel    per record: targets[r], the padding bytes, the 16 bytes behind
//   5. targets_write_kernel    per tile: sequence byte -> seq[seq_off[r] + (S - S at the record's start)], hdr
// A tile is kTile bytes, a block owns a tile, a thread 16 bytes of it (one 16-byte load).  What a byte IS needs only the last line start
// in front of it: the line is a header where that byte is '>'.  A thread finds the files that start inside its 16 bytes by an ordered
// search over file_off (several may: ">" alone is a whole file).  targets_scan_kernel is ONE block.  No atomic decides a position: the same
// bytes give the same outputs.  Every loop is bounded by the range, the file table or max_records.  Plain HIP C++; no inline assembly.
#include "parse_scan.h"

#include <cstring>

using namespace mcamd;
using namespace mcamd::parsek;

namespace {

// the workspace, in 32-bit words: kHead words, kArrays arrays of one word per tile, one word per kBlock rows of the file table, then the
// record layer: len and file by record number (max_records words each), firstRec by file, one word per kQBlock records
constexpr uint32_t kHead = 32, kArrays = 8, kQBlock = kBlock;
enum { hTabBad = 0, hRecs, hSeq, hOffence, hOffFile, hPads, hNonEmpty, hLongest, hVerdict, hSeqEnd };
enum { aLastLine = 0, aRecs, aSeq, aOffence, aRecAt, aPads, aNonEmpty, aLongest };

struct TargetsArgs {
    const uint8_t* B; const uint64_t* fileOff;
    uint32_t* ws;
    uint32_t* hdr; mc_parse_target* targets; uint8_t* seq; uint64_t* status;
    unsigned long long* counters;            // the context's: records, refused ranges (mc_parse_stats)
    uint64_t seqCap;
    uint32_t n, tiles, numFiles, maxRecords, tabBlocks;
};

__host__ __device__ __forceinline__ uint32_t blocks_of(uint64_t rows) { return (uint32_t)((rows + kBlock - 1) / kBlock); }
__device__ __forceinline__ uint32_t* arr(const TargetsArgs& a, uint32_t which) { return a.ws + kHead + (uint64_t)which * a.tiles; }
__device__ __forceinline__ uint32_t* tab_blocks(const TargetsArgs& a) { return a.ws + kHead + (uint64_t)kArrays * a.tiles; }
__device__ __forceinline__ uint32_t* rec_len(const TargetsArgs& a) { return tab_blocks(a) + a.tabBlocks; }
__device__ __forceinline__ uint32_t* rec_file(const TargetsArgs& a) { return rec_len(a) + a.maxRecords; }
__device__ __forceinline__ uint32_t* first_rec(const TargetsArgs& a) { return rec_file(a) + a.maxRecords; }
__device__ __forceinline__ uint32_t* rec_blocks(const TargetsArgs& a) { return first_rec(a) + a.numFiles; }
__device__ __forceinline__ uint32_t pad4(uint32_t len) { return (len + 3u) & ~3u; }

// the first row of file_off[lo .. hi) that is not below p (hi: none); at most 32 steps whatever the table holds
__device__ __forceinline__ uint32_t lower_row(const TargetsArgs& a, uint64_t p, uint32_t lo, uint32_t hi)
{
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.fileOff[mid] < p) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- the files of a thread's 16 bytes: bit k of starts: position g + k is the first byte of a file; bit k of ends: it is the last byte
// of its file; inFront: the file of position g - 1 (of no meaning where bit 0 of starts is set).  EVERY thread of the block calls this: two
// of them search the whole table for the rows of the tile's two ends, and a thread's own search runs between those (a tile of a few files:
// a step or two, not one per bit of the file count) ---------------------------------------------------------------------------------------
struct Files { uint32_t starts, ends, inFront; };

__device__ __forceinline__ Files files_of(const TargetsArgs& a, uint32_t g)
{
    __shared__ uint32_t tileRows[2];
    if (threadIdx.x < 2) tileRows[threadIdx.x] = lower_row(a, ((uint64_t)blockIdx.x + threadIdx.x) * kTile, 0, a.numFiles + 1);
    __syncthreads();
    Files fl{0, 0, 0};
    if (g >= a.n) return fl;
    uint32_t f = lower_row(a, g, tileRows[0], tileRows[1]);
    fl.inFront = f - 1u;
    const uint64_t end = (uint64_t)g + 16u;
    uint32_t starts = 0;
    for (uint32_t it = 0; it < 16 && f < a.numFiles; ++it, ++f) {                // (a table that ascends strictly has at most 16 rows in 16 bytes)
        const uint64_t o = a.fileOff[f];
        if (o < g || o >= end) break;
        starts |= 1u << (uint32_t)(o - g);
    }
    if (f <= a.numFiles && a.fileOff[f] == end) starts |= 1u << 16;              // (the byte behind the chunk begins a file, or the range ends there)
    fl.starts = starts & 0xFFFFu;
    fl.ends = (starts >> 1) & 0xFFFFu;
    if (a.n - 1u - g < 16u) fl.ends |= 1u << (a.n - 1u - g);
    return fl;
}

// layer 1, which needs nothing in front of it: the last line start + 1 (0: none)
__device__ __forceinline__ uint32_t chunk_last_line(const Chunk& c, const Files& fl)
{
    uint32_t lastLine = 0, prev = c.prev;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k >= c.hi) continue;
        if (((fl.starts >> k) & 1u) || prev == '\n') lastLine = c.g + k + 1;
        prev = CHUNK_BYTE(c, k);
    }
    return lastLine;
}

// what runs along the bytes (in front of the byte the walk stands at)
struct State { uint32_t lastLine, recs, S, recAt; };      // recAt: S at the last record start
// what a walk leaves for the scans.  recAt: S + 1 at the last record start of the walk (0: none); pads, nonEmpty, longest: ABSOLUTE walks,
// over the records that ended inside the walk
struct Tally { uint32_t recAt, offence, pads, nonEmpty, longest; };

__device__ __forceinline__ Tally empty_tally() { return Tally{0, kNone, 0, 0, 0}; }

struct NoSink {
    __device__ __forceinline__ void seq_byte(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void header(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void record_start(uint32_t, uint32_t, bool) {}
    __device__ __forceinline__ void record(uint32_t, uint32_t) {}
};
// layer 3: the record tables (rows: how many records they hold)
struct LenSink {
    const TargetsArgs& a; uint32_t rows;
    __device__ __forceinline__ void seq_byte(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void header(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void record_start(uint32_t r, uint32_t file, bool fileStart)
    {
        if (r < rows) rec_file(a)[r] = file;
        if (fileStart && file < a.numFiles) first_rec(a)[file] = r;
    }
    __device__ __forceinline__ void record(uint32_t r, uint32_t len) { if (r < rows) rec_len(a)[r] = len; }
};
// layer 5: the bytes (the verdict is MC_PARSE_OK: every record has its row)
struct WriteSink {
    const TargetsArgs& a; uint32_t curRec, curPlace;
    __device__ __forceinline__ void seq_byte(uint32_t r, uint32_t within, uint32_t ch)
    {
        if (r != curRec) { curRec = r; curPlace = (uint32_t)a.targets[r].seq_off; }
        a.seq[curPlace + within] = (uint8_t)ch;
    }
    __device__ __forceinline__ void header(uint32_t r, uint32_t off, uint32_t len) { a.hdr[2ull * r] = off; a.hdr[2ull * r + 1] = len; }
    __device__ __forceinline__ void record_start(uint32_t, uint32_t, bool) {}
    __device__ __forceinline__ void record(uint32_t, uint32_t) {}
};

// a record has ended with S sequence bytes in front of the walk (ABSOLUTE walks only)
template <class Sink>
__device__ __forceinline__ void close_record(State& s, Tally& t, Sink& sink)
{
    const uint32_t len = s.S - s.recAt;
    sink.record(s.recs - 1, len);
    t.pads += (0u - len) & 3u;
    t.nonEmpty += len ? 1u : 0u;
    t.longest = max(t.longest, len);
}

// the one walk over a thread's bytes.  ABS: s holds the true values in front of the thread; otherwise only lastLine is true and recs, S
// count from 0 (the kind of a line needs no more than its line start).
template <bool ABS, class Sink>
__device__ __forceinline__ void walk(const TargetsArgs& a, const Chunk& c, const Files& fl, State& s, Tally& t, Sink& sink)
{
    bool hdr = false, seq = false;                                               // the kind of the line the walk stands in
    if (s.lastLine) { hdr = a.B[s.lastLine - 1] == '>'; seq = !hdr; }
    uint32_t prev = c.prev, file = fl.inFront;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k >= c.hi) continue;
        const uint32_t p = c.g + k, ch = CHUNK_BYTE(c, k);
        const bool fileStart = (fl.starts >> k) & 1u, fileEnd = (fl.ends >> k) & 1u;
        const uint32_t nx = fileEnd ? (uint32_t)'\n' : (k == 15 ? c.next : CHUNK_BYTE(c, (k + 1) & 15u));
        if (fileStart) ++file;
        if (fileStart || prev == '\n') {
            s.lastLine = p + 1;
            hdr = ch == '>'; seq = !hdr;
            if (ch == '+' || (fileStart && !hdr)) t.offence = min(t.offence, p);
            if (hdr) {
                if (ABS && s.recs) close_record(s, t, sink);
                ++s.recs;
                s.recAt = s.S; t.recAt = s.S + 1;
                if (ABS) sink.record_start(s.recs - 1, file, fileStart);
            }
        }
        const bool kept = ch != '\n' && !(ch == '\r' && nx == '\n');
        if (ch == '\r' && nx != '\n') t.offence = min(t.offence, p);            // a '\r' that does not end its line: not decided here, refused
        if (seq && kept) { if (ABS && s.recs) sink.seq_byte(s.recs - 1, s.S - s.recAt, ch); ++s.S; }
        if (hdr && (ch == '\n' || fileEnd)) {
            const uint32_t te = ch == '\n' ? p - (prev == '\r' ? 1u : 0u) : p + 1u - (ch == '\r' ? 1u : 0u);
            sink.header(s.recs - 1, s.lastLine, te - s.lastLine);
        }
        if (ABS && p + 1 == a.n && s.recs) close_record(s, t, sink);
        prev = ch;
    }
}

// layer 1 for the block: lastLine in front of the thread (the tile's own comes from targets_scan_kernel<1>)
__device__ __forceinline__ void layer1(const TargetsArgs& a, const Chunk& c, const Files& fl, State& s, uint32_t* lds)
{
    uint32_t s0[1] = {0}, mv[1] = {chunk_last_line(c, fl)}, s0t[1], mt[1];
    block_excl_scan<1, 1>(s0, mv, s0t, mt, lds);
    s.lastLine = max(arr(a, aLastLine)[blockIdx.x], mv[0]);
    s.recs = s.S = s.recAt = 0;
}

// layer 2 for the block: the relative walk, then recs / S / recAt in front of the thread (the tile's own from targets_scan_kernel<2>)
__device__ __forceinline__ void layer2(const TargetsArgs& a, const Chunk& c, const Files& fl, State& s, uint32_t* lds)
{
    State r = s;
    Tally t = empty_tally();
    NoSink none;
    walk<false>(a, c, fl, r, t, none);
    uint32_t sv[2] = {r.recs, r.S}, m0[1] = {0}, st[2], m0t[1];
    block_excl_scan<2, 1>(sv, m0, st, m0t, lds);
    s.recs = arr(a, aRecs)[blockIdx.x] + sv[0];
    s.S = arr(a, aSeq)[blockIdx.x] + sv[1];
    uint32_t s0[1] = {0}, av[1] = {t.recAt ? s.S + t.recAt - 1 : 0u}, s0t[1], at[1];
    block_excl_scan<1, 1>(s0, av, s0t, at, lds);
    s.recAt = max(arr(a, aRecAt)[blockIdx.x], av[0]);
}

// a thread per row of the file table: row 0 is 0, every row lies above the one in front of it, row numFiles is the range's end
__global__ __launch_bounds__(kBlock) void targets_table_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[kWaves];
    const uint32_t row = blockIdx.x * kBlock + threadIdx.x;
    uint32_t bad = kNone;
    if (row <= a.numFiles) {
        const uint64_t o = a.fileOff[row];
        if ((row == 0 && o != 0) || (row > 0 && o <= a.fileOff[row - 1]) || (row == a.numFiles && o != a.n)) bad = row;
    }
    bad = block_min(bad, lds);
    if (threadIdx.x == 0) tab_blocks(a)[blockIdx.x] = bad;
}

__global__ __launch_bounds__(kBlock) void targets_lines_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const uint32_t g = blockIdx.x * kTile + threadIdx.x * 16u;
    const Chunk c = load_chunk(a.B, a.n, 0, g);
    const Files fl = files_of(a, g);
    uint32_t s0[1] = {0}, mv[1] = {chunk_last_line(c, fl)}, s0t[1], mt[1];
    block_excl_scan<1, 1>(s0, mv, s0t, mt, lds);
    if (threadIdx.x == 0) arr(a, aLastLine)[blockIdx.x] = mt[0];
}

__global__ __launch_bounds__(kBlock) void targets_classify_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[3 * kWaves];
    if (a.ws[hTabBad] != kNone) return;
    const uint32_t g = blockIdx.x * kTile + threadIdx.x * 16u;
    const Chunk c = load_chunk(a.B, a.n, 0, g);
    const Files fl = files_of(a, g);
    State s;
    layer1(a, c, fl, s, lds);
    Tally t = empty_tally();
    NoSink none;
    walk<false>(a, c, fl, s, t, none);
    // the tile's sums, and S + 1 at its last record start, S counted from the tile's first byte
    uint32_t sv[2] = {s.recs, s.S}, m0[1] = {0}, st[2], m0t[1];
    block_excl_scan<2, 1>(sv, m0, st, m0t, lds);
    uint32_t s0[1] = {0}, mv[1] = {t.recAt ? sv[1] + t.recAt : 0u}, s0t[1], mt[1];
    block_excl_scan<1, 1>(s0, mv, s0t, mt, lds);
    const uint32_t offence = block_min(t.offence, lds);
    if (threadIdx.x == 0) {
        arr(a, aRecs)[blockIdx.x] = st[0]; arr(a, aSeq)[blockIdx.x] = st[1];
        arr(a, aOffence)[blockIdx.x] = offence; arr(a, aRecAt)[blockIdx.x] = mt[0];
    }
}

__global__ __launch_bounds__(kBlock) void targets_lengths_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[3 * kWaves];
    if (a.ws[hOffence] != kNone) return;
    const uint32_t g = blockIdx.x * kTile + threadIdx.x * 16u;
    const Chunk c = load_chunk(a.B, a.n, 0, g);
    const Files fl = files_of(a, g);
    State s;
    layer1(a, c, fl, s, lds);
    layer2(a, c, fl, s, lds);
    Tally t = empty_tally();
    LenSink sink{a, a.ws[hRecs] <= a.maxRecords ? a.maxRecords : 0u};
    walk<true>(a, c, fl, s, t, sink);
    uint32_t sv[2] = {t.pads, t.nonEmpty}, mv[1] = {t.longest}, st[2], mt[1];
    block_excl_scan<2, 1>(sv, mv, st, mt, lds);
    if (threadIdx.x == 0) { arr(a, aPads)[blockIdx.x] = st[0]; arr(a, aNonEmpty)[blockIdx.x] = st[1]; arr(a, aLongest)[blockIdx.x] = mt[0]; }
}

// the records the tables hold (0 where the range was refused or holds more records than max_records)
__device__ __forceinline__ uint32_t table_records(const TargetsArgs& a)
{
    const uint32_t recs = a.ws[hRecs];
    return (a.ws[hOffence] == kNone && recs <= a.maxRecords) ? recs : 0u;
}

__global__ __launch_bounds__(kQBlock) void targets_sums_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    const uint32_t recs = table_records(a);
    if (blockIdx.x * kQBlock >= recs) return;
    const uint32_t r = blockIdx.x * kQBlock + threadIdx.x;
    uint32_t sv[1] = {r < recs ? pad4(rec_len(a)[r]) : 0u}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    if (threadIdx.x == 0) rec_blocks(a)[blockIdx.x] = st[0];
}

// ONE block: the tiles' values become what lies in front of each tile; the totals go to the head of the workspace.
// STAGE 1: the file table's verdict, layer 1.  STAGE 2: layer 2, the first offence and its file.  STAGE 3: the padding, the record
// blocks' places, the verdict, status.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void targets_scan_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[3 * kWaves];
    const uint32_t t = threadIdx.x;
    if (STAGE == 1) {
        uint32_t bad = kNone;
        for (uint32_t j = t; j < a.tabBlocks; j += kBlock) bad = min(bad, tab_blocks(a)[j]);
        bad = block_min(bad, lds);
        uint32_t lastLine = 0;
        for (uint32_t base = 0; base < a.tiles; base += kBlock) {                // (the same trips for every thread)
            const uint32_t j = base + t;
            const bool in = j < a.tiles;
            uint32_t s0[1] = {0}, mv[1] = {in ? arr(a, aLastLine)[j] : 0u}, s0t[1], mt[1];
            block_excl_scan<1, 1>(s0, mv, s0t, mt, lds);
            if (in) arr(a, aLastLine)[j] = max(lastLine, mv[0]);
            lastLine = max(lastLine, mt[0]);
        }
        if (t == 0) a.ws[hTabBad] = bad;
    }
    if (STAGE == 2) {
        const uint32_t tabBad = a.ws[hTabBad];
        uint32_t recs = 0, S = 0, recAt = 0, offence = kNone;
        if (tabBad == kNone)
            for (uint32_t base = 0; base < a.tiles; base += kBlock) {
                const uint32_t j = base + t;
                const bool in = j < a.tiles;
                uint32_t sv[2] = {in ? arr(a, aRecs)[j] : 0u, in ? arr(a, aSeq)[j] : 0u}, m0[1] = {0}, st[2], m0t[1];
                block_excl_scan<2, 1>(sv, m0, st, m0t, lds);
                const uint32_t recB = recs + sv[0], seqB = S + sv[1];
                const uint32_t ra = in ? arr(a, aRecAt)[j] : 0u;
                uint32_t s0[1] = {0}, av[1] = {ra ? seqB + ra - 1 : 0u}, s0t[1], at[1];
                block_excl_scan<1, 1>(s0, av, s0t, at, lds);
                if (in) {
                    offence = min(offence, arr(a, aOffence)[j]);
                    arr(a, aRecs)[j] = recB; arr(a, aSeq)[j] = seqB; arr(a, aRecAt)[j] = max(recAt, av[0]);
                }
                recs += st[0]; S += st[1]; recAt = max(recAt, at[0]);
            }
        offence = block_min(offence, lds);
        if (t == 0) {
            uint32_t file = 0;
            if (tabBad != kNone) { offence = a.n; file = tabBad; }
            else if (offence != kNone) file = lower_row(a, (uint64_t)offence + 1, 0, a.numFiles + 1) - 1u;   // (the last row that is not above the offence)
            a.ws[hRecs] = recs; a.ws[hSeq] = S; a.ws[hOffence] = offence; a.ws[hOffFile] = file;
        }
    }
    if (STAGE == 3) {
        const uint32_t offence = a.ws[hOffence], recs = a.ws[hRecs];
        uint32_t pads = 0, nonEmpty = 0, longest = 0;
        if (offence == kNone) {
            for (uint32_t j = t; j < a.tiles; j += kBlock) { pads += arr(a, aPads)[j]; nonEmpty += arr(a, aNonEmpty)[j]; longest = max(longest, arr(a, aLongest)[j]); }
            uint32_t sv[2] = {pads, nonEmpty}, mv[1] = {longest}, st[2], mt[1];
            block_excl_scan<2, 1>(sv, mv, st, mt, lds);
            pads = st[0]; nonEmpty = st[1]; longest = mt[0];
            const uint32_t nb = blocks_of(table_records(a));
            uint32_t inFront = 0;
            for (uint32_t base = 0; base < nb; base += kBlock) {                  // (the same trips for every thread; a trip: kBlock * kQBlock records)
                const uint32_t j = base + t;
                const bool in = j < nb;
                uint32_t bv[1] = {in ? rec_blocks(a)[j] : 0u}, m0[1] = {0}, bt[1], m0t[1];
                block_excl_scan<1, 1>(bv, m0, bt, m0t, lds);
                if (in) rec_blocks(a)[j] = inFront + bv[0];
                inFront += bt[0];
            }
        }
        if (t == 0) {
            const uint64_t seqNeed = (uint64_t)a.ws[hSeq] + pads + 16;
            uint32_t verdict = MC_PARSE_OK;
            if (offence != kNone) verdict = MC_PARSE_IRREGULAR;
            else if (recs > a.maxRecords || seqNeed > a.seqCap) verdict = MC_PARSE_OVERFLOW;
            const bool counted = verdict != MC_PARSE_IRREGULAR;
            a.ws[hPads] = pads; a.ws[hNonEmpty] = nonEmpty; a.ws[hLongest] = longest; a.ws[hVerdict] = verdict; a.ws[hSeqEnd] = (uint32_t)(seqNeed - 16);
            a.status[0] = counted ? recs : 0; a.status[1] = counted ? nonEmpty : 0; a.status[2] = counted ? seqNeed : 0; a.status[3] = 0;
            a.status[4] = verdict; a.status[5] = counted ? 0 : offence; a.status[6] = counted ? longest : 0; a.status[7] = counted ? 0 : a.ws[hOffFile];
            if (verdict == MC_PARSE_OK) atomicAdd(&a.counters[0], (unsigned long long)recs);   // (statistics, no position)
            else atomicAdd(&a.counters[1], 1ull);
        }
    }
}

__global__ __launch_bounds__(kQBlock) void targets_place_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[2 * kWaves];
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const uint32_t recs = a.ws[hRecs];
    if (blockIdx.x * kQBlock >= recs) return;
    const uint32_t r = blockIdx.x * kQBlock + threadIdx.x;
    const uint32_t len = r < recs ? rec_len(a)[r] : 0u;
    uint32_t sv[1] = {pad4(len)}, m0[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, m0, st, mt, lds);
    if (r == 0) {
        const uint32_t end = a.ws[hSeqEnd];
        for (uint32_t k = 0; k < 16; ++k) a.seq[end + k] = 0;
    }
    if (r >= recs) return;
    const uint32_t place = rec_blocks(a)[blockIdx.x] + sv[0], file = rec_file(a)[r];
    for (uint32_t k = len; k < pad4(len); ++k) a.seq[place + k] = 0;
    mc_parse_target tg;
    tg.seq_off = place; tg.len = len; tg.file = file; tg.index = r - (file < a.numFiles ? first_rec(a)[file] : 0u); tg.reserved = 0;
    a.targets[r] = tg;
}

__global__ __launch_bounds__(kBlock) void targets_write_kernel(TargetsArgs a)
{
    __shared__ uint32_t lds[3 * kWaves];
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const uint32_t g = blockIdx.x * kTile + threadIdx.x * 16u;
    const Chunk c = load_chunk(a.B, a.n, 0, g);
    const Files fl = files_of(a, g);
    State s;
    layer1(a, c, fl, s, lds);
    layer2(a, c, fl, s, lds);
    Tally t = empty_tally();
    WriteSink sink{a, kNone, 0u};
    walk<true>(a, c, fl, s, t, sink);
}

uint64_t targets_words(uint64_t nbytes, uint32_t numFiles, uint32_t maxRecords)
{
    return (uint64_t)kHead + (uint64_t)kArrays * tiles_of(nbytes) + blocks_of((uint64_t)numFiles + 1) + 2ull * maxRecords + numFiles + blocks_of(maxRecords);
}

}  // namespace

namespace mcamd {

struct TargetsState {                    // what the context keeps for the MC_PARSE_HOST form of mc_parse_targets
    std::mutex stageMtx;                 // callers take turns at the staging buffers
    DevBuf stageIn, stageOff, stageWs, stageHdr, stageTargets, stageSeq;
    StatusStage status;                  // [8]
};

void free_targets_state(mc_ctx* ctx)
{
    if (!ctx->parseTargets) return;
    TargetsState& S = *ctx->parseTargets;
    free_status_stage(S.status);
    for (DevBuf* b : {&S.stageIn, &S.stageOff, &S.stageWs, &S.stageHdr, &S.stageTargets, &S.stageSeq})
        if (b->p) (void)hipFree(b->p);
    delete ctx->parseTargets;
    ctx->parseTargets = nullptr;
}

}  // namespace mcamd

namespace {

int ensure_targets_state(mc_ctx* ctx, TargetsState** out)
{
    std::lock_guard<std::mutex> lock(ctx->parseTargetsMtx);
    if (!ctx->parseTargets) ctx->parseTargets = new TargetsState;
    TargetsState& S = *ctx->parseTargets;
    *out = &S;
    return make_status_stage(ctx, S.status, 8);
}

// the device form: the table pass, four byte passes, the record layer, three scans; nothing waited for
int enqueue_targets(mc_ctx* ctx, const uint8_t* dBytes, uint32_t n, const uint64_t* dFileOff, uint32_t numFiles, const mc_parse_targets_output& o, void* ws, hipStream_t st)
{
    TargetsArgs a{};
    if (const int rc = count_parse_call(ctx, n, &a.counters)) return rc;
    a.B = dBytes; a.fileOff = dFileOff; a.ws = (uint32_t*)ws;
    a.hdr = o.hdr; a.targets = o.targets; a.seq = o.seq; a.status = o.status; a.seqCap = o.seq_capacity;
    a.n = n; a.tiles = tiles_of(n); a.numFiles = numFiles; a.maxRecords = o.max_records; a.tabBlocks = blocks_of((uint64_t)numFiles + 1);
    const uint32_t recBlocks = blocks_of(o.max_records);
    {
        ScopedTimer timer(ctx, "targets_classify", st);
        hipLaunchKernelGGL(targets_table_kernel, dim3(a.tabBlocks), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(targets_lines_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(targets_scan_kernel<1>, dim3(1), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(targets_classify_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(targets_scan_kernel<2>, dim3(1), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(targets_lengths_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        if (recBlocks) hipLaunchKernelGGL(targets_sums_kernel, dim3(recBlocks), dim3(kQBlock), 0, st, a);
        hipLaunchKernelGGL(targets_scan_kernel<3>, dim3(1), dim3(kBlock), 0, st, a);
    }
    if (recBlocks) {
        ScopedTimer timer(ctx, "targets_write", st);
        hipLaunchKernelGGL(targets_place_kernel, dim3(recBlocks), dim3(kQBlock), 0, st, a);
        hipLaunchKernelGGL(targets_write_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

}  // namespace

extern "C" {

uint64_t mc_parse_targets_scratch_bytes(uint64_t nbytes, uint32_t num_files, uint32_t max_records)
{
    return (targets_words(nbytes, num_files, max_records) * 4 + 255) / 256 * 256;
}

int mc_parse_targets(mc_ctx* ctx, const char* bytes, uint64_t nbytes, const uint64_t* file_off, uint32_t num_files, int flags,
                     const mc_parse_targets_output* out, void* workspace, uint64_t workspace_bytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!out) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: no outputs");
    if (flags & ~MC_PARSE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: flags other than MC_PARSE_HOST");
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: no bytes");
    if (nbytes > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: more than 2^31 bytes in one range");
    if (!file_off || num_files == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: no file table");
    if (!out->status) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: no status");
    if (out->max_records > 0 && (!out->hdr || !out->targets)) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: null array");
    if (out->seq_capacity > 0 && !out->seq) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: a capacity without its array");
    const bool host = (flags & MC_PARSE_HOST) != 0;
    const uint64_t wsNeed = mc_parse_targets_scratch_bytes(nbytes, num_files, out->max_records);
    if (host) {
        bool ok = file_off[0] == 0 && file_off[num_files] == nbytes;
        for (uint32_t f = 0; ok && f < num_files; ++f) ok = file_off[f] < file_off[f + 1];
        if (!ok) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: the file table does not begin at 0, ascend strictly and end at nbytes");
    } else {
        if (!workspace || workspace_bytes < wsNeed) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: the workspace is smaller than mc_parse_targets_scratch_bytes");
        if (((uintptr_t)bytes | (uintptr_t)out->seq | (uintptr_t)workspace) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: device arrays must be aligned (bytes, seq, workspace: 16 bytes)");
        if (((uintptr_t)out->targets | (uintptr_t)out->status | (uintptr_t)file_off) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: device arrays must be aligned (targets, status, file_off: 8 bytes)");
        if ((uintptr_t)out->hdr & 3u) return fail(ctx, MC_ERR_INVALID, "mc_parse_targets: device arrays must be aligned (hdr: 4 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_parse_targets: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const uint32_t n = (uint32_t)nbytes;
    if (!host) return enqueue_targets(ctx, (const uint8_t*)bytes, n, file_off, num_files, *out, workspace, st);
    // host arrays: through the staging buffers, one caller at a time; outputs leave the device only with the verdict MC_PARSE_OK
    TargetsState* S = nullptr;
    int rc = ensure_targets_state(ctx, &S);
    if (rc) return rc;
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t mr = out->max_records, seqRoom = std::min<uint64_t>(out->seq_capacity, nbytes + num_files + 16);   // (no range needs more: padding
    // exceeds what a record's '>' and line ends give back only for a file's LAST record, where the final '\n' may be missing: by one byte)
    if ((rc = grow(ctx, S->stageWs, wsNeed)) != MC_OK || (rc = grow(ctx, S->stageOff, ((uint64_t)num_files + 1) * 8)) != MC_OK ||
        (rc = grow(ctx, S->stageHdr, std::max<uint64_t>(mr * 8, 16))) != MC_OK || (rc = grow(ctx, S->stageTargets, std::max<uint64_t>(mr * sizeof(mc_parse_target), 16))) != MC_OK ||
        (rc = grow(ctx, S->stageSeq, std::max<uint64_t>(seqRoom, 16))) != MC_OK || (rc = stage_bytes(ctx, S->stageIn, bytes, nbytes, st)) != MC_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(S->stageOff.p, file_off, ((uint64_t)num_files + 1) * 8, hipMemcpyHostToDevice, st));
    mc_parse_targets_output d = *out;
    d.hdr = (uint32_t*)S->stageHdr.p; d.targets = (mc_parse_target*)S->stageTargets.p; d.seq = (uint8_t*)S->stageSeq.p; d.seq_capacity = seqRoom;
    d.status = (uint64_t*)S->status.dev.p;
    if ((rc = enqueue_targets(ctx, (const uint8_t*)S->stageIn.p, n, (const uint64_t*)S->stageOff.p, num_files, d, S->stageWs.p, st)) != MC_OK) return rc;
    if ((rc = read_status(ctx, S->status, 8, out->status, st)) != MC_OK) return rc;
    if (out->status[4] != MC_PARSE_OK) return MC_OK;
    const uint64_t recs = out->status[0];
    HIP_TRY(ctx, hipMemcpyAsync(out->hdr, d.hdr, recs * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->targets, d.targets, recs * sizeof(mc_parse_target), hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->seq, d.seq, out->status[2], hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MC_OK;
}

}  // extern "C"
