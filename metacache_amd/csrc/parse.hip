// metacache_amd/csrc/parse.hip -- mc_parse_records / mc_parse_scratch_bytes / mc_parse_stats: a byte range of FASTA or FASTQ records cut
// into reads on the device.  The record rule is the one of include/metacache_amd.h (sequence_reader::read_next,
// sequence_io.cpp:160-236, for regular input); whatever this file cannot decide inside its rule it REFUSES (MC_PARSE_IRREGULAR).
//
// Everything is a prefix over the BYTES.  A tile is kTile consecutive bytes, a block owns a tile, a thread 16 consecutive bytes of it
// (one 16-byte load).  Along the bytes run
//     sums : line starts, record starts, sequence bytes kept (S), name bytes kept (N), padding behind finished sequences (P)
//     maxes: the last line start, the last blank, S at the last record start, S at the last query start
// and with them every output has its place: sequence byte -> seq[S + P], name byte -> names[N], record r -> qinfo from S at its two ends.
// What a byte IS depends on the sums in front of it (its line's kind), so the passes are layered:
//   1. parse_lines_kernel    per tile: line starts, last line start, last blank                 -> parse_scan_kernel<1>
//   2. parse_classify_kernel per tile: records, S, N (by record parity), first offence          -> parse_scan_kernel<2> (+ the verdict so far)
//   3. parse_pads_kernel     per tile: padding, longest len1 + len2                             -> parse_scan_kernel<3> (+ capacities, status)
//   4. parse_write_kernel    per tile: seq, names, name_off, hdr, qinfo
//   5. parse_queries_kernel  per query: max_win, the ends of name_off and seq
// parse_scan_kernel is ONE block that turns the tile values into what lies in front of each tile.  No atomic decides a position: the same
// bytes give the same outputs.  The five byte passes read the input once each: this is built to be right, not yet to be fast (7h).
// mc_parse_mates (two ranges, query q = record q of each) runs layers 1 and 2 per range and adds a layer per RECORD: see "mates" below.
// Plain HIP C++; no inline assembly.
#include "parse_scan.h"

#include <atomic>
#include <cstring>

using namespace mcamd;
using namespace mcamd::parsek;

namespace {

constexpr int kAllFlags = MC_PARSE_HOST | MC_PARSE_PAIRS;
// the workspace, in 32-bit words: kHead words, then kArrays arrays of one word per tile
constexpr uint32_t kHead = 32, kArrays = 13;
enum { hLines = 0, hRecs, hSeq, hNames, hOffence, hPads, hLongest, hVerdict };
enum { aLines = 0, aLastLine, aLastBlank, aRecs, aSeq, aName0, aName1, aOffence, aRecAt, aQueryAt0, aQueryAt1, aPads, aLongest };

struct ParseArgs {
    const uint8_t* B;
    uint32_t* ws;
    uint32_t* hdr; uint32_t* qinfo; uint8_t* seq; uint8_t* names; uint64_t* nameOff; uint32_t* maxWin; uint64_t* status;
    unsigned long long* counters;            // the context's: records, refused ranges
    uint64_t seqCap, namesCap, insertMax;
    uint32_t n, tiles, pairs, maxRecords, stride;
};

__device__ __forceinline__ uint32_t* arr(const ParseArgs& a, uint32_t which) { return a.ws + kHead + (uint64_t)which * a.tiles; }

// ---- a thread's 16 bytes: the Chunk of parse_scan.h with shift 0 (g: the position of its first byte, hi: how many of them the range holds)
// layer 1, which needs nothing in front of it: line starts, the last line start + 1, the last blank + 1 (0: none)
__device__ __forceinline__ void chunk_lines(const Chunk& c, uint32_t& lines, uint32_t& lastLine, uint32_t& lastBlank)
{
    lines = 0; lastLine = 0; lastBlank = 0;
    uint32_t prev = c.prev;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k >= c.hi) continue;
        const uint32_t p = c.g + k, ch = CHUNK_BYTE(c, k);
        if (p == 0 || prev == '\n') { ++lines; lastLine = p + 1; }
        if (ch == ' ') lastBlank = p + 1;
        prev = ch;
    }
}

// what runs along the bytes (in front of the byte the walk stands at)
struct State {
    uint32_t lines, lastLine, lastBlank;     // layer 1
    uint32_t recs, S, N;                     // record starts, sequence bytes, name bytes
    uint32_t recAt, queryAt;                 // S at the last record start, at the last query start
    uint32_t P;                              // padding behind the sequences of the records that have ended
};
// what a RELATIVE walk (nothing of layer 2 known in front of the thread: recs and S count from 0) leaves for the scans
struct Tally {
    uint32_t name0, name1;                   // name bytes of the records by local number li (the record starts of the walk up to the byte): name<li & 1>
    uint32_t recAt, queryAt0, queryAt1;      // S + 1 at the last record start of the walk (0: none); the same by li & 1
    uint32_t offence;                        // the first byte that breaks the rule (kNone: none)
    uint32_t pads, longest;                  // ABSOLUTE walks: padding added, longest len1 + len2 among the queries that ended
};

struct NoSink {
    __device__ __forceinline__ void seq_byte(uint32_t, uint32_t) {}
    __device__ __forceinline__ void name_byte(uint32_t, uint32_t) {}
    __device__ __forceinline__ void query_start(uint32_t, uint32_t) {}
    __device__ __forceinline__ void header(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void record(uint32_t, uint32_t, uint32_t, uint32_t, bool) {}
};
struct WriteSink {
    const ParseArgs& a;
    __device__ __forceinline__ void seq_byte(uint32_t at, uint32_t ch) { a.seq[at] = (uint8_t)ch; }
    __device__ __forceinline__ void name_byte(uint32_t at, uint32_t ch) { a.names[at] = (uint8_t)ch; }
    __device__ __forceinline__ void query_start(uint32_t q, uint32_t N) { a.nameOff[q] = N; }
    __device__ __forceinline__ void header(uint32_t r, uint32_t off, uint32_t len) { a.hdr[2ull * r] = off; a.hdr[2ull * r + 1] = len; }
    __device__ __forceinline__ void record(uint32_t r, uint32_t off, uint32_t len, uint32_t pad, bool last)
    {
        for (uint32_t k = 0; k < pad; ++k) a.seq[off + len + k] = 0;
        uint32_t* q = a.qinfo + 4ull * (a.pairs ? r >> 1 : r);
        if (a.pairs && (r & 1u)) { q[2] = off; q[3] = len; return; }
        q[0] = off; q[1] = len;
        if (!a.pairs || last) { q[2] = off + len + pad; q[3] = 0; }             // (as mc_batch_add leaves a single read: the second mate begins behind the first, with no byte)
    }
};

// a record has ended with S sequence bytes in front of the walk (ABSOLUTE walks only)
template <class Sink>
__device__ __forceinline__ void close_record(const ParseArgs& a, State& s, Tally& t, Sink& sink, bool last)
{
    const uint32_t r = s.recs - 1, len = s.S - s.recAt, pad = (0u - len) & 3u;
    sink.record(r, s.recAt + s.P, len, pad, last);
    if (!a.pairs || (r & 1u) || last) t.longest = max(t.longest, s.S - s.queryAt);
    s.P += pad;
    t.pads += pad;
}

// the one walk over a thread's bytes.  ABS: s holds the true values in front of the thread; otherwise only layer 1 is true and recs, S
// count from 0 (the kind of a line needs no more than layer 1).
template <bool ABS, class Sink>
__device__ __forceinline__ void walk(const ParseArgs& a, const Chunk& c, bool fastq, State& s, Tally& t, Sink& sink)
{
    bool hdr = false, seq = false;                                               // the kind of the line the walk stands in
    if (s.lastLine) {
        if (fastq) { const uint32_t ph = (s.lines - 1) & 3u; hdr = ph == 0; seq = ph == 1; }
        else { hdr = a.B[s.lastLine - 1] == '>'; seq = !hdr; }
    }
    uint32_t prev = c.prev;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k >= c.hi) continue;
        const uint32_t p = c.g + k, ch = CHUNK_BYTE(c, k);
        const uint32_t nx = k == 15 ? c.next : (k + 1 < c.hi ? CHUNK_BYTE(c, (k + 1) & 15u) : (uint32_t)'\n');
        if (p == 0 || prev == '\n') {
            ++s.lines; s.lastLine = p + 1;
            bool bad;
            if (fastq) {
                const uint32_t ph = (s.lines - 1) & 3u;
                hdr = ph == 0; seq = ph == 1;
                bad = ph == 0 ? ch != '@' : ph == 1 ? (ch == '+' || ch == '>' || ch == '\n' || ch == '\r') : ph == 2 ? ch != '+' : false;
            } else { hdr = ch == '>'; seq = !hdr; bad = ch == '+'; }
            if (bad) t.offence = min(t.offence, p);
            if (hdr) {
                if (ABS && s.recs) close_record(a, s, t, sink, false);
                ++s.recs;
                s.recAt = s.S; t.recAt = s.S + 1;
                if (s.recs & 1u) t.queryAt1 = s.S + 1; else t.queryAt0 = s.S + 1;
                if (ABS && (!a.pairs || (s.recs & 1u))) { s.queryAt = s.S; sink.query_start(a.pairs ? (s.recs - 1) >> 1 : s.recs - 1, s.N); }
            }
        }
        const bool kept = ch != '\n' && !(ch == '\r' && nx == '\n');
        if (ch == '\r' && nx != '\n') t.offence = min(t.offence, p);            // a '\r' that does not end its line: not decided here, refused
        if (seq && kept) { sink.seq_byte(s.S + s.P, ch); ++s.S; }
        if (ch == ' ') s.lastBlank = p + 1;
        if (hdr && p + 1 > s.lastLine && kept && !(s.lastBlank > s.lastLine)) {   // a byte of the header in front of its first blank
            if (ABS) { if (!a.pairs || (s.recs & 1u)) { sink.name_byte(s.N, ch); ++s.N; } }
            else if (s.recs & 1u) ++t.name1; else ++t.name0;
        }
        const bool rangeEnds = p + 1 == a.n;
        if (hdr && (ch == '\n' || rangeEnds)) {
            const uint32_t te = ch == '\n' ? p - (prev == '\r' ? 1u : 0u) : a.n - (ch == '\r' ? 1u : 0u);
            sink.header(s.recs - 1, s.lastLine, te - s.lastLine);
        }
        if (ABS && rangeEnds && s.recs) close_record(a, s, t, sink, true);
        prev = ch;
    }
}

__device__ __forceinline__ Tally empty_tally() { Tally t; t.name0 = t.name1 = 0; t.recAt = 0; t.queryAt0 = t.queryAt1 = 0; t.offence = kNone; t.pads = 0; t.longest = 0; return t; }

// which of a relative walk's two parity classes are the FIRST records of their queries, given the record starts in front of the walk:
// local number li has true number recs + li - 1, even where (recs + li) is odd
__device__ __forceinline__ uint32_t first_class(uint32_t recsInFront) { return 1u - (recsInFront & 1u); }

// layer 1 for the block: s.lines / lastLine / lastBlank in front of the thread (the tile's own come from parse_scan_kernel<1>)
__device__ __forceinline__ void layer1(const ParseArgs& a, const Chunk& c, State& s, uint32_t* lds)
{
    uint32_t sv[1], mv[2], st[1], mt[2];
    chunk_lines(c, sv[0], mv[0], mv[1]);
    block_excl_scan<1, 2>(sv, mv, st, mt, lds);
    s.lines = arr(a, aLines)[blockIdx.x] + sv[0];
    s.lastLine = max(arr(a, aLastLine)[blockIdx.x], mv[0]);
    s.lastBlank = max(arr(a, aLastBlank)[blockIdx.x], mv[1]);
    s.recs = s.S = s.N = s.recAt = s.queryAt = s.P = 0;
}

// layer 2 for the block: the relative walk, then recs / S / N / recAt / queryAt in front of the thread (the tile's own from parse_scan_kernel<2>)
__device__ __forceinline__ void layer2(const ParseArgs& a, const Chunk& c, bool fastq, State& s, uint32_t* lds)
{
    State r = s;
    Tally t = empty_tally();
    NoSink none;
    walk<false>(a, c, fastq, r, t, none);
    uint32_t sv[2] = {r.recs, r.S}, st[2], m0[1] = {0}, m0t[1];
    block_excl_scan<2, 1>(sv, m0, st, m0t, lds);
    s.recs = arr(a, aRecs)[blockIdx.x] + sv[0];
    s.S = arr(a, aSeq)[blockIdx.x] + sv[1];
    const uint32_t fc = first_class(s.recs);
    uint32_t nv[1] = {a.pairs ? (fc ? t.name1 : t.name0) : t.name0 + t.name1}, nt[1];
    const uint32_t qa = a.pairs ? (fc ? t.queryAt1 : t.queryAt0) : t.recAt;
    uint32_t av[2] = {t.recAt ? s.S + t.recAt - 1 : 0u, qa ? s.S + qa - 1 : 0u}, at[2];
    block_excl_scan<1, 2>(nv, av, nt, at, lds);
    s.N = arr(a, aName0)[blockIdx.x] + nv[0];
    s.recAt = max(arr(a, aRecAt)[blockIdx.x], av[0]);
    s.queryAt = max(arr(a, aQueryAt0)[blockIdx.x], av[1]);
}

__global__ __launch_bounds__(kBlock) void parse_lines_kernel(ParseArgs a)
{
    __shared__ uint32_t lds[3 * kWaves];
    const Chunk c = load_chunk(a.B, a.n, 0, blockIdx.x * kTile + threadIdx.x * 16u);
    uint32_t sv[1], mv[2], st[1], mt[2];
    chunk_lines(c, sv[0], mv[0], mv[1]);
    block_excl_scan<1, 2>(sv, mv, st, mt, lds);
    if (threadIdx.x == 0) { arr(a, aLines)[blockIdx.x] = st[0]; arr(a, aLastLine)[blockIdx.x] = mt[0]; arr(a, aLastBlank)[blockIdx.x] = mt[1]; }
}

__global__ __launch_bounds__(kBlock) void parse_classify_kernel(ParseArgs a)
{
    __shared__ uint32_t lds[8 * kWaves];
    const bool fastq = a.B[0] == '@';
    const Chunk c = load_chunk(a.B, a.n, 0, blockIdx.x * kTile + threadIdx.x * 16u);
    State s;
    layer1(a, c, s, lds);
    Tally t = empty_tally();
    NoSink none;
    walk<false>(a, c, fastq, s, t, none);
    // the tile's sums, and S + 1 at its last record start (by parity class too), S counted from the tile's first byte
    uint32_t sv[2] = {s.recs, s.S}, m0[1] = {0}, st[2], m0t[1];
    block_excl_scan<2, 1>(sv, m0, st, m0t, lds);
    uint32_t s0[1] = {0}, s0t[1], mv[3] = {t.recAt ? sv[1] + t.recAt : 0u, 0u, 0u}, mt[3];
    // a thread's parity classes are local to it: class k of the thread is class (k + record starts in front of it in the tile) & 1 of the tile
    const uint32_t flip = sv[0] & 1u;
    const uint32_t qc0 = flip ? t.queryAt1 : t.queryAt0, qc1 = flip ? t.queryAt0 : t.queryAt1;
    mv[1] = qc0 ? sv[1] + qc0 : 0u;
    mv[2] = qc1 ? sv[1] + qc1 : 0u;
    block_excl_scan<1, 3>(s0, mv, s0t, mt, lds);
    const uint32_t offence = block_min(t.offence, lds);
    // the name bytes by the TILE's parity classes: the same shift
    uint32_t nv[2] = {flip ? t.name1 : t.name0, flip ? t.name0 : t.name1}, m1[1] = {0}, nt[2], m1t[1];
    block_excl_scan<2, 1>(nv, m1, nt, m1t, lds);
    if (threadIdx.x == 0) {
        arr(a, aRecs)[blockIdx.x] = st[0]; arr(a, aSeq)[blockIdx.x] = st[1];
        arr(a, aName0)[blockIdx.x] = nt[0]; arr(a, aName1)[blockIdx.x] = nt[1];
        arr(a, aOffence)[blockIdx.x] = offence;
        arr(a, aRecAt)[blockIdx.x] = mt[0]; arr(a, aQueryAt0)[blockIdx.x] = mt[1]; arr(a, aQueryAt1)[blockIdx.x] = mt[2];
    }
}

__global__ __launch_bounds__(kBlock) void parse_pads_kernel(ParseArgs a)
{
    __shared__ uint32_t lds[8 * kWaves];
    if (a.ws[hOffence] != kNone) return;
    const bool fastq = a.B[0] == '@';
    const Chunk c = load_chunk(a.B, a.n, 0, blockIdx.x * kTile + threadIdx.x * 16u);
    State s;
    layer1(a, c, s, lds);
    layer2(a, c, fastq, s, lds);
    Tally t = empty_tally();
    NoSink none;
    walk<true>(a, c, fastq, s, t, none);
    uint32_t sv[1] = {t.pads}, mv[1] = {t.longest}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, mv, st, mt, lds);
    if (threadIdx.x == 0) { arr(a, aPads)[blockIdx.x] = st[0]; arr(a, aLongest)[blockIdx.x] = mt[0]; }
}

__global__ __launch_bounds__(kBlock) void parse_write_kernel(ParseArgs a)
{
    __shared__ uint32_t lds[8 * kWaves];
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const bool fastq = a.B[0] == '@';
    const Chunk c = load_chunk(a.B, a.n, 0, blockIdx.x * kTile + threadIdx.x * 16u);
    State s;
    layer1(a, c, s, lds);
    layer2(a, c, fastq, s, lds);
    {
        State r = s;
        Tally t = empty_tally();
        NoSink none;
        walk<true>(a, c, fastq, r, t, none);
        uint32_t sv[1] = {t.pads}, mv[1] = {0}, st[1], mt[1];
        block_excl_scan<1, 1>(sv, mv, st, mt, lds);
        s.P = arr(a, aPads)[blockIdx.x] + sv[0];
    }
    Tally t = empty_tally();
    WriteSink sink{a};
    walk<true>(a, c, fastq, s, t, sink);
}

__global__ __launch_bounds__(kBlock) void parse_queries_kernel(ParseArgs a)
{
    if (a.ws[hVerdict] != MC_PARSE_OK) return;
    const uint32_t recs = a.ws[hRecs], queries = a.pairs ? (recs + 1) / 2 : recs;
    const uint32_t q = blockIdx.x * kBlock + threadIdx.x;
    if (q == 0) {
        a.nameOff[queries] = a.ws[hNames];
        const uint32_t end = a.ws[hSeq] + a.ws[hPads];
        for (uint32_t k = 0; k < 16; ++k) a.seq[end + k] = 0;
    }
    if (q >= queries) return;
    const uint64_t both = (uint64_t)a.qinfo[4ull * q + 1] + a.qinfo[4ull * q + 3];
    a.maxWin[q] = (uint32_t)(2 + max(both, a.insertMax) / a.stride);
}

// ONE block: the tiles' values become what lies in front of each tile; the totals go to the head of the workspace.
// STAGE 1: layer 1.  STAGE 2: layer 2 and the verdict so far.  STAGE 3: the padding, the capacities, status.
template <int STAGE>
__global__ __launch_bounds__(kBlock) void parse_scan_kernel(ParseArgs a)
{
    __shared__ uint32_t lds[8 * kWaves];
    const uint32_t t = threadIdx.x;
    if (STAGE == 1) {
        uint32_t lines = 0, lastLine = 0, lastBlank = 0;
        for (uint32_t base = 0; base < a.tiles; base += kBlock) {                // (the same trips for every thread)
            const uint32_t j = base + t;
            const bool in = j < a.tiles;
            uint32_t sv[1] = {in ? arr(a, aLines)[j] : 0u}, mv[2] = {in ? arr(a, aLastLine)[j] : 0u, in ? arr(a, aLastBlank)[j] : 0u}, st[1], mt[2];
            block_excl_scan<1, 2>(sv, mv, st, mt, lds);
            if (in) { arr(a, aLines)[j] = lines + sv[0]; arr(a, aLastLine)[j] = max(lastLine, mv[0]); arr(a, aLastBlank)[j] = max(lastBlank, mv[1]); }
            lines += st[0]; lastLine = max(lastLine, mt[0]); lastBlank = max(lastBlank, mt[1]);
        }
        if (t == 0) a.ws[hLines] = lines;
    }
    if (STAGE == 2) {
        uint32_t recs = 0, S = 0, N = 0, recAt = 0, queryAt = 0, offence = kNone;
        for (uint32_t base = 0; base < a.tiles; base += kBlock) {
            const uint32_t j = base + t;
            const bool in = j < a.tiles;
            uint32_t sv[2] = {in ? arr(a, aRecs)[j] : 0u, in ? arr(a, aSeq)[j] : 0u}, m0[1] = {0}, st[2], m0t[1];
            block_excl_scan<2, 1>(sv, m0, st, m0t, lds);
            const uint32_t recB = recs + sv[0], seqB = S + sv[1], fc = first_class(recB);
            // (tile class k holds the records of local number li with li & 1 == k; the first records of their queries are class fc)
            const uint32_t n0 = in ? arr(a, aName0)[j] : 0u, n1 = in ? arr(a, aName1)[j] : 0u;
            const uint32_t ra = in ? arr(a, aRecAt)[j] : 0u, q0 = in ? arr(a, aQueryAt0)[j] : 0u, q1 = in ? arr(a, aQueryAt1)[j] : 0u;
            const uint32_t qa = a.pairs ? (fc ? q1 : q0) : ra;
            uint32_t nv[1] = {a.pairs ? (fc ? n1 : n0) : n0 + n1}, av[2] = {ra ? seqB + ra - 1 : 0u, qa ? seqB + qa - 1 : 0u}, nt[1], at[2];
            block_excl_scan<1, 2>(nv, av, nt, at, lds);
            if (in) {
                offence = min(offence, arr(a, aOffence)[j]);
                arr(a, aRecs)[j] = recB; arr(a, aSeq)[j] = seqB; arr(a, aName0)[j] = N + nv[0];
                arr(a, aRecAt)[j] = max(recAt, av[0]); arr(a, aQueryAt0)[j] = max(queryAt, av[1]);
            }
            recs += st[0]; S += st[1]; N += nt[0]; recAt = max(recAt, at[0]); queryAt = max(queryAt, at[1]);
        }
        offence = block_min(offence, lds);
        if (t == 0) {
            const uint32_t first = a.B[0];
            if (first == '@' && (a.ws[hLines] & 3u)) offence = min(offence, a.n);   // an incomplete last group
            if (first != '@' && first != '>') offence = 0;
            a.ws[hRecs] = recs; a.ws[hSeq] = S; a.ws[hNames] = N; a.ws[hOffence] = offence;
        }
    }
    if (STAGE == 3) {
        const uint32_t offence = a.ws[hOffence];
        uint32_t pads = 0, longest = 0;
        if (offence == kNone)
            for (uint32_t base = 0; base < a.tiles; base += kBlock) {
                const uint32_t j = base + t;
                const bool in = j < a.tiles;
                uint32_t sv[1] = {in ? arr(a, aPads)[j] : 0u}, mv[1] = {in ? arr(a, aLongest)[j] : 0u}, st[1], mt[1];
                block_excl_scan<1, 1>(sv, mv, st, mt, lds);
                if (in) arr(a, aPads)[j] = pads + sv[0];
                pads += st[0]; longest = max(longest, mt[0]);
            }
        if (t == 0) {
            const uint32_t recs = a.ws[hRecs];
            const uint64_t seqNeed = (uint64_t)a.ws[hSeq] + pads + 16, nameNeed = a.ws[hNames];
            uint32_t verdict = MC_PARSE_OK;
            if (offence != kNone) verdict = MC_PARSE_IRREGULAR;
            else if (recs > a.maxRecords || seqNeed > a.seqCap || nameNeed > a.namesCap) verdict = MC_PARSE_OVERFLOW;
            a.ws[hPads] = pads; a.ws[hLongest] = longest; a.ws[hVerdict] = verdict;
            a.status[0] = recs; a.status[1] = a.pairs ? (recs + 1) / 2 : recs; a.status[2] = seqNeed; a.status[3] = nameNeed;
            a.status[4] = verdict; a.status[5] = offence == kNone ? 0 : offence; a.status[6] = longest; a.status[7] = (a.pairs && (recs & 1u)) ? 1 : 0;
            if (verdict == MC_PARSE_OK) atomicAdd(&a.counters[0], (unsigned long long)recs);   // (statistics, no position)
            else atomicAdd(&a.counters[1], 1ull);
        }
    }
}

// ---- mates: TWO ranges, query q = record q of the first + record q of the second (mc_parse_mates) --------------------------------------
// Each range is classified on its own by the layers above (lines -> scan<1> -> classify -> scan<2>, no pairing), in a workspace of its
// own.  A mate's place in seq depends on the lengths of all earlier records of BOTH ranges, which no prefix over one range's bytes
// holds, so a layer per RECORD follows:
//   a. mates_lengths_kernel per tile of either range: len[f][r] (the place is the record's number) and the tile's padding
//   b. mates_sums_kernel    per kQBlock queries: the sum of pad4(len1) + pad4(len2), the longest len1 + len2
//      mates_scan_kernel    ONE block: what lies in front of each such block, the verdict, status
//   c. mates_place_kernel   per query: place[f][q], qinfo, max_win, the ends of name_off and seq
//   d. mates_write_kernel   per tile of either range: sequence byte -> seq[place[f][r] + (S - S at the record's start)], hdr; names from range 0
// A block of b./c. takes kQBlock = 256 queries (one a thread); ONE TRIP of mates_scan_kernel takes kBlock such blocks = 65 536 queries,
// and it makes as many trips as the queries need.  No atomic decides a position.
constexpr uint32_t kQBlock = kBlock, kMHead = 32;
enum { mVerdict = 0, mQueries, mSeqEnd, mNames };
enum { tLen0 = 0, tLen1, tPlace0, tPlace1 };

struct MatesArgs {
    ParseArgs f[2];                          // the two ranges (pairs = 0; the outputs, capacities and maxRecords are the call's in both)
    uint32_t* m;                             // kMHead words, four tables of Q words (len, place by range), two of one word per kQBlock queries
    uint32_t Q;                              // rows of a table: max_records / 2
};

__device__ __forceinline__ uint32_t* mtab(const MatesArgs& m, uint32_t which) { return m.m + kMHead + (uint64_t)which * m.Q; }
__host__ __device__ __forceinline__ uint32_t qblocks_of(uint32_t queries) { return (queries + kQBlock - 1) / kQBlock; }
__device__ __forceinline__ uint32_t* mblk(const MatesArgs& m, uint32_t which) { return m.m + kMHead + 4ull * m.Q + (uint64_t)which * qblocks_of(m.Q); }
__device__ __forceinline__ uint32_t pad4(uint32_t len) { return (len + 3u) & ~3u; }

// the verdict as far as the ranges' own layers give it: with MC_PARSE_OK the records of both ranges fit the tables
__device__ __forceinline__ uint32_t mates_so_far(const MatesArgs& m)
{
    if (m.f[0].ws[hOffence] != kNone || m.f[1].ws[hOffence] != kNone) return MC_PARSE_IRREGULAR;
    const uint32_t r0 = m.f[0].ws[hRecs], r1 = m.f[1].ws[hRecs];
    if (r0 != r1) return MC_PARSE_UNEQUAL;
    return (uint64_t)r0 + r1 > m.f[0].maxRecords ? MC_PARSE_OVERFLOW : MC_PARSE_OK;
}

struct LenSink {
    uint32_t* len; uint32_t rows;
    __device__ __forceinline__ void seq_byte(uint32_t, uint32_t) {}
    __device__ __forceinline__ void name_byte(uint32_t, uint32_t) {}
    __device__ __forceinline__ void query_start(uint32_t, uint32_t) {}
    __device__ __forceinline__ void header(uint32_t, uint32_t, uint32_t) {}
    __device__ __forceinline__ void record(uint32_t r, uint32_t, uint32_t l, uint32_t, bool) { if (r < rows) len[r] = l; }
};
// (the walk hands S + P to seq_byte, P being the padding of the records that ended inside this thread's bytes: the walk started with P = 0)
struct MatesSink {
    const ParseArgs& a; const State& s; const uint32_t* place; uint32_t f, curRec, curPlace;
    __device__ __forceinline__ uint32_t place_of(uint32_t r) { if (r != curRec) { curRec = r; curPlace = place[r]; } return curPlace; }
    __device__ __forceinline__ void seq_byte(uint32_t at, uint32_t ch) { a.seq[place_of(s.recs - 1) + (at - s.P - s.recAt)] = (uint8_t)ch; }
    __device__ __forceinline__ void name_byte(uint32_t at, uint32_t ch) { if (!f) a.names[at] = (uint8_t)ch; }
    __device__ __forceinline__ void query_start(uint32_t q, uint32_t N) { if (!f) a.nameOff[q] = N; }
    __device__ __forceinline__ void header(uint32_t r, uint32_t off, uint32_t len) { uint32_t* h = a.hdr + 2ull * (2ull * r + f); h[0] = off; h[1] = len; }
    __device__ __forceinline__ void record(uint32_t r, uint32_t, uint32_t len, uint32_t pad, bool)
    {
        const uint32_t end = place_of(r) + len;
        for (uint32_t k = 0; k < pad; ++k) a.seq[end + k] = 0;
    }
};

__global__ __launch_bounds__(kBlock) void mates_lengths_kernel(MatesArgs m)
{
    __shared__ uint32_t lds[8 * kWaves];
    const ParseArgs& a = m.f[blockIdx.y];
    if (blockIdx.x >= a.tiles) return;
    const uint32_t soFar = mates_so_far(m);
    if (soFar == MC_PARSE_IRREGULAR || soFar == MC_PARSE_UNEQUAL) return;
    const bool fastq = a.B[0] == '@';
    const Chunk c = load_chunk(a.B, a.n, 0, blockIdx.x * kTile + threadIdx.x * 16u);
    State s;
    layer1(a, c, s, lds);
    layer2(a, c, fastq, s, lds);
    Tally t = empty_tally();
    LenSink sink{mtab(m, tLen0 + blockIdx.y), soFar == MC_PARSE_OK ? m.Q : 0u};
    walk<true>(a, c, fastq, s, t, sink);
    uint32_t sv[1] = {t.pads}, mv[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, mv, st, mt, lds);
    if (threadIdx.x == 0) arr(a, aPads)[blockIdx.x] = st[0];
}

__global__ __launch_bounds__(kQBlock) void mates_sums_kernel(MatesArgs m)
{
    __shared__ uint32_t lds[2 * kWaves];
    if (mates_so_far(m) != MC_PARSE_OK) return;
    const uint32_t queries = m.f[0].ws[hRecs];
    if (blockIdx.x * kQBlock >= queries) return;
    const uint32_t q = blockIdx.x * kQBlock + threadIdx.x;
    const uint32_t l0 = q < queries ? mtab(m, tLen0)[q] : 0u, l1 = q < queries ? mtab(m, tLen1)[q] : 0u;
    uint32_t sv[1] = {pad4(l0) + pad4(l1)}, mv[1] = {l0 + l1}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, mv, st, mt, lds);
    if (threadIdx.x == 0) { mblk(m, 0)[blockIdx.x] = st[0]; mblk(m, 1)[blockIdx.x] = mt[0]; }
}

// ONE block: the tiles' padding summed, the query blocks' sums turned into what lies in front of each, the verdict, status
__global__ __launch_bounds__(kBlock) void mates_scan_kernel(MatesArgs m)
{
    __shared__ uint32_t lds[2 * kWaves];
    const uint32_t t = threadIdx.x, soFar = mates_so_far(m);
    const uint32_t r0 = m.f[0].ws[hRecs], r1 = m.f[1].ws[hRecs];
    uint32_t pads = 0, longest = 0;
    if (soFar == MC_PARSE_OK || soFar == MC_PARSE_OVERFLOW) {
        uint32_t mine = 0;
#pragma unroll
        for (uint32_t f = 0; f < 2; ++f)
            for (uint32_t j = t; j < m.f[f].tiles; j += kBlock) mine += arr(m.f[f], aPads)[j];
        uint32_t sv[1] = {mine}, mv[1] = {0}, st[1], mt[1];
        block_excl_scan<1, 1>(sv, mv, st, mt, lds);
        pads = st[0];
    }
    if (soFar == MC_PARSE_OK) {
        const uint32_t nb = qblocks_of(r0);
        uint32_t inFront = 0;
        for (uint32_t base = 0; base < nb; base += kBlock) {                      // (the same trips for every thread; a trip: kBlock * kQBlock queries)
            const uint32_t j = base + t;
            const bool in = j < nb;
            uint32_t sv[1] = {in ? mblk(m, 0)[j] : 0u}, mv[1] = {in ? mblk(m, 1)[j] : 0u}, st[1], mt[1];
            block_excl_scan<1, 1>(sv, mv, st, mt, lds);
            if (in) mblk(m, 0)[j] = inFront + sv[0];
            inFront += st[0]; longest = max(longest, mt[0]);
        }
    }
    if (t == 0) {
        const ParseArgs& a = m.f[0];
        const uint32_t off0 = a.ws[hOffence], off1 = m.f[1].ws[hOffence];
        const uint64_t seqNeed = (uint64_t)a.ws[hSeq] + m.f[1].ws[hSeq] + pads + 16, nameNeed = a.ws[hNames];
        uint32_t verdict = soFar;
        if (verdict == MC_PARSE_OK && (seqNeed > a.seqCap || nameNeed > a.namesCap)) verdict = MC_PARSE_OVERFLOW;
        m.m[mVerdict] = verdict; m.m[mQueries] = r0; m.m[mSeqEnd] = (uint32_t)(seqNeed - 16); m.m[mNames] = (uint32_t)nameNeed;
        const bool counted = verdict != MC_PARSE_IRREGULAR;
        a.status[0] = counted ? (uint64_t)r0 + r1 : 0; a.status[1] = counted ? min(r0, r1) : 0;
        a.status[2] = counted ? seqNeed : 0; a.status[3] = counted ? nameNeed : 0;
        a.status[4] = verdict; a.status[5] = counted ? 0 : (off0 != kNone ? off0 : off1); a.status[6] = longest;
        a.status[7] = (!counted && off0 == kNone) ? 1 : 0;
        a.status[8] = counted ? r0 : 0; a.status[9] = counted ? r1 : 0;
        if (verdict == MC_PARSE_OK) atomicAdd(&a.counters[0], (unsigned long long)r0 + r1);   // (statistics, no position)
        else atomicAdd(&a.counters[1], 1ull);
    }
}

__global__ __launch_bounds__(kQBlock) void mates_place_kernel(MatesArgs m)
{
    __shared__ uint32_t lds[2 * kWaves];
    if (m.m[mVerdict] != MC_PARSE_OK) return;
    const ParseArgs& a = m.f[0];
    const uint32_t queries = m.m[mQueries];
    if (blockIdx.x * kQBlock >= queries) return;
    const uint32_t q = blockIdx.x * kQBlock + threadIdx.x;
    const uint32_t l0 = q < queries ? mtab(m, tLen0)[q] : 0u, l1 = q < queries ? mtab(m, tLen1)[q] : 0u;
    uint32_t sv[1] = {pad4(l0) + pad4(l1)}, mv[1] = {0}, st[1], mt[1];
    block_excl_scan<1, 1>(sv, mv, st, mt, lds);
    if (q == 0) {
        a.nameOff[queries] = m.m[mNames];
        const uint32_t end = m.m[mSeqEnd];
        for (uint32_t k = 0; k < 16; ++k) a.seq[end + k] = 0;
    }
    if (q >= queries) return;
    const uint32_t p0 = mblk(m, 0)[blockIdx.x] + sv[0], p1 = p0 + pad4(l0);
    mtab(m, tPlace0)[q] = p0; mtab(m, tPlace1)[q] = p1;
    uint32_t* qi = a.qinfo + 4ull * q;
    qi[0] = p0; qi[1] = l0; qi[2] = p1; qi[3] = l1;
    a.maxWin[q] = (uint32_t)(2 + max((uint64_t)l0 + l1, a.insertMax) / a.stride);
}

__global__ __launch_bounds__(kBlock) void mates_write_kernel(MatesArgs m)
{
    __shared__ uint32_t lds[8 * kWaves];
    const ParseArgs& a = m.f[blockIdx.y];
    if (blockIdx.x >= a.tiles || m.m[mVerdict] != MC_PARSE_OK) return;
    const bool fastq = a.B[0] == '@';
    const Chunk c = load_chunk(a.B, a.n, 0, blockIdx.x * kTile + threadIdx.x * 16u);
    State s;
    layer1(a, c, s, lds);
    layer2(a, c, fastq, s, lds);
    Tally t = empty_tally();
    MatesSink sink{a, s, mtab(m, tPlace0 + blockIdx.y), blockIdx.y, kNone, 0u};
    walk<true>(a, c, fastq, s, t, sink);
}

uint64_t mates_words(uint32_t maxRecords) { const uint32_t Q = maxRecords / 2; return (uint64_t)kMHead + 4ull * Q + 2ull * qblocks_of(Q); }

}  // namespace

namespace mcamd {

struct ParseState {                      // what the context keeps for mc_parse_*
    unsigned long long* dCounters = nullptr;   // records parsed, ranges refused
    std::atomic<uint64_t> calls{0}, bytes{0};
    std::mutex stageMtx;                 // MC_PARSE_HOST callers take turns at the staging buffers
    DevBuf stageIn, stageWs, stageHdr, stageQinfo, stageSeq, stageNames, stageNameOff, stageMaxWin;
    StatusStage status;                  // [16]: mc_parse_records reads 8 words, mc_parse_mates 10
};

void free_parse_state(mc_ctx* ctx)
{
    if (!ctx->parse) return;
    ParseState& S = *ctx->parse;
    if (S.dCounters) (void)hipFree(S.dCounters);
    free_status_stage(S.status);
    for (DevBuf* b : {&S.stageIn, &S.stageWs, &S.stageHdr, &S.stageQinfo, &S.stageSeq, &S.stageNames, &S.stageNameOff, &S.stageMaxWin})
        if (b->p) (void)hipFree(b->p);
    delete ctx->parse;
    ctx->parse = nullptr;
}

}  // namespace mcamd

namespace {

int ensure_parse_state(mc_ctx* ctx, ParseState** out)
{
    std::lock_guard<std::mutex> lock(ctx->parseMtx);
    if (!ctx->parse) ctx->parse = new ParseState;
    ParseState& S = *ctx->parse;
    *out = &S;
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, 16));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, 16));
    }
    return make_status_stage(ctx, S.status, 16);
}

}  // namespace

namespace mcamd {

int count_parse_call(mc_ctx* ctx, uint64_t bytes, unsigned long long** counters)
{
    ParseState* S = nullptr;
    if (const int rc = ensure_parse_state(ctx, &S)) return rc;
    ++S->calls; S->bytes += bytes;
    *counters = S->dCounters;
    return MC_OK;
}

}  // namespace mcamd

namespace {

// the device form: five byte passes, three scans, nothing waited for
int enqueue_parse(mc_ctx* ctx, ParseState& S, const uint8_t* dBytes, uint32_t n, int flags, uint64_t insertMax, const mc_parse_output& o, void* ws, hipStream_t st)
{
    ParseArgs a{};
    a.B = dBytes; a.ws = (uint32_t*)ws;
    a.hdr = o.hdr; a.qinfo = o.qinfo; a.seq = o.seq; a.names = (uint8_t*)o.names; a.nameOff = o.name_off; a.maxWin = o.max_win; a.status = o.status;
    a.counters = S.dCounters;
    a.seqCap = o.seq_capacity; a.namesCap = o.names_capacity; a.insertMax = insertMax;
    a.n = n; a.tiles = tiles_of(n); a.pairs = (flags & MC_PARSE_PAIRS) ? 1u : 0u; a.maxRecords = o.max_records;
    a.stride = ctx->targetSketch.stride ? ctx->targetSketch.stride : 1u;
    {
        ScopedTimer timer(ctx, "parse_classify", st);
        hipLaunchKernelGGL(parse_lines_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(parse_scan_kernel<1>, dim3(1), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(parse_classify_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(parse_scan_kernel<2>, dim3(1), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(parse_pads_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(parse_scan_kernel<3>, dim3(1), dim3(kBlock), 0, st, a);
    }
    {
        ScopedTimer timer(ctx, "parse_write", st);
        hipLaunchKernelGGL(parse_write_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
        if (o.max_records) hipLaunchKernelGGL(parse_queries_kernel, dim3((o.max_records + kBlock - 1) / kBlock), dim3(kBlock), 0, st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    ++S.calls; S.bytes += n;
    return MC_OK;
}

// the device form for two ranges: each range's own layers, then the per-record layer; nothing waited for.  ws: range 0's workspace, range
// 1's, the tables (mc_parse_mates_scratch_bytes)
int enqueue_mates(mc_ctx* ctx, ParseState& S, const uint8_t* d1, uint32_t n1, const uint8_t* d2, uint32_t n2, uint64_t insertMax, const mc_parse_output& o, void* ws, hipStream_t st)
{
    MatesArgs m{};
    const uint8_t* B[2] = {d1, d2};
    const uint32_t n[2] = {n1, n2};
    uint8_t* w = (uint8_t*)ws;
    for (int f = 0; f < 2; ++f) {
        ParseArgs& a = m.f[f];
        a.B = B[f]; a.ws = (uint32_t*)w;
        w += mc_parse_scratch_bytes(n[f]);
        a.hdr = o.hdr; a.qinfo = o.qinfo; a.seq = o.seq; a.names = (uint8_t*)o.names; a.nameOff = o.name_off; a.maxWin = o.max_win; a.status = o.status;
        a.counters = S.dCounters;
        a.seqCap = o.seq_capacity; a.namesCap = o.names_capacity; a.insertMax = insertMax;
        a.n = n[f]; a.tiles = tiles_of(n[f]); a.pairs = 0; a.maxRecords = o.max_records;
        a.stride = ctx->targetSketch.stride ? ctx->targetSketch.stride : 1u;
    }
    m.m = (uint32_t*)w; m.Q = o.max_records / 2;
    const dim3 both(std::max(m.f[0].tiles, m.f[1].tiles), 2);
    {
        ScopedTimer timer(ctx, "parse_classify", st);
        for (int f = 0; f < 2; ++f) {
            const ParseArgs& a = m.f[f];
            hipLaunchKernelGGL(parse_lines_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
            hipLaunchKernelGGL(parse_scan_kernel<1>, dim3(1), dim3(kBlock), 0, st, a);
            hipLaunchKernelGGL(parse_classify_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
            hipLaunchKernelGGL(parse_scan_kernel<2>, dim3(1), dim3(kBlock), 0, st, a);
        }
        hipLaunchKernelGGL(mates_lengths_kernel, both, dim3(kBlock), 0, st, m);
        if (m.Q) hipLaunchKernelGGL(mates_sums_kernel, dim3(qblocks_of(m.Q)), dim3(kQBlock), 0, st, m);
        hipLaunchKernelGGL(mates_scan_kernel, dim3(1), dim3(kBlock), 0, st, m);
    }
    if (m.Q) {
        ScopedTimer timer(ctx, "parse_write", st);
        hipLaunchKernelGGL(mates_place_kernel, dim3(qblocks_of(m.Q)), dim3(kQBlock), 0, st, m);
        hipLaunchKernelGGL(mates_write_kernel, both, dim3(kBlock), 0, st, m);
    }
    HIP_TRY(ctx, hipGetLastError());
    ++S.calls; S.bytes += (uint64_t)n1 + n2;
    return MC_OK;
}

}  // namespace

extern "C" {

const uint32_t mc_parse_tile = kTile;

uint64_t mc_parse_scratch_bytes(uint64_t nbytes)
{
    return (((uint64_t)kHead + (uint64_t)kArrays * tiles_of(nbytes)) * 4 + 255) / 256 * 256;
}

int mc_parse_records(mc_ctx* ctx, const char* bytes, uint64_t nbytes, int flags, uint64_t insert_size_max, const mc_parse_output* out,
                     void* workspace, uint64_t workspace_bytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!out) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: no outputs");
    if (flags & ~kAllFlags) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: unknown flag");
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: no bytes");
    if (nbytes > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: more than 2^31 bytes in one range");
    if (!out->status) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: no status");
    if (out->max_records > 0 && (!out->hdr || !out->qinfo || !out->name_off || !out->max_win)) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: null array");
    if ((out->seq_capacity > 0 && !out->seq) || (out->names_capacity > 0 && !out->names)) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: a capacity without its array");
    if (out->seq_capacity > 0xFFFFFFFFull || out->names_capacity > 0xFFFFFFFFull) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: a capacity beyond 32-bit offsets");
    const bool host = (flags & MC_PARSE_HOST) != 0;
    if (host) {
        if (bytes[0] != '>' && bytes[0] != '@') return fail(ctx, MC_ERR_INVALID, "mc_parse_records: the range does not begin with '>' or '@'");
    } else {
        if (!workspace || workspace_bytes < mc_parse_scratch_bytes(nbytes)) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: the workspace is smaller than mc_parse_scratch_bytes");
        if (((uintptr_t)bytes | (uintptr_t)out->seq | (uintptr_t)workspace) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: device arrays must be aligned (bytes, seq, workspace: 16 bytes)");
        if (((uintptr_t)out->name_off | (uintptr_t)out->status) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: device arrays must be aligned (name_off, status: 8 bytes)");
        if (((uintptr_t)out->hdr | (uintptr_t)out->qinfo | (uintptr_t)out->max_win) & 3u) return fail(ctx, MC_ERR_INVALID, "mc_parse_records: device arrays must be aligned (hdr, qinfo, max_win: 4 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_parse_records: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    ParseState* S = nullptr;
    int rc = ensure_parse_state(ctx, &S);
    if (rc) return rc;
    const uint32_t n = (uint32_t)nbytes;
    if (!host) return enqueue_parse(ctx, *S, (const uint8_t*)bytes, n, flags, insert_size_max, *out, workspace, st);
    // host arrays: through the staging buffers, one caller at a time; outputs leave the device only with the verdict MC_PARSE_OK
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t mr = out->max_records;
    if ((rc = grow(ctx, S->stageWs, mc_parse_scratch_bytes(nbytes))) != MC_OK ||
        (rc = grow(ctx, S->stageHdr, std::max<uint64_t>(mr * 8, 16))) != MC_OK || (rc = grow(ctx, S->stageQinfo, std::max<uint64_t>(mr * 16, 16))) != MC_OK ||
        (rc = grow(ctx, S->stageSeq, std::max<uint64_t>(out->seq_capacity, 16))) != MC_OK || (rc = grow(ctx, S->stageNames, std::max<uint64_t>(out->names_capacity, 16))) != MC_OK ||
        (rc = grow(ctx, S->stageNameOff, (mr + 1) * 8)) != MC_OK || (rc = grow(ctx, S->stageMaxWin, std::max<uint64_t>(mr * 4, 16))) != MC_OK ||
        (rc = stage_bytes(ctx, S->stageIn, bytes, nbytes, st)) != MC_OK) return rc;
    mc_parse_output d = *out;
    d.hdr = (uint32_t*)S->stageHdr.p; d.qinfo = (uint32_t*)S->stageQinfo.p; d.seq = (uint8_t*)S->stageSeq.p; d.names = (char*)S->stageNames.p;
    d.name_off = (uint64_t*)S->stageNameOff.p; d.max_win = (uint32_t*)S->stageMaxWin.p; d.status = (uint64_t*)S->status.dev.p;
    if ((rc = enqueue_parse(ctx, *S, (const uint8_t*)S->stageIn.p, n, flags & ~MC_PARSE_HOST, insert_size_max, d, S->stageWs.p, st)) != MC_OK) return rc;
    if ((rc = read_status(ctx, S->status, 8, out->status, st)) != MC_OK) return rc;
    if (out->status[4] != MC_PARSE_OK) return MC_OK;
    const uint64_t recs = out->status[0], queries = out->status[1];
    if (recs) HIP_TRY(ctx, hipMemcpyAsync(out->hdr, d.hdr, recs * 8, hipMemcpyDeviceToHost, st));
    if (queries) {
        HIP_TRY(ctx, hipMemcpyAsync(out->qinfo, d.qinfo, queries * 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipMemcpyAsync(out->max_win, d.max_win, queries * 4, hipMemcpyDeviceToHost, st));
    }
    if (out->max_records) HIP_TRY(ctx, hipMemcpyAsync(out->name_off, d.name_off, (queries + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->seq, d.seq, out->status[2], hipMemcpyDeviceToHost, st));
    if (out->status[3]) HIP_TRY(ctx, hipMemcpyAsync(out->names, d.names, out->status[3], hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MC_OK;
}

uint64_t mc_parse_mates_scratch_bytes(uint64_t n1, uint64_t n2, uint32_t max_records)
{
    return mc_parse_scratch_bytes(n1) + mc_parse_scratch_bytes(n2) + (mates_words(max_records) * 4 + 255) / 256 * 256;
}

int mc_parse_mates(mc_ctx* ctx, const char* bytes1, uint64_t n1, const char* bytes2, uint64_t n2, int flags, uint64_t insert_size_max,
                   const mc_parse_output* out, void* workspace, uint64_t workspace_bytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!out) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: no outputs");
    if (flags & ~MC_PARSE_HOST) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: flags other than MC_PARSE_HOST (the ranges ARE the pairing)");
    if (!bytes1 || !bytes2 || n1 == 0 || n2 == 0) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: no bytes");
    if (n1 > (1ull << 31) || n2 > (1ull << 31) || n1 + n2 > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: more than 2^31 bytes in the two ranges");
    if (!out->status) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: no status");
    if (out->max_records > 0 && (!out->hdr || !out->qinfo || !out->name_off || !out->max_win)) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: null array");
    if ((out->seq_capacity > 0 && !out->seq) || (out->names_capacity > 0 && !out->names)) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: a capacity without its array");
    if (out->seq_capacity > 0xFFFFFFFFull || out->names_capacity > 0xFFFFFFFFull) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: a capacity beyond 32-bit offsets");
    const bool host = (flags & MC_PARSE_HOST) != 0;
    const uint64_t wsNeed = mc_parse_mates_scratch_bytes(n1, n2, out->max_records);
    if (host) {
        if ((bytes1[0] != '>' && bytes1[0] != '@') || (bytes2[0] != '>' && bytes2[0] != '@')) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: a range does not begin with '>' or '@'");
    } else {
        if (!workspace || workspace_bytes < wsNeed) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: the workspace is smaller than mc_parse_mates_scratch_bytes");
        if (((uintptr_t)bytes1 | (uintptr_t)bytes2 | (uintptr_t)out->seq | (uintptr_t)workspace) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: device arrays must be aligned (bytes1, bytes2, seq, workspace: 16 bytes)");
        if (((uintptr_t)out->name_off | (uintptr_t)out->status) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: device arrays must be aligned (name_off, status: 8 bytes)");
        if (((uintptr_t)out->hdr | (uintptr_t)out->qinfo | (uintptr_t)out->max_win) & 3u) return fail(ctx, MC_ERR_INVALID, "mc_parse_mates: device arrays must be aligned (hdr, qinfo, max_win: 4 bytes)");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_parse_mates: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    ParseState* S = nullptr;
    int rc = ensure_parse_state(ctx, &S);
    if (rc) return rc;
    if (!host) return enqueue_mates(ctx, *S, (const uint8_t*)bytes1, (uint32_t)n1, (const uint8_t*)bytes2, (uint32_t)n2, insert_size_max, *out, workspace, st);
    // host arrays: through the staging buffers, one caller at a time (range 2 behind range 1, at a multiple of 16); outputs leave the
    // device only with the verdict MC_PARSE_OK
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t mr = out->max_records, at2 = (n1 + 15) / 16 * 16;
    if ((rc = grow(ctx, S->stageIn, at2 + (n2 + 15) / 16 * 16)) != MC_OK || (rc = grow(ctx, S->stageWs, wsNeed)) != MC_OK ||
        (rc = grow(ctx, S->stageHdr, std::max<uint64_t>(mr * 8, 16))) != MC_OK || (rc = grow(ctx, S->stageQinfo, std::max<uint64_t>(mr * 16, 16))) != MC_OK ||
        (rc = grow(ctx, S->stageSeq, std::max<uint64_t>(out->seq_capacity, 16))) != MC_OK || (rc = grow(ctx, S->stageNames, std::max<uint64_t>(out->names_capacity, 16))) != MC_OK ||
        (rc = grow(ctx, S->stageNameOff, (mr + 1) * 8)) != MC_OK || (rc = grow(ctx, S->stageMaxWin, std::max<uint64_t>(mr * 4, 16))) != MC_OK) return rc;
    uint8_t* in = (uint8_t*)S->stageIn.p;
    HIP_TRY(ctx, hipMemcpyAsync(in, bytes1, n1, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(in + at2, bytes2, n2, hipMemcpyHostToDevice, st));
    mc_parse_output d = *out;
    d.hdr = (uint32_t*)S->stageHdr.p; d.qinfo = (uint32_t*)S->stageQinfo.p; d.seq = (uint8_t*)S->stageSeq.p; d.names = (char*)S->stageNames.p;
    d.name_off = (uint64_t*)S->stageNameOff.p; d.max_win = (uint32_t*)S->stageMaxWin.p; d.status = (uint64_t*)S->status.dev.p;
    if ((rc = enqueue_mates(ctx, *S, in, (uint32_t)n1, in + at2, (uint32_t)n2, insert_size_max, d, S->stageWs.p, st)) != MC_OK) return rc;
    if ((rc = read_status(ctx, S->status, 10, out->status, st)) != MC_OK) return rc;
    if (out->status[4] != MC_PARSE_OK) return MC_OK;
    const uint64_t recs = out->status[0], queries = out->status[1];
    HIP_TRY(ctx, hipMemcpyAsync(out->hdr, d.hdr, recs * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->qinfo, d.qinfo, queries * 16, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->max_win, d.max_win, queries * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->name_off, d.name_off, (queries + 1) * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(out->seq, d.seq, out->status[2], hipMemcpyDeviceToHost, st));
    if (out->status[3]) HIP_TRY(ctx, hipMemcpyAsync(out->names, d.names, out->status[3], hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    return MC_OK;
}

int mc_parse_stats(mc_ctx* ctx, uint64_t stats[4])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_parse_stats: no place for the counters");
    stats[0] = stats[1] = stats[2] = stats[3] = 0;
    ParseState* S = nullptr;
    { std::lock_guard<std::mutex> lock(ctx->parseMtx); S = ctx->parse; }
    if (!S) return MC_OK;
    stats[0] = S->calls; stats[1] = S->bytes;
    if (S->dCounters) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        unsigned long long c[2];
        HIP_TRY(ctx, hipMemcpy(c, S->dCounters, 16, hipMemcpyDeviceToHost));
        stats[2] = c[0]; stats[3] = c[1];
    }
    return MC_OK;
}

}  // extern "C"
