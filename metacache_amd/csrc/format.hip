// metacache_amd/csrc/format.hip -- mc_format_set_text / mc_format_mappings / mc_format_stats (+ mc_format_matches*, mc_format_mappings_with): the per-read mapping lines of `metacache query`
// (show_query_mapping, classification.cpp:432-523; show_candidates / show_candidate_ranges, printing.cpp:283-380) rendered on the
// device, behind the query and the vote.  What a line is, piece by piece: include/metacache_amd.h.
//
// THREE LAUNCHES, none of which waits for another block:
//   1. format_lengths_kernel: one lane per read walks the read's pieces and adds up their lengths (exact: digit counts, string lengths
//      from the tables) into line_off[i]; block b owns TILE b, a run of consecutive reads, and leaves the tile's sum in the workspace
//      behind line_off (MC_FORMAT_SCRATCH entries, so at most that many tiles: a tile grows with the batch instead of the grid).
//   2. tile_scan_kernel (block_scan.h): ONE block turns the tile sums into tile offsets and stores the total in line_off[n].
//   3. format_write_kernel: block b scans its tile's lengths into line_off (chunks of 256 reads, a running offset), and -- unless the
//      total exceeds the capacity -- renders the chunk's lines.  Consecutive reads' lines are consecutive in `out`, so a chunk owns one
//      byte range [c0, c1): the block walks it in WINDOWS of kStage bytes that begin at multiples of 16, every lane stores the part of
//      its line that falls into the window into LDS (the same walk as pass 1, clipped), and the block moves the window out in 16-byte
//      lane-consecutive stores; the 16-byte slots at the range's two ends that the chunk owns only partly go out byte by byte.  A line of
//      any length takes this path -- it simply spans more windows, its lane walking it once per window with whole pieces skipped by
//      arithmetic -- so there is no second, direct path to keep equal to the first.
// mc_format_mappings_with is the same three launches with EXTRA = true: one more column, whose bytes somebody else has rendered (piece i
// of `extra`), is given its room by the lanes and copied into the windows by the whole block.  mc_format_mappings launches EXTRA = false.
// mc_format_matches_* (the -allhits column, show_matches, printing.cpp:315-365): a section of its own below, a wave or the block per read.
// Plain HIP C++; no inline assembly.
#include "rows_common.h"
#include "block_scan.h"

#include <algorithm>
#include <atomic>
#include <cstring>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kMaxTiles = MC_FORMAT_SCRATCH, kStage = 32768;
constexpr int kAllFlags = MC_FORMAT_HOST | MC_FORMAT_QUERY_IDS | MC_FORMAT_TRUTH | MC_FORMAT_TOPHITS | MC_FORMAT_LOCATIONS | MC_FORMAT_MAPPED_ONLY;
constexpr uint32_t kCtrLines = 0, kCtrBytes = 1, kCtrOutOfTable = 2, kCtrMatchRuns = 3, kCtrMatchBytes = 4, kCtrMatchBeyond = 5, kCounters = 6;
static_assert(sizeof(mc_candidate) == 16 && sizeof(mc_assignment) == 8, "ABI sizes");
static_assert(kStage % 16 == 0, "windows begin at multiples of 16");
static_assert(kBlock == kScanBlock, "the scans of block_scan.h are for blocks of 256 threads");

struct Text {                            // one table of strings on the device: string k = bytes[off[k] .. off[k + 1])
    const uint8_t* bytes; const uint64_t* off; uint32_t count;
};

struct FmtArgs {
    const mc_candidate* cands;
    const mc_assignment* assigned;
    const uint32_t* truth;
    const uint64_t* ids;                 // may be null: firstId + i
    const uint8_t* names;                // name i = names[nameOff[i] - nameBias .. nameOff[i + 1] - nameBias)
    const uint64_t* nameOff;
    uint8_t* out;
    uint64_t* lineOff;                   // [n + 1], then the tile sums / tile offsets [tiles]
    unsigned long long* counters;        // [kCounters]
    uint64_t firstId, nameBias, cap;
    Text result, targetResult, cand;
    uint32_t n, stride, flags, winStride, winLen, columnLen, tileReads, tiles;
    uint32_t column[4];                  // the column separator's bytes, little-endian in words (a byte of it is picked by shifts: no indexed access to the arguments)
    const uint8_t* extra;                // mc_format_mappings_with: piece i = extra[extraOff[i] - extraBias .. extraOff[i + 1] - extraBias); null: no such column
    const uint64_t* extraOff;
    uint64_t extraBias;
};

__device__ __forceinline__ uint32_t digits_u32(uint32_t v)
{
    return v < 10u ? 1u : v < 100u ? 2u : v < 1000u ? 3u : v < 10000u ? 4u : v < 100000u ? 5u : v < 1000000u ? 6u : v < 10000000u ? 7u : v < 100000000u ? 8u
         : v < 1000000000u ? 9u : 10u;
}
__device__ __forceinline__ uint32_t digits_u64(uint64_t v)
{
    if (v <= 0xFFFFFFFFull) return digits_u32((uint32_t)v);
    uint32_t d = 10; uint64_t p = 10000000000ull;                  // 10^10 <= v?  (2^32 < 10^10: d = 10 at least)
    while (d < 20 && v >= p) { ++d; p *= 10ull; }                  // (p reaches 10^19 at d = 19; 10^20 does not fit and is not formed)
    return d;
}

// where a lane's line goes: pos is the place of the next byte in `out`; only bytes inside the window [w0, w1) are stored, at lds[pos - w0].
// Without WRITE nothing is stored and pos counts the line's length.
template <bool WRITE>
struct Sink {
    uint8_t* lds; uint64_t pos, w0, w1;
    __device__ __forceinline__ bool past() const { return WRITE && pos >= w1; }     // nothing of what follows falls into the window
    __device__ __forceinline__ void ch(uint8_t c)
    {
        if (WRITE && pos >= w0 && pos < w1) lds[pos - w0] = c;
        ++pos;
    }
    __device__ __forceinline__ void bytes(const uint8_t* src, uint64_t len)
    {
        if (WRITE) {
            const uint64_t lo = pos > w0 ? pos : w0, hi = pos + len < w1 ? pos + len : w1;
            for (uint64_t k = lo; k < hi; ++k) lds[k - w0] = src[k - pos];
        }
        pos += len;
    }
    __device__ __forceinline__ void skip(uint64_t len) { pos += len; }             // bytes that somebody else stores
    __device__ __forceinline__ void num(uint64_t v)
    {
        const uint32_t d = digits_u64(v);
        if (WRITE && pos + d > w0 && pos < w1) {
            if (v <= 0xFFFFFFFFull) {
                uint32_t x = (uint32_t)v;
                for (uint32_t k = d; k-- > 0;) { const uint64_t p = pos + k; if (p >= w0 && p < w1) lds[p - w0] = (uint8_t)('0' + x % 10u); x /= 10u; }
            } else {
                for (uint32_t k = d; k-- > 0;) { const uint64_t p = pos + k; if (p >= w0 && p < w1) lds[p - w0] = (uint8_t)('0' + (uint32_t)(v % 10ull)); v /= 10ull; }
            }
        }
        pos += d;
    }
    __device__ __forceinline__ void column(const FmtArgs& a)
    {
        for (uint32_t k = 0; k < a.columnLen; ++k) {
            const uint32_t q = k >> 2, word = q == 0 ? a.column[0] : q == 1 ? a.column[1] : q == 2 ? a.column[2] : a.column[3];
            ch((uint8_t)(word >> ((k & 3u) * 8u)));
        }
    }
    __device__ __forceinline__ void text(const Text& t, uint32_t k)              // k < t.count
    {
        const uint64_t b = t.off[k], e = t.off[k + 1];
        bytes(t.bytes + b, e > b ? e - b : 0);
    }
};

// entry `taxon` of MC_TEXT_RESULT; an index beyond the table takes entry 0 (the table has one: mc_format_set_text) and is counted
template <bool WRITE>
__device__ __forceinline__ void result_text(const FmtArgs& a, Sink<WRITE>& s, uint32_t taxon, uint32_t& beyond)
{
    if (taxon >= a.result.count) { taxon = 0; ++beyond; }
    s.text(a.result, taxon);
}

// the columns in front of the extra one: id, name, truth
template <bool WRITE>
__device__ __forceinline__ void walk_head(const FmtArgs& a, uint64_t i, Sink<WRITE>& s, uint32_t& beyond)
{
    if (a.flags & MC_FORMAT_QUERY_IDS) { s.num(a.ids ? a.ids[i] : a.firstId + i); s.column(a); }
    {
        const uint64_t b = a.nameOff[i], e = a.nameOff[i + 1];
        s.bytes(a.names + (b - a.nameBias), e > b ? e - b : 0);
        s.column(a);
    }
    if (a.flags & MC_FORMAT_TRUTH) { result_text(a, s, a.truth[i], beyond); s.column(a); }
}

// the one walk over a read's pieces that both passes take.  beyond: result indices that lay beyond their table (the caller counts them once per line).
// EXTRA (mc_format_mappings_with): the read's piece of the extra column is given its room and its separator here; its bytes are the block's to copy.
template <bool WRITE, bool EXTRA>
__device__ __forceinline__ void walk_line(const FmtArgs& a, uint64_t i, Sink<WRITE>& s, uint32_t& beyond)
{
    const uint2 as = reinterpret_cast<const uint2*>(a.assigned)[i];              // {taxon, info}
    if ((a.flags & MC_FORMAT_MAPPED_ONLY) && as.x == 0) return;
    const mc_candidate* row = a.cands ? a.cands + i * a.stride : nullptr;
    walk_head<WRITE>(a, i, s, beyond);
    if (EXTRA) {
        const uint64_t b = a.extraOff[i], e = a.extraOff[i + 1];
        s.skip(e > b ? e - b : 0);
        s.column(a);
    }
    if (a.flags & MC_FORMAT_TOPHITS) {                                           // show_candidates, printing.cpp:283-310
        for (uint32_t c = 0; c < a.stride && !s.past(); ++c) {
            const uint4 v = reinterpret_cast<const uint4*>(row)[c];              // {tgt, hits, beg, end}
            if (!v.y) break;
            if (c) s.ch(',');
            if (v.x < a.cand.count) {
                const uint64_t b = a.cand.off[v.x], e = a.cand.off[v.x + 1];
                if (e > b) { s.bytes(a.cand.bytes + b, e - b); s.ch(':'); s.num(v.y); }
            }
        }
        s.column(a);
    }
    if (a.flags & MC_FORMAT_LOCATIONS) {                                         // show_candidate_ranges, printing.cpp:370-380
        for (uint32_t c = 0; c < a.stride && !s.past(); ++c) {
            const uint4 v = reinterpret_cast<const uint4*>(row)[c];
            if (!v.y) break;
            s.ch('['); s.num((uint64_t)a.winStride * v.z); s.ch(','); s.num((uint64_t)a.winStride * v.w + a.winLen); s.ch(']'); s.ch(' ');
        }
        s.column(a);
    }
    if (s.past()) return;
    const bool seqLevel = as.x != 0 && (as.y & 0xFFu) == 0 && a.targetResult.count != 0 && row;
    if (seqLevel) {
        const uint32_t tgt = row[0].tgt;
        if (tgt < a.targetResult.count) s.text(a.targetResult, tgt);
        else result_text(a, s, 0xFFFFFFFFu, beyond);                             // no such target: the unclassified text, counted
    } else result_text(a, s, as.x, beyond);
    s.ch('\n');
}

template <bool EXTRA>
__global__ __launch_bounds__(kBlock) void format_lengths_kernel(FmtArgs a)
{
    __shared__ uint64_t sc[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * a.tileReads, t1 = min(t0 + (uint64_t)a.tileReads, (uint64_t)a.n);
    uint64_t mine = 0;
    for (uint64_t i = t0 + threadIdx.x; i < t1; i += kBlock) {
        Sink<false> s{nullptr, 0, 0, 0};
        uint32_t beyond = 0;
        walk_line<false, EXTRA>(a, i, s, beyond);
        a.lineOff[i] = s.pos;
        mine += s.pos;
    }
    uint64_t total;
    (void)block_excl_scan(mine, sc, total);
    if (threadIdx.x == 0) a.lineOff[(uint64_t)a.n + 1 + blockIdx.x] = total;
}

// EXTRA: the chunk's pieces of the extra column go into the window by the whole block -- a piece of any length costs every lane the same.
// xDst / xSrc / xLen: per read of the chunk where its piece begins in `out`, where in `extra`, and its length; xDst does not decrease
// (lines are consecutive in read order), so a lane finds the piece of an output byte by one binary search and then walks forward.
template <bool EXTRA>
__global__ __launch_bounds__(kBlock) void format_write_kernel(FmtArgs a)
{
    __shared__ uint64_t sc[kBlock];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStage];
    __shared__ uint64_t xDst[EXTRA ? kBlock : 1], xSrc[EXTRA ? kBlock : 1], xLen[EXTRA ? kBlock : 1];
    __shared__ uint32_t beyondAll;
    if (threadIdx.x == 0) beyondAll = 0;
    const uint64_t all = a.lineOff[a.n];
    const bool render = all <= a.cap;                                            // otherwise: offsets only, no byte of out is touched
    const uint64_t t0 = (uint64_t)blockIdx.x * a.tileReads, t1 = min(t0 + (uint64_t)a.tileReads, (uint64_t)a.n);
    uint64_t running = a.lineOff[(uint64_t)a.n + 1 + blockIdx.x];
    uint32_t lines = 0;
    __syncthreads();
    for (uint64_t base = t0; base < t1; base += kBlock) {                        // (the same trips for every lane)
        const uint64_t i = base + threadIdx.x;
        const uint64_t len = i < t1 ? a.lineOff[i] : 0;
        uint64_t chunk;
        const uint64_t off = running + block_excl_scan(len, sc, chunk);
        if (i < t1) a.lineOff[i] = off;
        const uint64_t c0 = running, c1 = running + chunk;                       // the chunk's bytes of out
        running = c1;
        if (!render) continue;
        lines += len ? 1u : 0u;
        if (EXTRA) {
            uint64_t dst = i < t1 ? off : c1, src = 0, xl = 0;                   // (a read without a line has no piece)
            if (len) {
                Sink<false> h{nullptr, 0, 0, 0};
                uint32_t unused = 0;
                walk_head<false>(a, i, h, unused);
                const uint64_t b = a.extraOff[i], e = a.extraOff[i + 1];
                dst = off + h.pos; src = b - a.extraBias; xl = e > b ? e - b : 0;
            }
            xDst[threadIdx.x] = dst; xSrc[threadIdx.x] = src; xLen[threadIdx.x] = xl;
            __syncthreads();
        }
        for (uint64_t w = c0 & ~15ull; w < c1; w += kStage) {
            const uint64_t w1 = min(w + (uint64_t)kStage, c1);
            if (len && off < w1 && off + len > w) {
                Sink<true> s{stage, off, w, w1};
                uint32_t beyond = 0;
                walk_line<true, EXTRA>(a, i, s, beyond);
                if (beyond && off + len <= w1) atomicAdd(&beyondAll, beyond);    // (counted where the line ENDS: the one window whose walk goes through all its pieces)
            }
            if (EXTRA) {
                uint64_t p = max(w, c0) + threadIdx.x;
                if (p < w1) {
                    uint32_t r = 0, hi = kBlock;                                 // r: the reads of the chunk whose pieces begin at or in front of p
                    while (r < hi) { const uint32_t mid = (r + hi) >> 1; if (xDst[mid] <= p) r = mid + 1; else hi = mid; }
                    for (; p < w1; p += kBlock) {
                        while (r < kBlock && xDst[r] <= p) ++r;
                        if (r) { const uint64_t k = p - xDst[r - 1]; if (k < xLen[r - 1]) stage[p - w] = a.extra[xSrc[r - 1] + k]; }
                    }
                }
            }
            __syncthreads();
            const uint64_t lo = max(w, c0);
            for (uint32_t slot = threadIdx.x; (uint64_t)slot * 16u < w1 - w; slot += kBlock) {
                const uint64_t g = w + (uint64_t)slot * 16u;
                if (g >= lo && g + 16u <= w1) *reinterpret_cast<uint4*>(a.out + g) = *reinterpret_cast<const uint4*>(stage + slot * 16u);
                else
                    for (uint32_t k = 0; k < 16u; ++k) { const uint64_t p = g + k; if (p >= lo && p < w1) a.out[p] = stage[slot * 16u + k]; }
            }
            __syncthreads();
        }
    }
    if (!render) return;
    uint64_t blockLines;
    (void)block_excl_scan(lines, sc, blockLines);
    if (threadIdx.x == 0) {
        if (blockLines) atomicAdd(&a.counters[kCtrLines], (unsigned long long)blockLines);
        if (beyondAll) atomicAdd(&a.counters[kCtrOutOfTable], (unsigned long long)beyondAll);
        if (blockIdx.x == 0 && all) atomicAdd(&a.counters[kCtrBytes], (unsigned long long)all);
    }
}

// ---- the all-hits column (mc_format_matches): a read's location list, run-length encoded -------------------------------------------
// show_matches (printing.cpp:315-365): a RUN is a maximal stretch of consecutive equal entries; it prints text '/' window ':' length ','
// (MC_MATCHES_WINDOWS) or text ':' length ','.  The same three launches as the lines -- lengths, the scan of the tile sums
// (tile_scan_kernel itself), write -- but inside a read the work is a wave's, or for a list of more than kMatchBlockList entries the
// block's: the lanes stride over the list in tiles of 64 (the block: of 256); the lane whose entry ENDS a run owns the run; it finds the
// run's first entry from the ballots of the tile's run heads (head k = end k - 1), or, where the tile has none in front of it, from the
// carry: the entries of the open run in front of the tile; a wave scan of the runs' byte lengths (the block: + the waves' sums through LDS)
// gives every run its place, and in the write pass the same walk stores the run there.  A run may span any number of tiles.
constexpr uint32_t kWaves = kBlock / 64, kMatchBlockList = 1024;
constexpr uint64_t kMatchMaxText = 1ull << 24;   // a table entry is shorter than this: 64 runs' bytes fit the 32-bit wave scan

struct MatchArgs {
    const unsigned long long* hits;      // mc_location as a 64-bit number: (tgt << 32) | win; list i = hits[hitOff[i] - hitBias .. hitOff[i + 1] - hitBias)
    const uint64_t* hitOff;
    uint8_t* out;
    uint64_t* pieceOff;                  // [n + 1], then the tile sums / tile offsets [tiles]
    unsigned long long* counters;
    uint64_t hitBias, cap;
    Text text;
    uint32_t n, windows, tileReads, tiles;
};
struct MatchShared { unsigned long long ends[kWaves]; uint32_t sums[kWaves]; };   // a tile's end ballots and byte sums, wave by wave (each is read between the two barriers that follow its store)

__device__ __forceinline__ void put_byte(uint8_t* out, uint64_t cap, uint64_t p, uint8_t c) { if (p < cap) out[p] = c; }
__device__ __forceinline__ void put_number(uint8_t* out, uint64_t cap, uint64_t p, uint64_t v, uint32_t d)
{
    for (uint32_t k = d; k-- > 0;) { put_byte(out, cap, p + k, (uint8_t)('0' + (uint32_t)(v % 10ull))); v /= 10ull; }
}

// one list, by a wave (W == 1: all its 64 lanes, none of the block's barriers) or by the block (W == kWaves: all its threads) -> the
// piece's bytes.  WRITE: the runs are stored from out[outAt] on.  runs / beyond: this WAVE's tallies (the same in all its lanes).
template <uint32_t W, bool WRITE>
__device__ __forceinline__ uint64_t walk_list(const MatchArgs& a, uint64_t b, uint64_t len, uint64_t outAt, MatchShared& sh, uint32_t& runs, uint32_t& beyond)
{
    constexpr uint32_t G = 64u * W;
    const uint32_t lane = threadIdx.x & 63u, wv = W == 1 ? 0u : threadIdx.x >> 6, t = wv * 64u + lane;
    uint64_t running = 0, carry = 0;                 // carry: the entries of the open run in front of this tile
    unsigned long long prevEnded = 1;                // the entry in front of this tile ended a run (or there is none)
    for (uint64_t base = 0; base < len; base += G) {
        const uint64_t j = base + t;
        const bool valid = j < len, last = j + 1 >= len;
        unsigned long long cur = 0, nxt = 0;
        if (valid) cur = a.hits[b + j];
        if (valid && !last) nxt = a.hits[b + j + 1];
        const bool isEnd = valid && (last || nxt != cur);
        const unsigned long long ends = __ballot(isEnd);
        unsigned long long mk[W];
        if (W == 1) mk[0] = ends;
        else {
            if (lane == 0) sh.ends[wv] = ends;
            __syncthreads();
#pragma unroll
            for (uint32_t w = 0; w < W; ++w) mk[w] = sh.ends[w];
        }
        // heads of wave w's 64 entries: entry k begins a run where entry k - 1 ended one
        uint64_t count = 0;
        bool found = false;
        uint32_t lastHead = 0;
        bool anyHead = false;
#pragma unroll
        for (int w = (int)W - 1; w >= 0; --w) {
            const unsigned long long heads = (mk[w] << 1) | (w == 0 ? prevEnded : (mk[w > 0 ? w - 1 : 0] >> 63));
            if (!anyHead && heads) { anyHead = true; lastHead = (uint32_t)w * 64u + 63u - (uint32_t)__clzll((long long)heads); }
            if (isEnd && !found && (uint32_t)w <= wv) {
                const unsigned long long mine = (uint32_t)w == wv ? heads & ((2ull << lane) - 1ull) : heads;   // (lane 63: 2 << 63 == 0, the mask is all ones)
                if (mine) { found = true; count = (uint64_t)(t - ((uint32_t)w * 64u + 63u - (uint32_t)__clzll((long long)mine))) + 1; }
            }
        }
        if (isEnd && !found) count = carry + t + 1;
        carry = anyHead ? (uint64_t)(G - lastHead) : carry + G;
        prevEnded = mk[W - 1] >> 63;
        // the run's bytes
        const uint32_t tgt = (uint32_t)(cur >> 32), win = (uint32_t)cur;
        const bool neg = (int32_t)win < 0;
        const uint32_t mag = neg ? 0u - win : win;
        uint32_t v = 0, tl = 0;
        uint64_t tb = 0;
        bool over = false;
        if (isEnd) {
            if (tgt < a.text.count) {
                tb = a.text.off[tgt];
                const uint64_t te = a.text.off[tgt + 1];
                tl = te > tb ? (uint32_t)(te - tb) : 0u;
                if (a.windows) { if (tl) v = tl + 1u + (neg ? 1u : 0u) + digits_u32(mag) + 1u + digits_u64(count) + 1u; }
                else v = tl + 1u + digits_u64(count) + 1u;
            } else over = true;
        }
        const uint32_t incl = wave_incl_scan_u32(v, lane);
        uint64_t at = running + (incl - v), tileBytes = rdlane(incl, 63);
        if (W > 1) {
            if (lane == 63) sh.sums[wv] = incl;
            __syncthreads();
            tileBytes = 0;
#pragma unroll
            for (uint32_t w = 0; w < W; ++w) { const uint32_t x = sh.sums[w]; if (w < wv) at += x; tileBytes += x; }
        }
        running += tileBytes;
        runs += (uint32_t)__popcll(__ballot(v != 0));
        beyond += (uint32_t)__popcll(__ballot(over));
        if (WRITE && v) {
            uint64_t p = outAt + at;
            for (uint32_t k = 0; k < tl; ++k) put_byte(a.out, a.cap, p + k, a.text.bytes[tb + k]);
            p += tl;
            if (a.windows) {
                put_byte(a.out, a.cap, p++, '/');
                if (neg) put_byte(a.out, a.cap, p++, '-');
                const uint32_t d = digits_u32(mag);
                put_number(a.out, a.cap, p, mag, d);
                p += d;
            }
            put_byte(a.out, a.cap, p++, ':');
            const uint32_t d = digits_u64(count);
            put_number(a.out, a.cap, p, count, d);
            put_byte(a.out, a.cap, p + d, ',');
        }
    }
    return running;
}

// block b owns tile b (tileReads consecutive reads).  Lengths pass: pieceOff[i] = the bytes of piece i, the tile's sum behind pieceOff[n].
// Write pass: the tile's lengths become offsets, and -- unless the total exceeds the capacity -- the same walk stores the runs.
template <bool WRITE>
__global__ __launch_bounds__(kBlock) void matches_kernel(MatchArgs a)
{
    __shared__ uint64_t sc[kBlock];
    __shared__ MatchShared sh;
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint64_t t0 = (uint64_t)blockIdx.x * a.tileReads, t1 = min(t0 + (uint64_t)a.tileReads, (uint64_t)a.n);
    const uint64_t all = WRITE ? a.pieceOff[a.n] : 0;
    if (WRITE) {
        uint64_t running = a.pieceOff[(uint64_t)a.n + 1 + blockIdx.x];
        for (uint64_t base = t0; base < t1; base += kBlock) {                    // (the same trips for every lane)
            const uint64_t i = base + threadIdx.x;
            const uint64_t len = i < t1 ? a.pieceOff[i] : 0;
            uint64_t chunk;
            const uint64_t off = running + block_excl_scan(len, sc, chunk);
            if (i < t1) a.pieceOff[i] = off;
            running += chunk;
        }
        if (all > a.cap) return;                                                 // offsets only: no byte of out is touched
        __syncthreads();                                                         // (the offsets are read by other waves below)
    }
    uint32_t runs = 0, beyond = 0;
    uint64_t mine = 0;
    for (uint64_t i = t0 + wave; i < t1; i += kWaves) {                          // lists up to kMatchBlockList entries: a wave each
        const uint64_t b = a.hitOff[i], e = a.hitOff[i + 1], len = e > b ? e - b : 0;
        if (len > kMatchBlockList) continue;
        const uint64_t bytes = walk_list<1, WRITE>(a, b - a.hitBias, len, WRITE ? a.pieceOff[i] : 0, sh, runs, beyond);
        if (!WRITE && lane == 0) { a.pieceOff[i] = bytes; mine += bytes; }
    }
    __syncthreads();
    for (uint64_t i = t0; i < t1; ++i) {                                         // longer ones: the block, one after the other
        const uint64_t b = a.hitOff[i], e = a.hitOff[i + 1], len = e > b ? e - b : 0;
        if (len <= kMatchBlockList) continue;
        const uint64_t bytes = walk_list<kWaves, WRITE>(a, b - a.hitBias, len, WRITE ? a.pieceOff[i] : 0, sh, runs, beyond);
        if (!WRITE && threadIdx.x == 0) { a.pieceOff[i] = bytes; mine += bytes; }
        __syncthreads();
    }
    if (!WRITE) {
        uint64_t total;
        (void)block_excl_scan(mine, sc, total);
        if (threadIdx.x == 0) a.pieceOff[(uint64_t)a.n + 1 + blockIdx.x] = total;
        return;
    }
    if (lane == 0) {
        if (runs) atomicAdd(&a.counters[kCtrMatchRuns], (unsigned long long)runs);
        if (beyond) atomicAdd(&a.counters[kCtrMatchBeyond], (unsigned long long)beyond);
        if (threadIdx.x == 0 && blockIdx.x == 0 && all) atomicAdd(&a.counters[kCtrMatchBytes], (unsigned long long)all);
    }
}

struct HostText { std::vector<uint8_t> bytes; std::vector<uint64_t> off; bool set = false; uint64_t version = 0; };
struct DevText { uint8_t* bytes = nullptr; uint64_t* off = nullptr; uint32_t count = 0; uint64_t version = 0; bool made = false; };

}  // namespace

namespace mcamd {

struct FormatState {                     // what the context keeps for mc_format_*
    HostText host[3];                    // the tables as mc_format_set_text left them
    DevText dev[3];                      // their device copies (made on first use, made again after a later set)
    unsigned long long* dCounters = nullptr;   // [kCounters]
    std::atomic<uint64_t> calls{0}, reads{0};
    std::mutex stageMtx;                 // MC_FORMAT_HOST callers take turns at the staging buffers
    DevBuf stageCands, stageAssigned, stageTruth, stageIds, stageNames, stageNameOff, stageLineOff, stageOut, stageExtra, stageExtraOff;
    HostText matchHost; DevText matchDev;      // mc_format_matches_set_text's table and its device copy
    std::atomic<uint64_t> matchCalls{0}, matchReads{0};
    DevBuf stageHits, stageHitOff, stagePieceOff;   // mc_format_matches(MC_FORMAT_HOST), under stageMtx (stageOut and hTotal are shared with the lines)
    uint64_t* hTotal = nullptr;          // pinned: a piece's total
};

void free_format_state(mc_ctx* ctx)
{
    if (!ctx->format) return;
    FormatState& S = *ctx->format;
    for (DevText* d : {&S.dev[0], &S.dev[1], &S.dev[2], &S.matchDev}) { if (d->bytes) (void)hipFree(d->bytes); if (d->off) (void)hipFree(d->off); }
    if (S.dCounters) (void)hipFree(S.dCounters);
    if (S.hTotal) (void)hipHostFree(S.hTotal);
    for (DevBuf* b : {&S.stageCands, &S.stageAssigned, &S.stageTruth, &S.stageIds, &S.stageNames, &S.stageNameOff, &S.stageLineOff, &S.stageOut, &S.stageExtra, &S.stageExtraOff, &S.stageHits, &S.stageHitOff, &S.stagePieceOff})
        if (b->p) (void)hipFree(b->p);
    delete ctx->format;
    ctx->format = nullptr;
}

}  // namespace mcamd

namespace {

FormatState& state_of(mc_ctx* ctx)       // under ctx->formatMtx
{
    if (!ctx->format) ctx->format = new FormatState;
    return *ctx->format;
}

// the device copies of the tables that have changed since they were made, and the counters
int ensure_format_state(mc_ctx* ctx, FormatState** out)
{
    std::lock_guard<std::mutex> lock(ctx->formatMtx);
    FormatState& S = state_of(ctx);
    *out = &S;
    for (int w = 0; w < 4; ++w) {
        const HostText& h = w < 3 ? S.host[w] : S.matchHost;
        DevText& d = w < 3 ? S.dev[w] : S.matchDev;
        if (!h.set || (d.made && d.version == h.version)) continue;
        if (d.made) {                                                  // (a new table: no format call may be in flight)
            HIP_TRY(ctx, hipDeviceSynchronize());
            (void)hipFree(d.bytes); (void)hipFree(d.off); d.bytes = nullptr; d.off = nullptr; d.made = false;
        }
        HIP_TRY(ctx, hipMalloc((void**)&d.bytes, std::max<size_t>(h.bytes.size(), 16)));
        HIP_TRY(ctx, hipMalloc((void**)&d.off, h.off.size() * 8));
        if (!h.bytes.empty()) HIP_TRY(ctx, hipMemcpy(d.bytes, h.bytes.data(), h.bytes.size(), hipMemcpyHostToDevice));
        HIP_TRY(ctx, hipMemcpy(d.off, h.off.data(), h.off.size() * 8, hipMemcpyHostToDevice));
        d.count = (uint32_t)(h.off.size() - 1);
        d.version = h.version;
        d.made = true;
    }
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, kCounters * 8));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, kCounters * 8));
    }
    if (!S.hTotal) HIP_TRY(ctx, hipHostMalloc((void**)&S.hTotal, 8));
    return MC_OK;
}

void tiles_of(uint32_t n, uint32_t& tileReads, uint32_t& tiles)
{
    const uint64_t per = ((uint64_t)n + kMaxTiles - 1) / kMaxTiles;
    tileReads = (uint32_t)std::max<uint64_t>(kBlock, (per + kBlock - 1) / kBlock * kBlock);
    tiles = (uint32_t)(((uint64_t)n + tileReads - 1) / tileReads);
}

// with the extra column a line is as long as its piece -- kilobytes -- and the pieces are the block's to copy, not a lane's: the tiles are
// as small as the workspace allows (down to kExtraTileReads reads), so that a batch of a few thousand reads still fills the device
constexpr uint32_t kExtraTileReads = 16;
void extra_tiles_of(uint32_t n, uint32_t& tileReads, uint32_t& tiles)
{
    const uint64_t per = ((uint64_t)n + kMaxTiles - 1) / kMaxTiles;
    tileReads = (uint32_t)std::max<uint64_t>(kExtraTileReads, (per + kExtraTileReads - 1) / kExtraTileReads * kExtraTileReads);
    tiles = (uint32_t)(((uint64_t)n + tileReads - 1) / tileReads);
}

FmtArgs make_args(const FormatState& S, const mc_format_options* opt, int flags, uint32_t n, uint32_t stride)
{
    FmtArgs a{};
    auto text = [&](int w) { const DevText& d = S.dev[w]; return d.made ? Text{d.bytes, d.off, d.count} : Text{nullptr, nullptr, 0}; };
    a.result = text(MC_TEXT_RESULT); a.targetResult = text(MC_TEXT_TARGET_RESULT); a.cand = text(MC_TEXT_CANDIDATE);
    a.counters = S.dCounters;
    a.n = n; a.stride = stride; a.flags = (uint32_t)(flags & ~MC_FORMAT_HOST);
    a.winStride = opt->win_stride; a.winLen = opt->win_len; a.columnLen = opt->column_len;
    std::memcpy(a.column, opt->column, 16);
    tiles_of(n, a.tileReads, a.tiles);
    return a;
}

void launch_lengths(mc_ctx* ctx, const FmtArgs& a, hipStream_t st)
{
    ScopedTimer timer(ctx, "format_lengths", st);
    if (a.extra) hipLaunchKernelGGL(format_lengths_kernel<true>, dim3(a.tiles), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(format_lengths_kernel<false>, dim3(a.tiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(tile_scan_kernel<uint64_t>, dim3(1), dim3(kBlock), 0, st, a.lineOff + (uint64_t)a.n + 1, a.tiles, a.lineOff + a.n);
}
void launch_write(mc_ctx* ctx, const FmtArgs& a, hipStream_t st)
{
    ScopedTimer timer(ctx, "format_write", st);
    if (a.extra) hipLaunchKernelGGL(format_write_kernel<true>, dim3(a.tiles), dim3(kBlock), 0, st, a);
    else hipLaunchKernelGGL(format_write_kernel<false>, dim3(a.tiles), dim3(kBlock), 0, st, a);
}

MatchArgs make_match_args(const FormatState& S, int flags, uint32_t n)
{
    MatchArgs a{};
    a.text = Text{S.matchDev.bytes, S.matchDev.off, S.matchDev.count};
    a.counters = S.dCounters;
    a.n = n; a.windows = (flags & MC_MATCHES_WINDOWS) ? 1u : 0u;
    const uint64_t per = ((uint64_t)n + kMaxTiles - 1) / kMaxTiles;            // (a tile is a whole number of waves' reads and grows with the batch instead of the grid)
    a.tileReads = (uint32_t)std::max<uint64_t>(kWaves, (per + kWaves - 1) / kWaves * kWaves);
    a.tiles = (uint32_t)(((uint64_t)n + a.tileReads - 1) / a.tileReads);
    return a;
}
void launch_match_lengths(mc_ctx* ctx, const MatchArgs& a, hipStream_t st)
{
    ScopedTimer timer(ctx, "matches_lengths", st);
    hipLaunchKernelGGL(matches_kernel<false>, dim3(a.tiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(tile_scan_kernel<uint64_t>, dim3(1), dim3(kBlock), 0, st, a.pieceOff + (uint64_t)a.n + 1, a.tiles, a.pieceOff + a.n);
}
void launch_match_write(mc_ctx* ctx, const MatchArgs& a, hipStream_t st)
{
    ScopedTimer timer(ctx, "matches_write", st);
    hipLaunchKernelGGL(matches_kernel<true>, dim3(a.tiles), dim3(kBlock), 0, st, a);
}

// mc_format_mappings (extra == nullptr) and mc_format_mappings_with: `fnName` is the name the error texts carry
int format_lines(const char* fnName, mc_ctx* ctx, const mc_format_options* opt, const mc_candidate* cands, uint32_t stride, const mc_assignment* assigned,
                 const uint32_t* truth, const uint64_t* query_ids, uint64_t first_query_id, const char* names, const uint64_t* name_off,
                 uint32_t n, int flags, char* out, uint64_t out_capacity, uint64_t* line_off, void* streamv, const char* extra, const uint64_t* extra_off)
{
    const std::string fn(fnName);
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!opt) return fail(ctx, MC_ERR_INVALID, fn + ": no options");
    if (flags & ~kAllFlags) return fail(ctx, MC_ERR_INVALID, fn + ": unknown flag");
    if (stride == 0) return fail(ctx, MC_ERR_INVALID, fn + ": stride == 0");
    if (opt->column_len > 16) return fail(ctx, MC_ERR_INVALID, fn + ": a column separator has at most 16 bytes");
    if (!line_off) return fail(ctx, MC_ERR_INVALID, fn + ": no line_off");
    if ((flags & MC_FORMAT_TRUTH) && n > 0 && !truth) return fail(ctx, MC_ERR_INVALID, fn + ": MC_FORMAT_TRUTH without truth");
    if (n > 0 && (!cands || !assigned || !name_off)) return fail(ctx, MC_ERR_INVALID, fn + ": null array");
    if (out_capacity > 0 && !out) return fail(ctx, MC_ERR_INVALID, fn + ": no out");
    if (extra && n > 0 && !extra_off) return fail(ctx, MC_ERR_INVALID, fn + ": extra without extra_off");
    const bool host = (flags & MC_FORMAT_HOST) != 0;
    if (host && n > 0 && name_off[n] > name_off[0] && !names) return fail(ctx, MC_ERR_INVALID, fn + ": no names");
    if (!host) {
        if (((uintptr_t)out | (uintptr_t)cands) & 15u) return fail(ctx, MC_ERR_INVALID, fn + ": device arrays must be aligned (out and cands: 16 bytes)");
        if (((uintptr_t)assigned | (uintptr_t)query_ids | (uintptr_t)name_off | (uintptr_t)line_off) & 7u) return fail(ctx, MC_ERR_INVALID, fn + ": device arrays must be aligned (assigned, query_ids, name_off, line_off: 8 bytes)");
        if (extra && ((uintptr_t)extra_off & 7u)) return fail(ctx, MC_ERR_INVALID, fn + ": device arrays must be aligned (extra_off: 8 bytes)");
        if ((uintptr_t)truth & 3u) return fail(ctx, MC_ERR_INVALID, fn + ": device arrays must be aligned (truth: 4 bytes)");
    }
    if (n > 0 && out_capacity > 0) {
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + out_capacity;
        auto hits = [&](const void* p, uint64_t bytes) { return p && ranges_overlap((uintptr_t)p, (uintptr_t)p + std::max<uint64_t>(bytes, 1), o0, o1); };
        const uint64_t nameBytes = host ? name_off[n] - name_off[0] : 1;           // (device form: the names' extent lies on the device; their first byte is looked at)
        if (hits(cands, (uint64_t)n * stride * sizeof(mc_candidate)) || hits(assigned, (uint64_t)n * sizeof(mc_assignment)) || hits(truth, (uint64_t)n * 4) ||
            hits(query_ids, (uint64_t)n * 8) || hits(names, nameBytes) || hits(name_off, ((uint64_t)n + 1) * 8) ||
            hits(line_off, ((uint64_t)n + 1 + (host ? 0 : MC_FORMAT_SCRATCH)) * 8) ||
            (extra && (hits(extra, host ? extra_off[n] - extra_off[0] : 1) || hits(extra_off, ((uint64_t)n + 1) * 8))))
            return fail(ctx, MC_ERR_INVALID, fn + ": out overlaps an input or line_off");
    }
    if (n == 0 && host) { line_off[0] = 0; return MC_OK; }
    // ... then state
    {
        std::lock_guard<std::mutex> lock(ctx->formatMtx);
        const FormatState* S = ctx->format;
        if (!S || !S->host[MC_TEXT_RESULT].set) return fail(ctx, MC_ERR_STATE, fn + ": the context has no MC_TEXT_RESULT table (mc_format_set_text)");
        if ((flags & MC_FORMAT_TOPHITS) && !S->host[MC_TEXT_CANDIDATE].set) return fail(ctx, MC_ERR_STATE, fn + ": MC_FORMAT_TOPHITS needs the MC_TEXT_CANDIDATE table (mc_format_set_text)");
    }
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, fn + ": the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(line_off, 0, 8, st));
        return MC_OK;
    }
    FormatState* S = nullptr;
    int rc = ensure_format_state(ctx, &S);
    if (rc) return rc;
    FmtArgs a = make_args(*S, opt, flags, n, stride);
    if (!host) {
        a.extra = (const uint8_t*)extra; a.extraOff = extra_off; a.extraBias = 0;
        if (extra) extra_tiles_of(n, a.tileReads, a.tiles);
        a.cands = cands; a.assigned = assigned; a.truth = truth; a.ids = query_ids; a.firstId = first_query_id;
        a.names = (const uint8_t*)names; a.nameOff = name_off; a.nameBias = 0; a.out = (uint8_t*)out; a.cap = out_capacity; a.lineOff = line_off;
        launch_lengths(ctx, a, st);
        launch_write(ctx, a, st);
        HIP_TRY(ctx, hipGetLastError());
        ++S->calls; S->reads += n;
        return MC_OK;
    }
    // host arrays: in pieces through the staging buffers, one caller at a time.  No byte of `out` may be written unless ALL lines fit, so
    // the pieces' totals come first (lengths + scan per piece); a batch of one piece -- the common case -- keeps its staged inputs on
    // the device for the write pass, more pieces are staged a second time.
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint32_t byBytes = staged_piece_rows(n, stride);
    const uint32_t piece = ctx->formatStageRows ? std::min<uint32_t>(byBytes, ctx->formatStageRows) : byBytes;
    const bool single = piece >= n;
    uint64_t maxNames = 0, maxExtra = 0;
    for (uint64_t done = 0; done < n; done += piece) {
        const uint64_t m = std::min<uint64_t>(piece, n - done);
        if (name_off[done + m] < name_off[done]) return fail(ctx, MC_ERR_INVALID, fn + ": name_off must not decrease");
        maxNames = std::max(maxNames, name_off[done + m] - name_off[done]);
        if (extra && extra_off[done + m] < extra_off[done]) return fail(ctx, MC_ERR_INVALID, fn + ": extra_off must not decrease");
        if (extra) maxExtra = std::max(maxExtra, extra_off[done + m] - extra_off[done]);
    }
    if (extra && ((rc = grow(ctx, S->stageExtra, std::max<uint64_t>(maxExtra, 16))) != MC_OK || (rc = grow(ctx, S->stageExtraOff, ((uint64_t)piece + 1) * 8)) != MC_OK)) return rc;
    if ((rc = grow(ctx, S->stageCands, (uint64_t)piece * stride * sizeof(mc_candidate))) != MC_OK || (rc = grow(ctx, S->stageAssigned, (uint64_t)piece * sizeof(mc_assignment))) != MC_OK ||
        (truth && (rc = grow(ctx, S->stageTruth, (uint64_t)piece * 4)) != MC_OK) || (query_ids && (rc = grow(ctx, S->stageIds, (uint64_t)piece * 8)) != MC_OK) ||
        (rc = grow(ctx, S->stageNames, std::max<uint64_t>(maxNames, 16))) != MC_OK || (rc = grow(ctx, S->stageNameOff, ((uint64_t)piece + 1) * 8)) != MC_OK ||
        (rc = grow(ctx, S->stageLineOff, ((uint64_t)piece + 1 + MC_FORMAT_SCRATCH) * 8)) != MC_OK) return rc;
    auto stage = [&](uint64_t done, uint32_t m, FmtArgs& p) -> int {
        HIP_TRY(ctx, hipMemcpyAsync(S->stageCands.p, cands + done * stride, (uint64_t)m * stride * sizeof(mc_candidate), hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(S->stageAssigned.p, assigned + done, (uint64_t)m * sizeof(mc_assignment), hipMemcpyHostToDevice, st));
        if (truth) HIP_TRY(ctx, hipMemcpyAsync(S->stageTruth.p, truth + done, (uint64_t)m * 4, hipMemcpyHostToDevice, st));
        if (query_ids) HIP_TRY(ctx, hipMemcpyAsync(S->stageIds.p, query_ids + done, (uint64_t)m * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(S->stageNameOff.p, name_off + done, ((uint64_t)m + 1) * 8, hipMemcpyHostToDevice, st));
        const uint64_t nb = name_off[done + m] - name_off[done];
        if (nb) HIP_TRY(ctx, hipMemcpyAsync(S->stageNames.p, names + name_off[done], nb, hipMemcpyHostToDevice, st));
        if (extra) {
            HIP_TRY(ctx, hipMemcpyAsync(S->stageExtraOff.p, extra_off + done, ((uint64_t)m + 1) * 8, hipMemcpyHostToDevice, st));
            const uint64_t xb = extra_off[done + m] - extra_off[done];
            if (xb) HIP_TRY(ctx, hipMemcpyAsync(S->stageExtra.p, extra + extra_off[done], xb, hipMemcpyHostToDevice, st));
        }
        p = a;
        if (extra) { p.extra = (const uint8_t*)S->stageExtra.p; p.extraOff = (const uint64_t*)S->stageExtraOff.p; p.extraBias = extra_off[done]; }
        p.n = m;
        if (extra) extra_tiles_of(m, p.tileReads, p.tiles); else tiles_of(m, p.tileReads, p.tiles);
        p.cands = (const mc_candidate*)S->stageCands.p; p.assigned = (const mc_assignment*)S->stageAssigned.p;
        p.truth = truth ? (const uint32_t*)S->stageTruth.p : nullptr; p.ids = query_ids ? (const uint64_t*)S->stageIds.p : nullptr;
        p.firstId = first_query_id + done;
        p.names = (const uint8_t*)S->stageNames.p; p.nameOff = (const uint64_t*)S->stageNameOff.p; p.nameBias = name_off[done];
        p.lineOff = (uint64_t*)S->stageLineOff.p;
        launch_lengths(ctx, p, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(S->hTotal, p.lineOff + m, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return MC_OK;
    };
    FmtArgs p{};
    uint64_t all = 0;
    for (uint64_t done = 0; done < n; done += piece) {
        if ((rc = stage(done, (uint32_t)std::min<uint64_t>(piece, n - done), p)) != MC_OK) return rc;
        all += *S->hTotal;
    }
    const bool fits = all <= out_capacity;
    uint64_t at = 0;
    for (uint64_t done = 0; done < n; done += piece) {
        const uint32_t m = (uint32_t)std::min<uint64_t>(piece, n - done);
        if (!single && (rc = stage(done, m, p)) != MC_OK) return rc;
        const uint64_t total = *S->hTotal;
        if (fits && (rc = grow(ctx, S->stageOut, std::max<uint64_t>(total, 16))) != MC_OK) return rc;
        p.out = (uint8_t*)S->stageOut.p;
        p.cap = fits ? total : 0;
        if (!fits && total == 0) p.cap = 0;
        launch_write(ctx, p, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(line_off + done, p.lineOff, (uint64_t)m * 8, hipMemcpyDeviceToHost, st));
        if (fits && total) HIP_TRY(ctx, hipMemcpyAsync(out + at, S->stageOut.p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (uint64_t k = done; k < done + m; ++k) line_off[k] += at;
        at += total;
    }
    line_off[n] = all;
    ++S->calls; S->reads += n;
    if (!fits) return fail(ctx, MC_ERR_NOMEM, fn + ": the lines need " + std::to_string(all) + " bytes, out has " + std::to_string(out_capacity) + " (line_off is complete)");
    return MC_OK;
}

}  // namespace

extern "C" {

int mc_format_set_text(mc_ctx* ctx, int which, const char* bytes, const uint64_t* offsets, uint64_t count)
{
    if (!ctx) return MC_ERR_INVALID;
    if (which != MC_TEXT_RESULT && which != MC_TEXT_TARGET_RESULT && which != MC_TEXT_CANDIDATE) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: unknown table");
    if (!offsets) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: no offsets");
    if (count >= 0xFFFFFFFFull) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: more strings than a 32-bit index reaches");
    if (which == MC_TEXT_RESULT && count == 0) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: MC_TEXT_RESULT needs entry 0, the unclassified text");
    if (offsets[0] != 0) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: offsets[0] must be 0");
    for (uint64_t k = 0; k < count; ++k)
        if (offsets[k + 1] < offsets[k]) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: offsets must not decrease");
    if (offsets[count] > 0 && !bytes) return fail(ctx, MC_ERR_INVALID, "mc_format_set_text: no bytes");
    std::lock_guard<std::mutex> lock(ctx->formatMtx);
    HostText& h = state_of(ctx).host[which];
    h.bytes.assign((const uint8_t*)bytes, (const uint8_t*)bytes + offsets[count]);
    h.off.assign(offsets, offsets + count + 1);
    h.set = true;
    ++h.version;
    return MC_OK;
}

int mc_format_mappings(mc_ctx* ctx, const mc_format_options* opt, const mc_candidate* cands, uint32_t stride, const mc_assignment* assigned,
                       const uint32_t* truth, const uint64_t* query_ids, uint64_t first_query_id, const char* names, const uint64_t* name_off,
                       uint32_t n, int flags, char* out, uint64_t out_capacity, uint64_t* line_off, void* stream)
{
    return format_lines("mc_format_mappings", ctx, opt, cands, stride, assigned, truth, query_ids, first_query_id, names, name_off, n, flags, out, out_capacity, line_off, stream, nullptr, nullptr);
}

int mc_format_mappings_with(mc_ctx* ctx, const mc_format_options* opt, const mc_candidate* cands, uint32_t stride, const mc_assignment* assigned,
                            const uint32_t* truth, const uint64_t* query_ids, uint64_t first_query_id, const char* names, const uint64_t* name_off,
                            uint32_t n, int flags, char* out, uint64_t out_capacity, uint64_t* line_off, void* stream, const char* extra, const uint64_t* extra_off)
{
    return format_lines("mc_format_mappings_with", ctx, opt, cands, stride, assigned, truth, query_ids, first_query_id, names, name_off, n, flags, out, out_capacity, line_off, stream, extra, extra_off);
}

int mc_format_matches_set_text(mc_ctx* ctx, const char* bytes, const uint64_t* offsets, uint64_t count)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!offsets) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_set_text: no offsets");
    if (count >= 0xFFFFFFFFull) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_set_text: more strings than a 32-bit index reaches");
    if (offsets[0] != 0) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_set_text: offsets[0] must be 0");
    for (uint64_t k = 0; k < count; ++k) {
        if (offsets[k + 1] < offsets[k]) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_set_text: offsets must not decrease");
        if (offsets[k + 1] - offsets[k] >= kMatchMaxText) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_set_text: a string of 16 MiB or more");
    }
    if (offsets[count] > 0 && !bytes) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_set_text: no bytes");
    std::lock_guard<std::mutex> lock(ctx->formatMtx);
    HostText& h = state_of(ctx).matchHost;
    h.bytes.assign((const uint8_t*)bytes, (const uint8_t*)bytes + offsets[count]);
    h.off.assign(offsets, offsets + count + 1);
    h.set = true;
    ++h.version;
    return MC_OK;
}

int mc_format_matches(mc_ctx* ctx, const mc_location* hits, const uint64_t* hit_off, uint32_t n, int flags, char* out, uint64_t out_capacity,
                      uint64_t* piece_off, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~(MC_FORMAT_HOST | MC_MATCHES_WINDOWS)) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: unknown flag");
    if (!piece_off) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: no piece_off");
    if (n > 0 && !hit_off) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: no hit_off");
    if (out_capacity > 0 && !out) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: no out");
    const bool host = (flags & MC_FORMAT_HOST) != 0;
    if (host) {
        for (uint32_t i = 0; i < n; ++i) if (hit_off[i + 1] < hit_off[i]) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: hit_off must not decrease");
        if (n > 0 && hit_off[n] > hit_off[0] && !hits) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: no hits");
    } else {
        if ((uintptr_t)out & 15u) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: device arrays must be aligned (out: 16 bytes)");
        if (((uintptr_t)hits | (uintptr_t)hit_off | (uintptr_t)piece_off) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_format_matches: device arrays must be aligned (hits, hit_off, piece_off: 8 bytes)");
    }
    if (n > 0 && out_capacity > 0) {
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + out_capacity;
        auto overlaps = [&](const void* p, uint64_t bytes) { return p && ranges_overlap((uintptr_t)p, (uintptr_t)p + std::max<uint64_t>(bytes, 1), o0, o1); };
        const uint64_t hitBytes = host ? (hit_off[n] - hit_off[0]) * sizeof(mc_location) : 1;   // (device form: the lists' extent lies on the device; their first byte is looked at)
        if (overlaps(host && hits ? hits + hit_off[0] : hits, hitBytes) || overlaps(hit_off, ((uint64_t)n + 1) * 8) || overlaps(piece_off, ((uint64_t)n + 1 + (host ? 0 : MC_FORMAT_SCRATCH)) * 8))
            return fail(ctx, MC_ERR_INVALID, "mc_format_matches: out overlaps an input or piece_off");
    }
    if (n == 0 && host) { piece_off[0] = 0; return MC_OK; }
    // ... then state
    {
        std::lock_guard<std::mutex> lock(ctx->formatMtx);
        if (!ctx->format || !ctx->format->matchHost.set) return fail(ctx, MC_ERR_STATE, "mc_format_matches: the context has no table of texts (mc_format_matches_set_text)");
    }
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_format_matches: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (n == 0) {
        HIP_TRY(ctx, hipMemsetAsync(piece_off, 0, 8, st));
        return MC_OK;
    }
    FormatState* S = nullptr;
    int rc = ensure_format_state(ctx, &S);
    if (rc) return rc;
    MatchArgs a = make_match_args(*S, flags, n);
    if (!host) {
        a.hits = (const unsigned long long*)hits; a.hitOff = hit_off; a.hitBias = 0; a.out = (uint8_t*)out; a.cap = out_capacity; a.pieceOff = piece_off;
        launch_match_lengths(ctx, a, st);
        launch_match_write(ctx, a, st);
        HIP_TRY(ctx, hipGetLastError());
        ++S->matchCalls; S->matchReads += n;
        return MC_OK;
    }
    // host arrays: in pieces of whole reads through the staging buffers, one caller at a time; a piece holds at most `room` locations, a
    // read whose list alone is longer goes alone.  As for the lines, the totals come first: no byte of `out` unless everything fits.
    std::lock_guard<std::mutex> lock(S->stageMtx);
    const uint64_t room = ctx->formatStageHits ? ctx->formatStageHits : (4ull << 20);
    constexpr uint32_t kPieceReads = 1u << 20;
    std::vector<uint32_t> cuts(1, 0);                                         // piece k = reads cuts[k] .. cuts[k + 1])
    uint64_t maxHits = 1;
    uint32_t maxReads = 1;
    for (uint32_t i = 0; i < n;) {
        uint32_t e = i + 1;
        while (e < n && e - i < kPieceReads && hit_off[e + 1] - hit_off[i] <= room) ++e;
        maxHits = std::max(maxHits, hit_off[e] - hit_off[i]); maxReads = std::max(maxReads, e - i);
        cuts.push_back(e);
        i = e;
    }
    const size_t pieces = cuts.size() - 1;
    if ((rc = grow(ctx, S->stageHits, maxHits * sizeof(mc_location))) != MC_OK || (rc = grow(ctx, S->stageHitOff, ((uint64_t)maxReads + 1) * 8)) != MC_OK ||
        (rc = grow(ctx, S->stagePieceOff, ((uint64_t)maxReads + 1 + MC_FORMAT_SCRATCH) * 8)) != MC_OK) return rc;
    auto stage = [&](size_t k, MatchArgs& p) -> int {
        const uint32_t r0 = cuts[k], m = cuts[k + 1] - r0;
        const uint64_t nh = hit_off[r0 + m] - hit_off[r0];
        HIP_TRY(ctx, hipMemcpyAsync(S->stageHitOff.p, hit_off + r0, ((uint64_t)m + 1) * 8, hipMemcpyHostToDevice, st));
        if (nh) HIP_TRY(ctx, hipMemcpyAsync(S->stageHits.p, hits + hit_off[r0], nh * sizeof(mc_location), hipMemcpyHostToDevice, st));
        p = make_match_args(*S, flags, m);
        p.hits = (const unsigned long long*)S->stageHits.p; p.hitOff = (const uint64_t*)S->stageHitOff.p; p.hitBias = hit_off[r0];
        p.pieceOff = (uint64_t*)S->stagePieceOff.p;
        launch_match_lengths(ctx, p, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(S->hTotal, p.pieceOff + m, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        return MC_OK;
    };
    MatchArgs p{};
    uint64_t all = 0;
    for (size_t k = 0; k < pieces; ++k) {
        if ((rc = stage(k, p)) != MC_OK) return rc;
        all += *S->hTotal;
    }
    const bool fits = all <= out_capacity;
    uint64_t at = 0;
    for (size_t k = 0; k < pieces; ++k) {
        const uint32_t r0 = cuts[k], m = cuts[k + 1] - r0;
        if (pieces > 1 && (rc = stage(k, p)) != MC_OK) return rc;
        const uint64_t total = *S->hTotal;
        if (fits && (rc = grow(ctx, S->stageOut, std::max<uint64_t>(total, 16))) != MC_OK) return rc;
        p.out = (uint8_t*)S->stageOut.p;
        p.cap = fits ? total : 0;
        launch_match_write(ctx, p, st);
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(piece_off + r0, p.pieceOff, (uint64_t)m * 8, hipMemcpyDeviceToHost, st));
        if (fits && total) HIP_TRY(ctx, hipMemcpyAsync(out + at, S->stageOut.p, total, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, hipStreamSynchronize(st));
        for (uint64_t i = r0; i < (uint64_t)r0 + m; ++i) piece_off[i] += at;
        at += total;
    }
    piece_off[n] = all;
    ++S->matchCalls; S->matchReads += n;
    if (!fits) return fail(ctx, MC_ERR_NOMEM, "mc_format_matches: the pieces need " + std::to_string(all) + " bytes, out has " + std::to_string(out_capacity) + " (piece_off is complete)");
    return MC_OK;
}

int mc_format_matches_stats(mc_ctx* ctx, uint64_t stats[5])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_format_matches_stats: no place for the counters");
    for (int k = 0; k < 5; ++k) stats[k] = 0;
    FormatState* S;
    { std::lock_guard<std::mutex> lock(ctx->formatMtx); S = ctx->format; }
    if (!S) return MC_OK;
    stats[0] = S->matchCalls; stats[1] = S->matchReads;
    if (!ctx->stream || !S->dCounters) return MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int drc = drain_query_streams(ctx)) return drc;
    uint64_t c[kCounters];
    HIP_TRY(ctx, hipMemcpy(c, S->dCounters, sizeof c, hipMemcpyDeviceToHost));
    stats[2] = c[kCtrMatchRuns]; stats[3] = c[kCtrMatchBytes]; stats[4] = c[kCtrMatchBeyond];
    return MC_OK;
}

int mc_format_stats(mc_ctx* ctx, uint64_t stats[5])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_format_stats: no place for the counters");
    for (int k = 0; k < 5; ++k) stats[k] = 0;
    FormatState* S;
    { std::lock_guard<std::mutex> lock(ctx->formatMtx); S = ctx->format; }
    if (!S) return MC_OK;
    stats[0] = S->calls; stats[1] = S->reads;
    if (!ctx->stream || !S->dCounters) return MC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (const int drc = drain_query_streams(ctx)) return drc;
    uint64_t c[kCounters];
    HIP_TRY(ctx, hipMemcpy(c, S->dCounters, sizeof c, hipMemcpyDeviceToHost));
    stats[2] = c[kCtrLines]; stats[3] = c[kCtrBytes]; stats[4] = c[kCtrOutOfTable];
    return MC_OK;
}

}  // extern "C"
