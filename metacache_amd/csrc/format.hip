// metacache_amd/csrc/format.hip -- mc_format_set_text / mc_format_mappings / mc_format_stats: the per-read mapping lines of `metacache query`
// (show_query_mapping, classification.cpp:432-523; show_candidates / show_candidate_ranges, printing.cpp:283-380) rendered on the
// device, behind the query and the vote.  What a line is, piece by piece: include/metacache_amd.h.
//
// THREE LAUNCHES, none of which waits for another block:
//   1. format_lengths_kernel: one lane per read walks the read's pieces and adds up their lengths (exact: digit counts, string lengths
//      from the tables) into line_off[i]; block b owns TILE b, a run of consecutive reads, and leaves the tile's sum in the workspace
//      behind line_off (MC_FORMAT_SCRATCH entries, so at most that many tiles: a tile grows with the batch instead of the grid).
//   2. format_scan_kernel: ONE block turns the tile sums into tile offsets and stores the total in line_off[n].
//   3. format_write_kernel: block b scans its tile's lengths into line_off (chunks of 256 reads, a running offset), and -- unless the
//      total exceeds the capacity -- renders the chunk's lines.  Consecutive reads' lines are consecutive in `out`, so a chunk owns one
//      byte range [c0, c1): the block walks it in WINDOWS of kStage bytes that begin at multiples of 16, every lane stores the part of
//      its line that falls into the window into LDS (the same walk as pass 1, clipped), and the block moves the window out in 16-byte
//      lane-consecutive stores; the 16-byte slots at the range's two ends that the chunk owns only partly go out byte by byte.  A line of
//      any length takes this path -- it simply spans more windows, its lane walking it once per window with whole pieces skipped by
//      arithmetic -- so there is no second, direct path to keep equal to the first.
// Plain HIP C++; no inline assembly.
#include "rows_common.h"

#include <algorithm>
#include <atomic>
#include <cstring>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kMaxTiles = MC_FORMAT_SCRATCH, kStage = 32768;
constexpr int kAllFlags = MC_FORMAT_HOST | MC_FORMAT_QUERY_IDS | MC_FORMAT_TRUTH | MC_FORMAT_TOPHITS | MC_FORMAT_LOCATIONS | MC_FORMAT_MAPPED_ONLY;
constexpr uint32_t kCtrLines = 0, kCtrBytes = 1, kCtrOutOfTable = 2, kCounters = 3;
static_assert(sizeof(mc_candidate) == 16 && sizeof(mc_assignment) == 8, "ABI sizes");
static_assert(kStage % 16 == 0, "windows begin at multiples of 16");

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

// the one walk over a read's pieces that both passes take.  beyond: result indices that lay beyond their table (the caller counts them once per line)
template <bool WRITE>
__device__ __forceinline__ void walk_line(const FmtArgs& a, uint64_t i, Sink<WRITE>& s, uint32_t& beyond)
{
    const uint2 as = reinterpret_cast<const uint2*>(a.assigned)[i];              // {taxon, info}
    if ((a.flags & MC_FORMAT_MAPPED_ONLY) && as.x == 0) return;
    const mc_candidate* row = a.cands ? a.cands + i * a.stride : nullptr;
    if (a.flags & MC_FORMAT_QUERY_IDS) { s.num(a.ids ? a.ids[i] : a.firstId + i); s.column(a); }
    {
        const uint64_t b = a.nameOff[i], e = a.nameOff[i + 1];
        s.bytes(a.names + (b - a.nameBias), e > b ? e - b : 0);
        s.column(a);
    }
    if (a.flags & MC_FORMAT_TRUTH) { result_text(a, s, a.truth[i], beyond); s.column(a); }
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

// exclusive scan of one 64-bit value per thread of the block; total = the block's sum.  sc: kBlock entries of LDS.
__device__ __forceinline__ uint64_t block_excl_scan(uint64_t v, uint64_t* sc, uint64_t& total)
{
    const uint32_t t = threadIdx.x;
    sc[t] = v;
    __syncthreads();
    for (uint32_t d = 1; d < kBlock; d <<= 1) {
        const uint64_t add = t >= d ? sc[t - d] : 0;
        __syncthreads();
        sc[t] += add;
        __syncthreads();
    }
    total = sc[kBlock - 1];
    const uint64_t incl = sc[t];
    __syncthreads();
    return incl - v;
}

__global__ __launch_bounds__(kBlock) void format_lengths_kernel(FmtArgs a)
{
    __shared__ uint64_t sc[kBlock];
    const uint64_t t0 = (uint64_t)blockIdx.x * a.tileReads, t1 = min(t0 + (uint64_t)a.tileReads, (uint64_t)a.n);
    uint64_t mine = 0;
    for (uint64_t i = t0 + threadIdx.x; i < t1; i += kBlock) {
        Sink<false> s{nullptr, 0, 0, 0};
        uint32_t beyond = 0;
        walk_line<false>(a, i, s, beyond);
        a.lineOff[i] = s.pos;
        mine += s.pos;
    }
    uint64_t total;
    (void)block_excl_scan(mine, sc, total);
    if (threadIdx.x == 0) a.lineOff[(uint64_t)a.n + 1 + blockIdx.x] = total;
}

__global__ __launch_bounds__(kBlock) void format_scan_kernel(FmtArgs a)
{
    __shared__ uint64_t sc[kBlock];
    uint64_t* sums = a.lineOff + (uint64_t)a.n + 1;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < a.tiles; base += kBlock) {                    // (the same trips for every lane)
        const uint32_t j = base + threadIdx.x;
        const uint64_t v = j < a.tiles ? sums[j] : 0;
        uint64_t total;
        const uint64_t excl = block_excl_scan(v, sc, total);
        if (j < a.tiles) sums[j] = carry + excl;
        carry += total;
    }
    if (threadIdx.x == 0) a.lineOff[a.n] = carry;
}

__global__ __launch_bounds__(kBlock) void format_write_kernel(FmtArgs a)
{
    __shared__ uint64_t sc[kBlock];
    __shared__ __attribute__((aligned(16))) uint8_t stage[kStage];
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
        for (uint64_t w = c0 & ~15ull; w < c1; w += kStage) {
            const uint64_t w1 = min(w + (uint64_t)kStage, c1);
            if (len && off < w1 && off + len > w) {
                Sink<true> s{stage, off, w, w1};
                uint32_t beyond = 0;
                walk_line<true>(a, i, s, beyond);
                if (beyond && off + len <= w1) atomicAdd(&beyondAll, beyond);    // (counted where the line ENDS: the one window whose walk goes through all its pieces)
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
    DevBuf stageCands, stageAssigned, stageTruth, stageIds, stageNames, stageNameOff, stageLineOff, stageOut;
    uint64_t* hTotal = nullptr;          // pinned: a piece's total
};

void free_format_state(mc_ctx* ctx)
{
    if (!ctx->format) return;
    FormatState& S = *ctx->format;
    for (DevText& d : S.dev) { if (d.bytes) (void)hipFree(d.bytes); if (d.off) (void)hipFree(d.off); }
    if (S.dCounters) (void)hipFree(S.dCounters);
    if (S.hTotal) (void)hipHostFree(S.hTotal);
    for (DevBuf* b : {&S.stageCands, &S.stageAssigned, &S.stageTruth, &S.stageIds, &S.stageNames, &S.stageNameOff, &S.stageLineOff, &S.stageOut})
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
    for (int w = 0; w < 3; ++w) {
        const HostText& h = S.host[w];
        DevText& d = S.dev[w];
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
    hipLaunchKernelGGL(format_lengths_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
    hipLaunchKernelGGL(format_scan_kernel, dim3(1), dim3(kBlock), 0, st, a);
}
void launch_write(mc_ctx* ctx, const FmtArgs& a, hipStream_t st)
{
    ScopedTimer timer(ctx, "format_write", st);
    hipLaunchKernelGGL(format_write_kernel, dim3(a.tiles), dim3(kBlock), 0, st, a);
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
                       uint32_t n, int flags, char* out, uint64_t out_capacity, uint64_t* line_off, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!opt) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: no options");
    if (flags & ~kAllFlags) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: unknown flag");
    if (stride == 0) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: stride == 0");
    if (opt->column_len > 16) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: a column separator has at most 16 bytes");
    if (!line_off) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: no line_off");
    if ((flags & MC_FORMAT_TRUTH) && n > 0 && !truth) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: MC_FORMAT_TRUTH without truth");
    if (n > 0 && (!cands || !assigned || !name_off)) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: null array");
    if (out_capacity > 0 && !out) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: no out");
    const bool host = (flags & MC_FORMAT_HOST) != 0;
    if (host && n > 0 && name_off[n] > name_off[0] && !names) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: no names");
    if (!host) {
        if (((uintptr_t)out | (uintptr_t)cands) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: device arrays must be aligned (out and cands: 16 bytes)");
        if (((uintptr_t)assigned | (uintptr_t)query_ids | (uintptr_t)name_off | (uintptr_t)line_off) & 7u) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: device arrays must be aligned (assigned, query_ids, name_off, line_off: 8 bytes)");
        if ((uintptr_t)truth & 3u) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: device arrays must be aligned (truth: 4 bytes)");
    }
    if (n > 0 && out_capacity > 0) {
        const uintptr_t o0 = (uintptr_t)out, o1 = o0 + out_capacity;
        auto hits = [&](const void* p, uint64_t bytes) { return p && ranges_overlap((uintptr_t)p, (uintptr_t)p + std::max<uint64_t>(bytes, 1), o0, o1); };
        const uint64_t nameBytes = host ? name_off[n] - name_off[0] : 1;           // (device form: the names' extent lies on the device; their first byte is looked at)
        if (hits(cands, (uint64_t)n * stride * sizeof(mc_candidate)) || hits(assigned, (uint64_t)n * sizeof(mc_assignment)) || hits(truth, (uint64_t)n * 4) ||
            hits(query_ids, (uint64_t)n * 8) || hits(names, nameBytes) || hits(name_off, ((uint64_t)n + 1) * 8) ||
            hits(line_off, ((uint64_t)n + 1 + (host ? 0 : MC_FORMAT_SCRATCH)) * 8))
            return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: out overlaps an input or line_off");
    }
    if (n == 0 && host) { line_off[0] = 0; return MC_OK; }
    // ... then state
    {
        std::lock_guard<std::mutex> lock(ctx->formatMtx);
        const FormatState* S = ctx->format;
        if (!S || !S->host[MC_TEXT_RESULT].set) return fail(ctx, MC_ERR_STATE, "mc_format_mappings: the context has no MC_TEXT_RESULT table (mc_format_set_text)");
        if ((flags & MC_FORMAT_TOPHITS) && !S->host[MC_TEXT_CANDIDATE].set) return fail(ctx, MC_ERR_STATE, "mc_format_mappings: MC_FORMAT_TOPHITS needs the MC_TEXT_CANDIDATE table (mc_format_set_text)");
    }
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_format_mappings: the context has no device (mc_open_metadata)");
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
    uint64_t maxNames = 0;
    for (uint64_t done = 0; done < n; done += piece) {
        const uint64_t m = std::min<uint64_t>(piece, n - done);
        if (name_off[done + m] < name_off[done]) return fail(ctx, MC_ERR_INVALID, "mc_format_mappings: name_off must not decrease");
        maxNames = std::max(maxNames, name_off[done + m] - name_off[done]);
    }
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
        p = a;
        p.n = m; tiles_of(m, p.tileReads, p.tiles);
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
    if (!fits) return fail(ctx, MC_ERR_NOMEM, "mc_format_mappings: the lines need " + std::to_string(all) + " bytes, out has " + std::to_string(out_capacity) + " (line_off is complete)");
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
