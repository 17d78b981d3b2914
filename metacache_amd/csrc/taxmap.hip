// metacache_amd/csrc/taxmap.hip -- mc_taxmap_*: the rows of accession2taxid tables matched against the target names on the device
// (DESIGN.md 7k).  The rules -- the names, the target of a row, the winner, the line rule -- are those of include/metacache_amd.h
// (try_to_rank_unranked_targets of mcq_build.h, after building.cpp:85-149 and taxonomy.hpp:1108-1127); a line outside the line rule
// makes the range IRREGULAR and nothing but status changes.
//
// A row names its target by itself and the winner of a name is the FIRST row in the order of calls and bytes, so the result is a minimum
// over {call, line start} and nothing is carried from line to line.  A tile is kTile consecutive bytes, a block owns a tile, a thread 16
// consecutive bytes of it (one 16-byte load) and every line that STARTS in them; the lane walks a line byte by byte, at most
// kMaxLine + 1 bytes far.  The passes of one mc_taxmap_add, enqueued back to back and never waited for:
//   1. taxmap_validate_kernel  per tile: lines counted, every line judged, the smallest offending line start (atomicMax of its inverse)
//   2. taxmap_match_kernel     per tile, where pass 1 found no offence: tokens cut, the target by the three ordered searches over
//                              the 8-byte name prefixes (full compare on prefix ties), atomicMin of {call, line start} on a wanted name's key
//   3. taxmap_finish_kernel    per name: a key of this call -> the taxid of its line is parsed and stored; newly ranked names and
//                              names still wanted are counted
//   4. taxmap_status_kernel    one thread: status and the context's counters
// No atomic decides anything but a minimum, a maximum or a sum, so the same calls give the same bytes.  Plain HIP C++; no inline assembly.
#include "parse_scan.h"

#include <cstring>

using namespace mcamd;
using namespace mcamd::parsek;

namespace {

constexpr uint32_t kMaxBlocks = 2048, kMaxLine = 1024, kMaxDigits = 18;
constexpr uint64_t kScratchBytes = 256, kNoKey = ~0ull;
constexpr uint64_t kMaxNames = 1ull << 31, kMaxNameBytes = 0xFFFFFFFFull;
// the call's workspace, in 32-bit words (zeroed in front of pass 1)
enum { wLines = 0, wOffenceInv /* kNone - offence; 0: none */, wTargeted, wWanted, wNewly, wStill };
// the context's device counters
enum { cLines = 0, cTargeted, cWanted, cRanked, cRefused, cCounters };

struct TaxmapArgs {
    const uint8_t* B;
    uint32_t* ws;
    uint64_t* status;
    unsigned long long* counters;
    const uint8_t* names; const uint32_t* nameOff; const uint64_t* prefix; const uint8_t* wanted;   // the names ascending
    unsigned long long* key; int64_t* taxid;                                                        // per name
    uint32_t n, count, callNo;
};

// the line rule on the line that starts at s; tok[k] / len[k]: where token k begins and how long it is (filled as far as the line is regular)
__device__ __forceinline__ bool cut_line(const TaxmapArgs& a, uint32_t s, uint32_t tok[4], uint32_t len[4])
{
    const uint32_t limit = s + kMaxLine;                       // the line's last byte lies below this
    uint32_t p = s, c;
    for (int k = 0; k < 4; ++k) {
        while (is_blank(c = byte_at(a.B, a.n, p))) if (++p > limit) return false;
        tok[k] = p;
        for (; (c = byte_at(a.B, a.n, p)) != '\n' && !is_blank(c); ++p) {
            if (is_refused(c) || p >= limit) return false;
            if (k == 2 && (!is_digit(c) || p - tok[k] >= kMaxDigits)) return false;
        }
        len[k] = p - tok[k];
        if (!len[k]) return false;                             // (an empty or blank-only line; fewer than four tokens)
    }
    while (is_blank(c = byte_at(a.B, a.n, p))) if (++p > limit) return false;
    return c == '\n';                                          // (anything else: a fifth token or a refused byte)
}

// the first 8 bytes of a string, big-endian, zeros behind its end: ordered as the strings are wherever two prefixes differ
__device__ __forceinline__ uint64_t prefix_of(const uint8_t* s, uint32_t len)
{
    uint64_t v = 0;
#pragma unroll
    for (uint32_t k = 0; k < 8; ++k) v = (v << 8) | (k < len ? (uint64_t)s[k] : 0ull);
    return v;
}

// std::string::compare of name i with the token: < 0, 0, > 0
__device__ __forceinline__ int compare_name(const TaxmapArgs& a, uint32_t i, const uint8_t* t, uint32_t tlen)
{
    const uint32_t off = a.nameOff[i], nlen = a.nameOff[i + 1] - off, m = min(nlen, tlen);
    const uint8_t* s = a.names + off;
    for (uint32_t k = 0; k < m; ++k) if (s[k] != t[k]) return s[k] < t[k] ? -1 : 1;
    return nlen < tlen ? -1 : nlen > tlen ? 1 : 0;
}

// the first name that is not below the token (UPPER: that is above it); count: none
template <bool UPPER>
__device__ __forceinline__ uint32_t bound_of(const TaxmapArgs& a, const uint8_t* t, uint32_t tlen)
{
    const uint64_t pt = prefix_of(t, tlen);
    uint32_t lo = 0, hi = a.count;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        const uint64_t pm = a.prefix[mid];
        bool below;                                            // name mid < token (UPPER: <= token)
        if (pm != pt) below = pm < pt;
        else { const int c = compare_name(a, mid, t, tlen); below = UPPER ? c <= 0 : c < 0; }
        if (below) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint32_t name_equal_to(const TaxmapArgs& a, const uint8_t* t, uint32_t tlen)
{
    const uint32_t i = bound_of<false>(a, t, tlen);
    return (i < a.count && compare_name(a, i, t, tlen) == 0) ? i : kNone;
}

// taxon_with_similar_name: the smallest name above the token, if the token is a prefix of it
__device__ __forceinline__ uint32_t name_similar_to(const TaxmapArgs& a, const uint8_t* t, uint32_t tlen)
{
    const uint32_t i = bound_of<true>(a, t, tlen);
    if (i >= a.count) return kNone;
    const uint32_t off = a.nameOff[i], nlen = a.nameOff[i + 1] - off;
    if (nlen < tlen) return kNone;
    for (uint32_t k = 0; k < tlen; ++k) if (a.names[off + k] != t[k]) return kNone;
    return i;
}

// ---- the passes -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void taxmap_validate_kernel(TaxmapArgs a)
{
    const uint32_t p0 = blockIdx.x * kTile + threadIdx.x * 16u;
    uint32_t lines = 0, offenceInv = 0;
    for_each_line_start(a.B, a.n, p0, [&](uint32_t s) {
        uint32_t tok[4], len[4];
        ++lines;
        if (!cut_line(a, s, tok, len)) offenceInv = max(offenceInv, kNone - s);
    });
    lines = wave_sum_u32(lines); offenceInv = wave_max_u32(offenceInv);
    if ((threadIdx.x & 63u) == 0) {                            // (a sum and a maximum: the same whatever the order)
        if (lines) atomicAdd(&a.ws[wLines], lines);
        if (offenceInv) atomicMax(&a.ws[wOffenceInv], offenceInv);
    }
}

__global__ __launch_bounds__(kBlock) void taxmap_match_kernel(TaxmapArgs a)
{
    if (a.ws[wOffenceInv] != 0 || a.count == 0) return;        // (the same for every thread of the grid)
    const uint32_t p0 = blockIdx.x * kTile + threadIdx.x * 16u;
    uint32_t targeted = 0, wanted = 0;
    for_each_line_start(a.B, a.n, p0, [&](uint32_t s) {
        uint32_t tok[4], len[4];
        if (!cut_line(a, s, tok, len)) return;                 // (cannot happen without an offence)
        uint32_t t = name_equal_to(a, a.B + tok[1], len[1]);
        if (t == kNone) t = name_similar_to(a, a.B + tok[0], len[0]);
        if (t == kNone) t = name_equal_to(a, a.B + tok[3], len[3]);
        if (t == kNone) return;
        ++targeted;
        if (!a.wanted[t]) return;
        ++wanted;
        atomicMin(&a.key[t], ((unsigned long long)a.callNo << 32) | s);   // (a minimum: the same whatever the order)
    });
    targeted = wave_sum_u32(targeted); wanted = wave_sum_u32(wanted);
    if ((threadIdx.x & 63u) == 0) {
        if (targeted) atomicAdd(&a.ws[wTargeted], targeted);
        if (wanted) atomicAdd(&a.ws[wWanted], wanted);
    }
}

__global__ __launch_bounds__(kBlock) void taxmap_finish_kernel(TaxmapArgs a)
{
    const bool ok = a.ws[wOffenceInv] == 0;
    const uint32_t step = gridDim.x * kBlock;
    uint32_t newly = 0, still = 0;
    for (uint32_t base = blockIdx.x * kBlock; base < a.count; base += step) {      // (the same trips for every lane of a block)
        const uint32_t i = base + threadIdx.x;
        if (i >= a.count) continue;
        const unsigned long long k = a.key[i];
        if (k == kNoKey) { still += a.wanted[i] ? 1u : 0u; continue; }
        if (!ok || (uint32_t)(k >> 32) != a.callNo) continue;
        uint32_t tok[4], len[4];
        int64_t v = 0;
        if (cut_line(a, (uint32_t)k, tok, len))
            for (uint32_t j = 0; j < len[2]; ++j) v = v * 10 + (int64_t)(a.B[tok[2] + j] - '0');
        a.taxid[i] = v;
        ++newly;
    }
    newly = wave_sum_u32(newly); still = wave_sum_u32(still);
    if ((threadIdx.x & 63u) == 0) {
        if (newly) atomicAdd(&a.ws[wNewly], newly);
        if (still) atomicAdd(&a.ws[wStill], still);
    }
}

__global__ void taxmap_status_kernel(TaxmapArgs a)
{
    if (blockIdx.x || threadIdx.x) return;
    const uint32_t inv = a.ws[wOffenceInv];
    a.status[0] = a.ws[wLines]; a.status[1] = a.ws[wTargeted]; a.status[2] = a.ws[wWanted]; a.status[3] = a.ws[wNewly]; a.status[4] = a.ws[wStill];
    a.status[5] = inv ? MC_TAXMAP_IRREGULAR : MC_TAXMAP_OK; a.status[6] = inv ? kNone - inv : 0; a.status[7] = 0;
    if (inv) { atomicAdd(&a.counters[cRefused], 1ull); return; }
    atomicAdd(&a.counters[cLines], (unsigned long long)a.ws[wLines]);
    atomicAdd(&a.counters[cTargeted], (unsigned long long)a.ws[wTargeted]);
    atomicAdd(&a.counters[cWanted], (unsigned long long)a.ws[wWanted]);
    atomicAdd(&a.counters[cRanked], (unsigned long long)a.ws[wNewly]);
}

}  // namespace

namespace mcamd {

struct TaxmapState {                     // what the context keeps for mc_taxmap_*
    // mc_taxmap_begin: the names, their offsets, 8-byte prefixes and wanted flags; the key and the taxid of each
    uint8_t* dNames = nullptr; uint32_t* dOff = nullptr; uint64_t* dPrefix = nullptr; uint8_t* dWanted = nullptr;
    unsigned long long* dKey = nullptr; int64_t* dTaxid = nullptr;
    uint32_t count = 0, callNo = 0;
    bool begun = false;
    unsigned long long* dCounters = nullptr;
    uint64_t calls = 0, bytes = 0;
    DevBuf stageIn, stageWs;
    StatusStage status;                  // [8]
};

void free_taxmap_state(mc_ctx* ctx)
{
    if (!ctx->taxmap) return;
    TaxmapState& S = *ctx->taxmap;
    for (void* p : {(void*)S.dNames, (void*)S.dOff, (void*)S.dPrefix, (void*)S.dWanted, (void*)S.dKey, (void*)S.dTaxid, (void*)S.dCounters,
                    S.stageIn.p, S.stageWs.p})
        if (p) (void)hipFree(p);
    free_status_stage(S.status);
    delete ctx->taxmap;
    ctx->taxmap = nullptr;
}

}  // namespace mcamd

namespace {

void free_names(TaxmapState& S)
{
    for (void* p : {(void*)S.dNames, (void*)S.dOff, (void*)S.dPrefix, (void*)S.dWanted, (void*)S.dKey, (void*)S.dTaxid}) if (p) (void)hipFree(p);
    S.dNames = nullptr; S.dOff = nullptr; S.dPrefix = nullptr; S.dWanted = nullptr; S.dKey = nullptr; S.dTaxid = nullptr;
    S.count = 0; S.begun = false;
}

// the four passes of one range, nothing waited for
int enqueue_add(mc_ctx* ctx, TaxmapState& S, const uint8_t* dBytes, uint32_t n, uint64_t* dStatus, void* ws, hipStream_t st)
{
    TaxmapArgs a{};
    a.B = dBytes; a.ws = (uint32_t*)ws; a.status = dStatus; a.counters = S.dCounters;
    a.names = S.dNames; a.nameOff = S.dOff; a.prefix = S.dPrefix; a.wanted = S.dWanted; a.key = S.dKey; a.taxid = S.dTaxid;
    a.n = n; a.count = S.count; a.callNo = S.callNo++;
    const uint32_t tiles = tiles_of(n);
    HIP_TRY(ctx, hipMemsetAsync(ws, 0, kScratchBytes, st));
    {
        ScopedTimer timer(ctx, "taxmap_validate", st);
        hipLaunchKernelGGL(taxmap_validate_kernel, dim3(tiles), dim3(kBlock), 0, st, a);
    }
    {
        ScopedTimer timer(ctx, "taxmap_match", st);
        hipLaunchKernelGGL(taxmap_match_kernel, dim3(tiles), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(taxmap_finish_kernel, dim3(row_blocks(std::max<uint64_t>(S.count, 1), kBlock, kMaxBlocks)), dim3(kBlock), 0, st, a);
        hipLaunchKernelGGL(taxmap_status_kernel, dim3(1), dim3(64), 0, st, a);
    }
    HIP_TRY(ctx, hipGetLastError());
    ++S.calls; S.bytes += n;
    return MC_OK;
}

// what every call behind mc_taxmap_begin needs of the context, after its own argument checks
int taxmap_state(mc_ctx* ctx, const char* who, TaxmapState** out)
{
    const std::string name = who;
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, name + ": the context has no device (mc_open_metadata)");
    TaxmapState* S = ctx->taxmap;
    if (!S || !S->begun) return fail(ctx, MC_ERR_STATE, name + ": no names (mc_taxmap_begin)");
    *out = S;
    return MC_OK;
}

}  // namespace

extern "C" {

const uint32_t mc_taxmap_tile = kTile;
const uint32_t mc_taxmap_max_line = kMaxLine;

uint64_t mc_taxmap_scratch_bytes(uint64_t nbytes) { (void)nbytes; return kScratchBytes; }

int mc_taxmap_begin(mc_ctx* ctx, const char* names, const uint64_t* nameOff, uint64_t count, const uint8_t* wanted)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (!nameOff) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: no offsets");
    if (count && !wanted) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: no wanted flags");
    if (count >= kMaxNames) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: more than 2^31 - 1 names");
    for (uint64_t i = 0; i < count; ++i)
        if (nameOff[i + 1] < nameOff[i]) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: the offsets must not descend (name " + std::to_string(i) + ")");
    const uint64_t base = nameOff[0], total = nameOff[count] - base;
    if (total && !names) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: no names");
    if (total > kMaxNameBytes) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: more than 2^32 - 1 bytes of names");
    const uint8_t* nb = (const uint8_t*)names;
    for (uint64_t i = 1; i < count; ++i) {                      // strictly ascending as std::string::compare orders them
        const uint64_t la = nameOff[i] - nameOff[i - 1], lb = nameOff[i + 1] - nameOff[i];
        const int c = std::memcmp(nb + nameOff[i - 1], nb + nameOff[i], (size_t)std::min(la, lb));
        if (c > 0 || (c == 0 && la >= lb)) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_begin: the names must ascend strictly (name " + std::to_string(i) + ")");
    }
    // ... then state
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_taxmap_begin: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->taxmap) ctx->taxmap = new TaxmapState;
    TaxmapState& S = *ctx->taxmap;
    HIP_TRY(ctx, hipDeviceSynchronize());                       // (calls that still run finish with the old names)
    free_names(S);
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, cCounters * 8));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, cCounters * 8));
    }
    if (const int rc = make_status_stage(ctx, S.status, 8)) return rc;
    const uint64_t rows = std::max<uint64_t>(count, 1);
    std::vector<uint32_t> off(count + 1);
    std::vector<uint64_t> prefix(rows, 0);
    for (uint64_t i = 0; i <= count; ++i) off[i] = (uint32_t)(nameOff[i] - base);
    for (uint64_t i = 0; i < count; ++i) {
        const uint64_t len = nameOff[i + 1] - nameOff[i];
        uint64_t v = 0;
        for (uint64_t k = 0; k < 8; ++k) v = (v << 8) | (k < len ? (uint64_t)nb[nameOff[i] + k] : 0ull);
        prefix[i] = v;
    }
    HIP_TRY(ctx, hipMalloc((void**)&S.dNames, std::max<uint64_t>(total, 1)));
    HIP_TRY(ctx, hipMalloc((void**)&S.dOff, (count + 1) * 4));
    HIP_TRY(ctx, hipMalloc((void**)&S.dPrefix, rows * 8));
    HIP_TRY(ctx, hipMalloc((void**)&S.dWanted, rows));
    HIP_TRY(ctx, hipMalloc((void**)&S.dKey, rows * 8));
    HIP_TRY(ctx, hipMalloc((void**)&S.dTaxid, rows * 8));
    if (total) HIP_TRY(ctx, hipMemcpy(S.dNames, nb + base, total, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(S.dOff, off.data(), (count + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(S.dPrefix, prefix.data(), rows * 8, hipMemcpyHostToDevice));
    if (count) HIP_TRY(ctx, hipMemcpy(S.dWanted, wanted, count, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemset(S.dKey, 0xFF, rows * 8));
    HIP_TRY(ctx, hipMemset(S.dTaxid, 0, rows * 8));
    HIP_TRY(ctx, hipDeviceSynchronize());
    S.count = (uint32_t)count; S.callNo = 0;
    S.begun = true;
    return MC_OK;
}

int mc_taxmap_add(mc_ctx* ctx, const char* bytes, uint64_t nbytes, int flags, uint64_t status[8], void* workspace, uint64_t workspaceBytes, void* streamv)
{
    // arguments first ...
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_TAXMAP_HOST) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: unknown flag");
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: no bytes");
    if (nbytes > (1ull << 31)) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: more than 2^31 bytes in one range");
    if (!status) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: no status");
    const bool host = (flags & MC_TAXMAP_HOST) != 0;
    if (!host) {
        if (!workspace || workspaceBytes < kScratchBytes) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: the workspace is smaller than mc_taxmap_scratch_bytes");
        if (((uintptr_t)bytes | (uintptr_t)workspace) & 15u) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: device arrays must be aligned (bytes, workspace: 16 bytes)");
        if ((uintptr_t)status & 7u) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_add: device arrays must be aligned (status: 8 bytes)");
    }
    // ... then state
    TaxmapState* S = nullptr;
    int rc = taxmap_state(ctx, "mc_taxmap_add", &S);
    if (rc) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    if (!host) return enqueue_add(ctx, *S, (const uint8_t*)bytes, (uint32_t)nbytes, status, workspace, st);
    if ((rc = grow(ctx, S->stageWs, kScratchBytes)) != MC_OK || (rc = stage_bytes(ctx, S->stageIn, bytes, nbytes, st)) != MC_OK) return rc;
    if ((rc = enqueue_add(ctx, *S, (const uint8_t*)S->stageIn.p, (uint32_t)nbytes, (uint64_t*)S->status.dev.p, S->stageWs.p, st)) != MC_OK) return rc;
    return read_status(ctx, S->status, 8, status, st);
}

int mc_taxmap_result(mc_ctx* ctx, int64_t* taxid, uint64_t* position, uint64_t* remaining, int flags, void* streamv)
{
    if (!ctx) return MC_ERR_INVALID;
    if (flags & ~MC_TAXMAP_HOST) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_result: unknown flag");
    const bool host = (flags & MC_TAXMAP_HOST) != 0;
    if (!host && (((uintptr_t)taxid | (uintptr_t)position | (uintptr_t)remaining) & 7u)) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_result: device arrays must be aligned (8 bytes)");
    if (!host && remaining) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_result: the number of names still wanted is a host value (MC_TAXMAP_HOST)");
    TaxmapState* S = nullptr;
    if (const int rc = taxmap_state(ctx, "mc_taxmap_result", &S)) return rc;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const hipMemcpyKind kind = host ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice;
    const uint64_t n = S->count;
    if (!host) {
        if (n && taxid) HIP_TRY(ctx, hipMemcpyAsync(taxid, S->dTaxid, n * 8, kind, st));
        if (n && position) HIP_TRY(ctx, hipMemcpyAsync(position, S->dKey, n * 8, kind, st));
        return MC_OK;
    }
    // the host form reads the keys in any case: `remaining` is counted from them
    std::vector<uint64_t> keys(n);
    std::vector<uint8_t> wanted(n);
    if (n && taxid) HIP_TRY(ctx, hipMemcpyAsync(taxid, S->dTaxid, n * 8, kind, st));
    if (n) HIP_TRY(ctx, hipMemcpyAsync(keys.data(), S->dKey, n * 8, kind, st));
    if (n && remaining) HIP_TRY(ctx, hipMemcpyAsync(wanted.data(), S->dWanted, n, kind, st));
    HIP_TRY(ctx, hipStreamSynchronize(st));
    if (position) std::copy(keys.begin(), keys.end(), position);
    if (remaining) {
        uint64_t r = 0;
        for (uint64_t i = 0; i < n; ++i) r += wanted[i] && keys[i] == kNoKey;
        *remaining = r;
    }
    return MC_OK;
}

int mc_taxmap_stats(mc_ctx* ctx, uint64_t stats[8])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!stats) return fail(ctx, MC_ERR_INVALID, "mc_taxmap_stats: no place for the counters");
    for (int i = 0; i < 8; ++i) stats[i] = 0;
    TaxmapState* S = ctx->taxmap;
    if (!S) return MC_OK;
    stats[0] = S->calls; stats[1] = S->bytes;
    if (S->dCounters) {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        HIP_TRY(ctx, hipDeviceSynchronize());
        unsigned long long c[cCounters];
        HIP_TRY(ctx, hipMemcpy(c, S->dCounters, sizeof c, hipMemcpyDeviceToHost));
        stats[2] = c[cLines]; stats[3] = c[cTargeted]; stats[4] = c[cWanted]; stats[5] = c[cRanked]; stats[6] = c[cRefused];
    }
    return MC_OK;
}

void mc_taxmap_end(mc_ctx* ctx)
{
    if (!ctx || !ctx->taxmap) return;
    if (ctx->stream) { (void)hipSetDevice(ctx->device); (void)hipDeviceSynchronize(); }
    free_names(*ctx->taxmap);
}

}  // extern "C"
