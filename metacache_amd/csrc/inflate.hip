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
// Plain HIP C++; no inline assembly.
#include "rows_common.h"
#include "bgzf_rules.h"

#include <atomic>
#include <cstring>
#include <vector>

using namespace mcamd;

namespace {

constexpr uint32_t kBlock = 256, kWaves = kBlock / 64;
constexpr uint32_t kLitFast = 10, kDistFast = 8, kClFast = 7;      // bits of the fast tables (a code-length code has at most 7 bits: its table is complete)
constexpr uint32_t kCrcPoly = 0xEDB88320u;
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

// entry of a fast table / result of a decode: symbol << 4 | code length; 0 = no symbol
struct WaveTables {
    uint16_t litFast[1u << kLitFast];
    uint16_t distFast[1u << kDistFast];   // the code-length code's fast table while a dynamic header is read
    uint16_t litSym[288], distSym[32];    // symbols ordered by (length, symbol); distSym holds the code-length code's 19 first
    uint16_t litCnt[16], distCnt[16];     // codes per length
    uint8_t lens[320];                    // the code lengths as the header gives them: HLIT, then HDIST; [0, 19) the code-length code's first
};

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ uint64_t uni64(uint64_t v) { return (uint64_t)uni((uint32_t)v) | ((uint64_t)uni((uint32_t)(v >> 32)) << 32); }
// other lanes of this wave read what this lane wrote (LDS or global): the wave's operations are performed in order, the compiler must keep it
__device__ __forceinline__ void wave_order()
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// ---- the bit reader: wave-uniform.  buf holds `have` bits, the stream's next bit lowest; left = unread bits of the payload --------------
struct Bits {
    const uint32_t* w;        // the next aligned word
    const uint32_t* wend;     // the words that lie wholly inside the member end here: beyond, zeros are read
    uint64_t buf;
    uint32_t have, left;
};

// B is 16-byte aligned; at = offset of the payload's next byte
__device__ __forceinline__ void bits_start(Bits& b, const uint8_t* B, uint64_t at, uint64_t memberEnd, uint32_t leftBits)
{
    b.w = (const uint32_t*)B + (at >> 2);
    b.wend = (const uint32_t*)B + (memberEnd >> 2);
    const uint32_t sh = ((uint32_t)at & 3u) * 8u;
    const uint32_t x = b.w < b.wend ? uni(*b.w) : 0u;
    ++b.w;
    b.buf = x >> sh; b.have = 32u - sh; b.left = leftBits;
}
// the next n <= 32 bits, those beyond the payload as zeros
__device__ __forceinline__ uint32_t bits_peek(Bits& b, uint32_t n)
{
    if (b.have <= 32u) {
        const uint32_t x = b.w < b.wend ? uni(*b.w) : 0u;
        ++b.w;
        b.buf |= (uint64_t)x << b.have; b.have += 32u;
    }
    const uint32_t m = min(n, b.left);
    return (uint32_t)(b.buf & ((1ull << m) - 1ull));
}
__device__ __forceinline__ void bits_drop(Bits& b, uint32_t n) { b.buf >>= n; b.have -= n; b.left -= n; }   // n <= left, n <= have: the caller has peeked

// ---- canonical codes ---------------------------------------------------------------------------------
// the symbol whose code the low bits of v begin with, codes up to maxBits long: symbol << 4 | length, 0 = none
__device__ __forceinline__ uint32_t canon_decode(const uint16_t* cnt, const uint16_t* sym, uint32_t v, uint32_t maxBits)
{
    uint32_t code = 0, first = 0, index = 0;
    for (uint32_t len = 1; len <= maxBits; ++len) {
        code |= v & 1u; v >>= 1;
        const uint32_t c = cnt[len];
        if (code < first + c) return ((uint32_t)sym[index + (code - first)] << 4) | len;
        index += c; first = (first + c) << 1; code <<= 1;
    }
    return 0;
}

enum { CODE_OK = 0, CODE_OVER = 1, CODE_INCOMPLETE = 2 };

// lens[0, n) -> cnt, sym, fast.  CH = ceil(most symbols / 64).  All lanes call it.
template <uint32_t CH, uint32_t FB>
__device__ __forceinline__ int build_code(const uint8_t* lens, uint32_t n, uint16_t* cnt, uint16_t* sym, uint16_t* fast, uint32_t lane, uint32_t& maxLen)
{
    uint32_t ml[CH];
#pragma unroll
    for (uint32_t j = 0; j < CH; ++j) { const uint32_t s = j * 64u + lane; ml[j] = s < n ? lens[s] : 0u; }
    const unsigned long long below = (1ull << lane) - 1ull;
    int left = 1;
    uint32_t offs = 0;
    bool over = false;
    maxLen = 0;
    if (lane == 0) cnt[0] = 0;
    for (uint32_t l = 1; l <= 15; ++l) {
        uint32_t run = offs;
#pragma unroll
        for (uint32_t j = 0; j < CH; ++j) {
            const bool mine = ml[j] == l;
            const unsigned long long mask = __ballot(mine);
            if (mine) sym[run + (uint32_t)__popcll(mask & below)] = (uint16_t)(j * 64u + lane);
            run += (uint32_t)__popcll(mask);
        }
        const uint32_t c = run - offs;
        if (lane == 0) cnt[l] = (uint16_t)c;
        left = (left << 1) - (int)c;
        if (left < 0) { over = true; left = 0; }      // (over stays; the loop goes on so that every cnt is written)
        if (c) maxLen = l;
        offs = run;
    }
    wave_order();
    if (over) return CODE_OVER;
    for (uint32_t k = lane; k < (1u << FB); k += 64u) fast[k] = (uint16_t)canon_decode(cnt, sym, k, FB);
    wave_order();
    return left > 0 ? CODE_INCOMPLETE : CODE_OK;
}

// ---- the output of one member: literals wait in the lanes ---------------------------------------------------
struct Out {
    uint8_t* dst;             // the row's slice
    uint32_t pos, pstart;     // bytes produced; [pstart, pos) wait in the lanes, position p in lane p % 64
    uint32_t limit;           // out_len: no store at or beyond it
    uint32_t pend;
};
__device__ __forceinline__ void out_flush(Out& o, uint32_t lane)
{
    const uint32_t p = o.pstart + ((lane - o.pstart) & 63u);
    if (p < o.pos) o.dst[p] = (uint8_t)o.pend;
    o.pstart = o.pos;
}

#define NEED(bits_, n_) do { if ((n_) > (bits_).left) return MC_INFLATE_R_INPUT; } while (0)

// one deflate stream: payload bytes[payAt, payAt + payLen) -> o.  Returns 0 or the reason.  Wave-uniform but for the copies.
__device__ uint32_t inflate_stream(const uint8_t* B, uint64_t payAt, uint32_t payLen, uint64_t memberEnd, Out& o, WaveTables& T, uint32_t lane)
{
    // the code-length code's order in a dynamic header
    constexpr uint64_t kOrderLo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t kOrderHi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
    Bits b;
    bits_start(b, B, payAt, memberEnd, payLen * 8u);
    for (;;) {                                              // a deflate block per round: each takes at least 3 bits
        NEED(b, 3u);
        const uint32_t head = bits_peek(b, 3u);
        bits_drop(b, 3u);
        const uint32_t last = head & 1u, type = head >> 1;
        if (type == 3u) return MC_INFLATE_R_BTYPE;
        if (type == 0u) {
            bits_drop(b, b.left & 7u);                     // (fewer than 8, and have >= 29 after the peek above)
            NEED(b, 32u);
            const uint32_t v = bits_peek(b, 32u);
            bits_drop(b, 32u);
            const uint32_t len = v & 0xFFFFu;
            if ((len ^ 0xFFFFu) != (v >> 16)) return MC_INFLATE_R_STORED;
            NEED(b, len * 8u);
            if (len > o.limit - o.pos) return MC_INFLATE_R_OVER;
            out_flush(o, lane);
            const uint64_t src = payAt + payLen - (b.left >> 3);
            for (uint32_t i = lane; i < len; i += 64u) o.dst[o.pos + i] = B[src + i];
            o.pos += len; o.pstart = o.pos;
            bits_start(b, B, src + len, memberEnd, b.left - len * 8u);
        } else {
            uint32_t nlit, ndist;
            if (type == 1u) {
                for (uint32_t s = lane; s < 288u; s += 64u) T.lens[s] = s < 144u ? 8 : s < 256u ? 9 : s < 280u ? 7 : 8;
                if (lane < 32u) T.lens[288u + lane] = 5;
                nlit = 288u; ndist = 32u;                  // (286, 287 and 30, 31 take part in the code and are refused where they are decoded)
                wave_order();
            } else {
                NEED(b, 14u);
                const uint32_t h = bits_peek(b, 14u);
                bits_drop(b, 14u);
                nlit = (h & 31u) + 257u; ndist = ((h >> 5) & 31u) + 1u;
                const uint32_t ncl = (h >> 10) + 4u;
                if (nlit > 286u || ndist > 30u) return MC_INFLATE_R_LENGTHS;
                if (lane < 19u) T.lens[lane] = 0;
                wave_order();
                for (uint32_t i = 0; i < ncl; ++i) {
                    NEED(b, 3u);
                    const uint32_t x = bits_peek(b, 3u);
                    bits_drop(b, 3u);
                    const uint32_t at = (uint32_t)((i < 12u ? kOrderLo >> (5u * i) : kOrderHi >> (5u * (i - 12u))) & 31u);
                    if (lane == 0) T.lens[at] = (uint8_t)x;
                }
                wave_order();
                uint32_t clMax;
                if (build_code<1, kClFast>(T.lens, 19u, T.distCnt, T.distSym, T.distFast, lane, clMax) != CODE_OK) return MC_INFLATE_R_LENGTHS;
                const uint32_t total = nlit + ndist;
                uint32_t idx = 0, prev = 0;
                while (idx < total) {                       // each round takes at least one bit
                    const uint32_t e = uni(T.distFast[bits_peek(b, kClFast)]);
                    if (!e) return MC_INFLATE_R_LENGTHS;
                    NEED(b, e & 15u);
                    bits_drop(b, e & 15u);
                    const uint32_t s = e >> 4;
                    if (s < 16u) {
                        if (lane == 0) T.lens[idx] = (uint8_t)s;
                        ++idx; prev = s;
                        continue;
                    }
                    if (s == 16u && idx == 0) return MC_INFLATE_R_LENGTHS;
                    const uint32_t xb = s == 16u ? 2u : s == 17u ? 3u : 7u;
                    NEED(b, xb);
                    const uint32_t rep = (s == 16u ? 3u : s == 17u ? 3u : 11u) + bits_peek(b, xb);
                    bits_drop(b, xb);
                    if (rep > total - idx) return MC_INFLATE_R_LENGTHS;
                    const uint32_t val = s == 16u ? prev : 0u;
                    for (uint32_t i = lane; i < rep; i += 64u) T.lens[idx + i] = (uint8_t)val;
                    idx += rep; prev = val;
                }
                wave_order();
                if (uni(T.lens[256]) == 0u) return MC_INFLATE_R_LENGTHS;
            }
            uint32_t litMax, distMax;
            int rc = build_code<5, kLitFast>(T.lens, nlit, T.litCnt, T.litSym, T.litFast, lane, litMax);
            if (rc == CODE_OVER || (rc == CODE_INCOMPLETE && litMax != 1u)) return MC_INFLATE_R_LENGTHS;
            rc = build_code<1, kDistFast>(T.lens + nlit, ndist, T.distCnt, T.distSym, T.distFast, lane, distMax);
            if (rc == CODE_OVER || (rc == CODE_INCOMPLETE && distMax > 1u)) return MC_INFLATE_R_LENGTHS;
            for (;;) {                                      // a symbol per round: each takes at least one bit
                uint32_t v = bits_peek(b, 15u);
                uint32_t e = uni(T.litFast[v & ((1u << kLitFast) - 1u)]);
                if (!e) e = uni(canon_decode(T.litCnt, T.litSym, v, 15u));
                if (!e) return b.left ? MC_INFLATE_R_SYMBOL : MC_INFLATE_R_INPUT;
                NEED(b, e & 15u);
                bits_drop(b, e & 15u);
                const uint32_t s = e >> 4;
                if (s < 256u) {
                    if (o.pos >= o.limit) return MC_INFLATE_R_OVER;
                    if (lane == (o.pos & 63u)) o.pend = s;
                    ++o.pos;
                    if (o.pos - o.pstart == 64u) out_flush(o, lane);
                    continue;
                }
                if (s == 256u) break;
                if (s >= 286u) return MC_INFLATE_R_SYMBOL;
                uint32_t len;
                if (s < 265u) len = s - 254u;
                else if (s == 285u) len = 258u;
                else {
                    const uint32_t xb = (s - 261u) >> 2;
                    NEED(b, xb);
                    len = ((4u + ((s - 265u) & 3u)) << xb) + 3u + bits_peek(b, xb);
                    bits_drop(b, xb);
                }
                v = bits_peek(b, 15u);
                e = uni(T.distFast[v & ((1u << kDistFast) - 1u)]);
                if (!e) e = uni(canon_decode(T.distCnt, T.distSym, v, 15u));
                if (!e) return b.left ? MC_INFLATE_R_DISTANCE : MC_INFLATE_R_INPUT;
                NEED(b, e & 15u);
                bits_drop(b, e & 15u);
                const uint32_t ds = e >> 4;
                if (ds >= 30u) return MC_INFLATE_R_DISTANCE;
                uint32_t dist;
                if (ds < 4u) dist = ds + 1u;
                else {
                    const uint32_t xb = (ds >> 1) - 1u;
                    NEED(b, xb);
                    dist = ((2u + (ds & 1u)) << xb) + 1u + bits_peek(b, xb);
                    bits_drop(b, xb);
                }
                if (dist > o.pos) return MC_INFLATE_R_DISTANCE;
                if (len > o.limit - o.pos) return MC_INFLATE_R_OVER;
                out_flush(o, lane);
                wave_order();                               // the source bytes are this wave's earlier stores
                uint8_t* to = o.dst + o.pos;
                const uint8_t* from = to - dist;
                if (dist >= len) { for (uint32_t i = lane; i < len; i += 64u) to[i] = from[i]; }
                else { for (uint32_t i = lane; i < len; i += 64u) to[i] = from[i % dist]; }
                o.pos += len; o.pstart = o.pos;
            }
        }
        if (last) break;
    }
    out_flush(o, lane);
    bits_drop(b, b.left & 7u);
    return b.left ? MC_INFLATE_R_LEFT : 0u;
}

// ---- CRC-32 (reflected, polynomial kCrcPoly): a(x) * b(x) mod P, x^0 = bit 31 -----------------------------------------
__device__ __forceinline__ uint32_t crc_mul(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (uint32_t i = 0; i < 32u; ++i) {
        if (a & (0x80000000u >> i)) p ^= b;
        b = (b & 1u) ? (b >> 1) ^ kCrcPoly : b >> 1;
    }
    return p;
}
__device__ __forceinline__ uint32_t crc_pow(uint32_t a, uint32_t n)   // a^n
{
    uint32_t r = 0x80000000u;
    for (; n; n >>= 1) { if (n & 1u) r = crc_mul(r, a); a = crc_mul(a, a); }
    return r;
}
// the CRC-32 of dst[0, n), by the wave; all lanes get it
__device__ __forceinline__ uint32_t wave_crc32(const uint8_t* dst, uint32_t n, const uint32_t* tab, uint32_t lane)
{
    if (n == 0) return 0u;
    const uint32_t L = (n + 63u) / 64u, pad = 64u * L - n;          // the data with `pad` zeros in front: 64 chunks of L
    const int64_t a0 = (int64_t)lane * L - pad, b0 = a0 + L;
    uint32_t reg = 0;                                                // (a zero register stays zero over the padding)
    if (b0 > 0) {
        if (a0 <= 0) reg = 0xFFFFFFFFu;                              // the chunk that holds byte 0
        for (uint32_t p = (uint32_t)max(a0, (int64_t)0); p < (uint32_t)b0; ++p) reg = tab[(reg ^ dst[p]) & 255u] ^ (reg >> 8);
    }
    // lane i's register is followed by (63 - i) * L bytes
    const uint32_t op = crc_pow(0x00800000u /* x^8 */, L);
    uint32_t x = crc_mul(crc_pow(op, 63u - lane), reg);
    for (int m = 1; m < 64; m <<= 1) x ^= (uint32_t)__shfl_xor((int)x, m);
    return ~x;
}

__device__ __forceinline__ uint32_t load_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

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

struct InflateState {                    // what the context keeps for mc_inflate_*
    unsigned long long* dCounters = nullptr;   // bytes out of accepted calls, calls refused
    std::atomic<uint64_t> calls{0}, bytesIn{0};
    std::mutex stageMtx;                 // MC_INFLATE_HOST callers take turns at the staging buffers
    DevBuf stageIn, stageRows, stageOut;
    StatusStage status;                  // [4]
};

void free_inflate_state(mc_ctx* ctx)
{
    if (!ctx->inflate) return;
    InflateState& S = *ctx->inflate;
    if (S.dCounters) (void)hipFree(S.dCounters);
    free_status_stage(S.status);
    for (DevBuf* b : {&S.stageIn, &S.stageRows, &S.stageOut})
        if (b->p) (void)hipFree(b->p);
    delete ctx->inflate;
    ctx->inflate = nullptr;
}

}  // namespace mcamd

namespace {

int ensure_inflate_state(mc_ctx* ctx, InflateState** out)
{
    std::lock_guard<std::mutex> lock(ctx->inflateMtx);
    if (!ctx->inflate) ctx->inflate = new InflateState;
    InflateState& S = *ctx->inflate;
    *out = &S;
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, kCounterPairBytes));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, kCounterPairBytes));
    }
    return make_status_stage(ctx, S.status, 4);
}

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
