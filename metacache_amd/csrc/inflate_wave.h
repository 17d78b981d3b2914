// metacache_amd/csrc/inflate_wave.h -- the wave-level deflate decoder that inflate.hip (BGZF members) and inflate_streams.hip
// (whole gzip files, 7n) share: the bit reader (Bits), the canonical tables of a code set (build_code, canon_decode), the output of one
// member with its waiting literals (Out), the decode of one deflate stream (inflate_deflate; inflate_stream adds 7j's "ends exactly at the
// trailer"), the CRC-32 of a slice by the wave (wave_crc32) and the ordering fence (wave_order).  What the header comment of inflate.hip
// says about them holds here: everything the chain decides is wave-uniform, the tables live in LDS per wave, nothing per lane is indexed
// at run time, and every loop is bounded by what is left of the input bits or of the output slice.
// Behind the device part: the state both calls keep in the context (InflateState), so that their host forms share the staging buffers and
// their mutex.  Internal; plain HIP C++, no inline assembly.
#pragma once

#include "rows_common.h"

#include <atomic>
#include <mutex>

#ifdef __HIPCC__

namespace {

constexpr uint32_t kLitFast = 10, kDistFast = 8, kClFast = 7;      // bits of the fast tables (a code-length code has at most 7 bits: its table is complete)
constexpr uint32_t kCrcPoly = 0xEDB88320u;

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

// one deflate stream: bytes[payAt, payAt + payLen) bound its input -> o.  Returns 0 or the reason; with 0, b stands behind the final block's
// last bit, so that payLen * 8 - b.left bits were the stream's.  Matches reach back to o.dst and no further: a caller with several
// members in one slice gives each member an Out of its own.  Wave-uniform but for the copies.
__device__ __forceinline__ uint32_t inflate_deflate(const uint8_t* B, uint64_t payAt, uint32_t payLen, uint64_t memberEnd, Out& o, WaveTables& T, uint32_t lane, Bits& b)
{
    // the code-length code's order in a dynamic header
    constexpr uint64_t kOrderLo = 16ull | 17ull << 5 | 18ull << 10 | 0ull << 15 | 8ull << 20 | 7ull << 25 | 9ull << 30 | 6ull << 35 | 10ull << 40 | 5ull << 45 | 11ull << 50 | 4ull << 55;
    constexpr uint64_t kOrderHi = 12ull | 3ull << 5 | 13ull << 10 | 2ull << 15 | 14ull << 20 | 1ull << 25 | 15ull << 30;
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
    return 0u;
}

// 7j's block rule: the payload is exactly one deflate stream, which ends, after the bits up to the next byte, at the trailer
__device__ uint32_t inflate_stream(const uint8_t* B, uint64_t payAt, uint32_t payLen, uint64_t memberEnd, Out& o, WaveTables& T, uint32_t lane)
{
    Bits b;
    const uint32_t code = inflate_deflate(B, payAt, payLen, memberEnd, o, T, lane, b);
    if (code) return code;
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

}  // namespace

#endif  // __HIPCC__

namespace mcamd {

struct InflateState {                    // what the context keeps for mc_inflate_*
    unsigned long long* dCounters = nullptr;   // bytes out of accepted calls, calls refused; then mc_inflate_streams': bytes out of accepted rows, rows refused
    std::atomic<uint64_t> calls{0}, bytesIn{0};
    std::atomic<uint64_t> streamCalls{0}, streamBytesIn{0}, streamRefusedHost{0};   // (rows the host form refuses without the device)
    std::mutex stageMtx;                 // MC_INFLATE_HOST callers take turns at the staging buffers
    DevBuf stageIn, stageRows, stageOut;
    DevBuf stageResults;                 // mc_inflate_streams: the piece's mc_gzip_result rows
    StatusStage status;                  // [4]
};
constexpr size_t kInflateCounterBytes = 4 * sizeof(unsigned long long);

// the context's state, made on first use
inline int ensure_inflate_state(mc_ctx* ctx, InflateState** out)
{
    std::lock_guard<std::mutex> lock(ctx->inflateMtx);
    if (!ctx->inflate) ctx->inflate = new InflateState;
    InflateState& S = *ctx->inflate;
    *out = &S;
    if (!S.dCounters) {
        HIP_TRY(ctx, hipMalloc((void**)&S.dCounters, kInflateCounterBytes));
        HIP_TRY(ctx, hipMemset(S.dCounters, 0, kInflateCounterBytes));
    }
    return make_status_stage(ctx, S.status, 4);
}

}  // namespace mcamd
