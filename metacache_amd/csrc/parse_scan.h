// metacache_amd/csrc/parse_scan.h -- what the byte passes (parse.hip, parse_cut.hip, taxmap.hip, merge_results.hip) share: the tile, a
// thread's 16 bytes of it (Chunk), the byte classes and the line rule's line starts.  The block scans that turn a thread's values into
// what lies in front of the thread are block_scan.h's.  Device code; internal.
#pragma once

#include "rows_common.h"
#include "block_scan.h"

namespace mcamd {
namespace parsek {

constexpr uint32_t kTile = kBlock * 16, kNone = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint32_t tiles_of(uint64_t nbytes) { return (uint32_t)((nbytes + kTile - 1) / kTile); }

// ---- a thread's 16 bytes of A, the aligned address at or below the range (A = bytes - shift, shift < 16): bytes k in [lo, hi) are
// positions g + k - shift of the range; position p of the range is A[p + shift] ------------------------------------------------------------
struct Chunk { uint32_t w[4]; uint32_t g, lo, hi, prev, next; };  // prev / next: the byte in front of position g + lo - shift, the one behind g + 15 - shift ('\n' outside the range)

__device__ __forceinline__ Chunk load_chunk(const uint8_t* A, uint32_t n, uint32_t shift, uint32_t g)
{
    Chunk c;
    const uint32_t end = n + shift;                                              // (n <= 2^31, shift < 16)
    c.g = g;
    c.lo = g < shift ? shift - g : 0u;
    c.hi = g < end ? min(16u, end - g) : 0u;
    c.w[0] = c.w[1] = c.w[2] = c.w[3] = 0;
    c.prev = c.next = (uint32_t)'\n';
    if (c.lo >= c.hi) { c.lo = c.hi = 0; return c; }
    const uint4 v = *reinterpret_cast<const uint4*>(A + g);                      // (an aligned 16 bytes that hold a byte of the range: inside its pages)
    c.w[0] = v.x; c.w[1] = v.y; c.w[2] = v.z; c.w[3] = v.w;
    if (g + c.lo > shift) c.prev = A[g + c.lo - 1];
    if (c.hi == 16 && g + 16u < end) c.next = A[g + 16u];
    return c;
}
#define CHUNK_BYTE(c, k) (((c).w[(k) >> 2] >> (((k) & 3u) * 8u)) & 0xFFu)

// ---- the byte classes of the line rules; B: a range of n bytes at a 16-byte aligned address, '\n' behind its end -------------------------
__device__ __forceinline__ uint32_t byte_at(const uint8_t* B, uint32_t n, uint32_t p) { return p < n ? (uint32_t)B[p] : (uint32_t)'\n'; }
__device__ __forceinline__ bool is_digit(uint32_t c) { return c - '0' < 10u; }
__device__ __forceinline__ bool is_blank(uint32_t c) { return c == ' ' || c == '\t'; }
__device__ __forceinline__ bool is_refused(uint32_t c) { return c == '\r' || c == '\v' || c == '\f' || c == 0; }   // (a NUL ends the host's C string)

// bit k: byte p0 + k of the range is a line start (position 0 or the byte behind a '\n'); p0: a multiple of 16
__device__ __forceinline__ uint32_t line_starts(const uint8_t* B, uint32_t n, uint32_t p0)
{
    const Chunk c = load_chunk(B, n, 0, p0);
    uint32_t prev = c.prev, mask = 0;
#pragma unroll
    for (uint32_t k = 0; k < 16; ++k) {
        if (k < c.lo || k >= c.hi) continue;
        if (prev == '\n') mask |= 1u << k;
        prev = CHUNK_BYTE(c, k);
    }
    return mask;
}

// fn(s) for every line start s among the 16 bytes from p0 on, ascending
template <class Fn>
__device__ __forceinline__ void for_each_line_start(const uint8_t* B, uint32_t n, uint32_t p0, Fn&& fn)
{
    for (uint32_t m = line_starts(B, n, p0); m; m &= m - 1) fn(p0 + (uint32_t)__ffs((int)m) - 1u);
}

}  // namespace parsek
}  // namespace mcamd
