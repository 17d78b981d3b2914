// metacache_amd/csrc/gzip_rules.h -- the gzip member header of the stream rule of include/metacache_amd.h as plain host
// functions: the walk behind mc_gzip_hint and the row checks of mc_inflate_streams(MC_INFLATE_HOST).  They read untrusted bytes, so every
// access is checked against the end of the range before it is made.  No context, no device, no zlib; a stand-alone program can include
// this file alone (tools/gzip_rules_check.cpp).  The kernel's header walk (inflate_streams.hip) makes the same checks in the same order.
#pragma once

#include "../../include/metacache_amd.h"

#include <algorithm>
#include <vector>

namespace mcamd {

// The limits of a row.  The decoder counts a member's unread input in BITS and its output in bytes, both in 32-bit registers:
// in_len <= 2^28 keeps 8 * in_len <= 2^31, out_cap <= 2^31 keeps every position and every "limit - pos" below 2^32.
constexpr uint64_t kGzipMinRow = 18;              // a 10-byte header and an 8-byte trailer (the stream between them needs 2 bytes more: the decoder says so)
constexpr uint64_t kGzipMaxRowIn = 1ull << 28;
constexpr uint64_t kGzipMaxRowOut = 1ull << 31;

inline uint32_t gzip_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the header of the member at offset p < end of bytes[0, end): 0 and the offset of its deflate stream in `pay`, or the reason.  `first`:
// the row's first member (bytes that are no magic are a bad header there, and trailing bytes behind a trailer)
inline uint32_t gzip_header(const uint8_t* bytes, uint64_t end, uint64_t p, bool first, uint64_t& pay)
{
    if (end - p < 2 || bytes[p] != 0x1f || bytes[p + 1] != 0x8b) return first ? MC_INFLATE_R_HEADER : MC_INFLATE_R_TRAILING;
    if (end - p < 10) return MC_INFLATE_R_HEADER;
    if (bytes[p + 2] != 8) return MC_INFLATE_R_HEADER;
    const uint32_t flg = bytes[p + 3];
    if (flg & 0xE2u) return MC_INFLATE_R_HEADER;                  // FHCRC (2) or a reserved bit (32, 64, 128); FTEXT (1) is ignored
    uint64_t at = p + 10;
    if (flg & 4u) {                                               // FEXTRA: XLEN and its bytes
        if (end - at < 2) return MC_INFLATE_R_HEADER;
        const uint64_t xlen = (uint64_t)bytes[at] | ((uint64_t)bytes[at + 1] << 8);
        if (end - at - 2 < xlen) return MC_INFLATE_R_HEADER;
        at += 2 + xlen;
    }
    for (uint32_t bit = 8u; bit <= 16u; bit <<= 1)                // FNAME, then FCOMMENT: up to and with a zero byte
        if (flg & bit) {
            while (at < end && bytes[at] != 0) ++at;              // (a byte per round, at most end - at rounds)
            if (at == end) return MC_INFLATE_R_HEADER;
            ++at;
        }
    pay = at;
    return 0;
}

// mc_gzip_hint without its argument checks
inline void gzip_hint(const uint8_t* bytes, uint64_t nbytes, uint64_t info[4])
{
    info[0] = MC_GZIP_FOREIGN; info[1] = 0; info[3] = 0;
    info[2] = nbytes >= 4 ? gzip_u32(bytes + nbytes - 4) : 0;
    if (nbytes < kGzipMinRow) { info[3] = MC_INFLATE_R_INPUT; return; }
    uint64_t pay = 0;
    uint32_t reason = gzip_header(bytes, nbytes, 0, true, pay);
    if (!reason && nbytes - pay < 8) reason = MC_INFLATE_R_INPUT;         // no room for the trailer behind the header
    if (reason) { info[3] = reason; return; }
    info[0] = MC_GZIP_OK; info[1] = pay;
}

// the rows of a host call: every row within the limits and inside nbytes, the out slices free of overflow and pairwise disjoint (empty
// slices overlap nothing).  false: the call is refused before any device call
inline bool gzip_rows_ok(const mc_gzip_stream* rows, uint64_t numRows, uint64_t nbytes)
{
    std::vector<std::pair<uint64_t, uint64_t>> slices;
    slices.reserve(numRows);
    for (uint64_t i = 0; i < numRows; ++i) {
        const mc_gzip_stream& r = rows[i];
        if (r.in_len < kGzipMinRow || r.in_len > kGzipMaxRowIn || r.out_cap > kGzipMaxRowOut) return false;
        if (r.in_off > nbytes || nbytes - r.in_off < r.in_len) return false;
        if (r.out_off + r.out_cap < r.out_off) return false;
        if (r.out_cap) slices.emplace_back(r.out_off, r.out_off + r.out_cap);
    }
    std::sort(slices.begin(), slices.end());
    for (size_t i = 1; i < slices.size(); ++i)
        if (slices[i].first < slices[i - 1].second) return false;
    return true;
}

}  // namespace mcamd
