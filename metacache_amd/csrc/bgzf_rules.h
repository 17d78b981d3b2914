// metacache_amd/csrc/bgzf_rules.h -- the BGZF member rule of include/metacache_amd.h as plain host functions: the walk behind
// mc_bgzf_index and the row checks of mc_inflate_blocks(MC_INFLATE_HOST).  They read untrusted bytes, so every access is checked against
// nbytes before it is made.  No context, no device, no zlib; a stand-alone program can include this file alone (tools/bgzf_rules_check.cpp).
#pragma once

#include "../../include/metacache_amd.h"

namespace mcamd {

inline uint32_t bgzf_u16(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
inline uint32_t bgzf_u32(const uint8_t* p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }

// the member at offset p of bytes[0, nbytes): its size and ISIZE, or false
inline bool bgzf_member(const uint8_t* bytes, uint64_t nbytes, uint64_t p, uint32_t& size, uint32_t& isize)
{
    if (nbytes - p < 12) return false;
    const uint8_t* h = bytes + p;
    if (h[0] != 0x1f || h[1] != 0x8b || h[2] != 8 || h[3] != 4) return false;
    const uint32_t xlen = bgzf_u16(h + 10);
    if (nbytes - p - 12 < xlen) return false;
    // the subfields tile the extra field exactly; exactly one of them is BC with two bytes
    uint32_t at = 0, found = 0, bsize = 0;
    while (at < xlen) {
        if (xlen - at < 4) return false;
        const uint8_t* f = h + 12 + at;
        const uint32_t slen = bgzf_u16(f + 2);
        if (xlen - at - 4 < slen) return false;
        if (f[0] == 'B' && f[1] == 'C') {
            if (slen != 2 || found) return false;
            found = 1;
            bsize = bgzf_u16(f + 4);
        }
        at += 4 + slen;
    }
    if (!found) return false;
    size = bsize + 1;
    if (size < 12 + xlen + 8 || nbytes - p < size) return false;
    isize = bgzf_u32(h + size - 4);
    return isize <= 65536;
}

// mc_bgzf_index without its argument checks
inline void bgzf_index(const uint8_t* bytes, uint64_t nbytes, mc_bgzf_block* blocks, uint64_t capacity, uint64_t info[4])
{
    uint64_t p = 0, members = 0, outBytes = 0;
    info[2] = MC_BGZF_OK; info[3] = 0;
    if (nbytes == 0) { info[2] = MC_BGZF_FOREIGN; }       // (no member chains from 0 to 0: an empty file is not a BGZF file)
    while (p < nbytes) {
        uint32_t size = 0, isize = 0;
        if (!bgzf_member(bytes, nbytes, p, size, isize)) { info[2] = MC_BGZF_FOREIGN; info[3] = p; break; }
        if (blocks && members < capacity) {
            mc_bgzf_block& b = blocks[members];
            b.in_off = p; b.out_off = outBytes; b.in_len = size; b.out_len = isize;
        }
        ++members; outBytes += isize; p += size;
    }
    info[0] = members; info[1] = outBytes;
}

// the rows of a host call: non-decreasing and non-overlapping on both sides, inside nbytes, no slice beyond 64 KiB
inline bool bgzf_rows_ok(const mc_bgzf_block* blocks, uint64_t numBlocks, uint64_t nbytes)
{
    uint64_t inEnd = 0, outEnd = 0;
    for (uint64_t i = 0; i < numBlocks; ++i) {
        const mc_bgzf_block& b = blocks[i];
        if (b.out_len > 65536) return false;
        if (b.in_off < inEnd || b.in_off > nbytes || nbytes - b.in_off < b.in_len) return false;
        if (b.out_off < outEnd || b.out_off + b.out_len < b.out_off) return false;
        inEnd = b.in_off + b.in_len; outEnd = b.out_off + b.out_len;
    }
    return true;
}

}  // namespace mcamd
