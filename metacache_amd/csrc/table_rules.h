// metacache_amd/csrc/table_rules.h -- the query table's layout, its load-time rules (host and device) and the load steps that run on the
// host over a batch of the database file.  No HIP header, no mc_ctx: a plain host compiler can include it (tests/cpp/table_rules_check.cpp).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

#ifdef __HIPCC__
#define MC_HD __host__ __device__
#else
#define MC_HD
#endif

namespace mcamd {

// Table layout: an array of 64-byte BUCKETS of 4 slots, two per 128-byte line, structure-of-arrays so
// that a single LANE looks a feature up with four 16-byte loads of ONE half line and has key, size and
// payload of the match in registers -- no second, dependent access (a separate payload load re-fetched
// the line from L2 because thousands of lines are in flight per CU and the L1 holds 256):
//   key[4]     the features
//   size[4]    bucket sizes (u16), 0 = free slot
//   payload[4] size == 1: the location itself ((tgt << 32) | win);
//              size  > 1: index of the first location in DeviceTable::values
// Probe sequence of a key: its home bucket, the sibling bucket in the same line, then the following
// buckets linearly.  Insertion uses the first bucket of that sequence with a free slot, so a lookup
// ends at the first bucket that holds the key or has a free slot.
struct __attribute__((aligned(64))) TableBucket {
    uint32_t key[4];
    uint16_t size[4];
    uint32_t spare[2];
    uint64_t payload[4];
};
static_assert(sizeof(TableBucket) == 64, "two buckets per 128-byte line");
constexpr uint32_t kSlotsPerBucket = 4;

MC_HD inline uint32_t next_bucket(uint32_t home, uint32_t cur, uint32_t step, uint32_t nbuckets)
{
    // step = number of buckets already visited (>= 1)
    if (step == 1) return home ^ 1u;                          // sibling half of the same line
    const uint32_t nx = (step == 2 ? (home | 1u) : cur) + 1u;
    return nx >= nbuckets ? 0u : nx;
}

// table hash: features are the SMALLEST hash values of a window, i.e. far from uniform in their
// high bits, so they are mixed again (murmur3 fmix32) before the multiply-shift range reduction
// bucket = (mix32(key) * nbuckets) >> 32.
MC_HD inline uint32_t mix32(uint32_t x)
{
    x ^= x >> 16; x *= 0x85ebca6bu; x ^= x >> 13; x *= 0xc2b2ae35u; x ^= x >> 16;
    return x;
}

// Mode K: which key shard owns a feature (a different mix than the bucket hash, so a shard's keys spread over its whole table)
MC_HD inline uint32_t key_owner(uint32_t key, uint32_t shards)
{
    return shards <= 1 ? 0u : (uint32_t)(((uint64_t)mix32(key ^ 0x9E3779B9u) * shards) >> 32);
}

// table_build.hip: GPU-side table construction from the file's batch stream
struct LoadFilter { uint32_t maxLocs, rmOver, shardIdx, shardCnt, align = 1; };   // load-time modifiers + key shard + list alignment (below)
// LIST ALIGNMENT (round 5, compact store): a list of the location store may begin at a multiple of kListAlign numbers = 128 bytes.  The
// memory system serves random reads line by line (47 x 10^9 requests of 128 bytes per second, whatever part of the line is wanted:
// profiles/r05_fetch_calibration.md): a list of 196 bytes at an arbitrary 4-byte offset touches 2.6 lines, an aligned one 2.0 -- the
// filter kernels of read pairs and long reads run at that request rate.  Space a list takes in the store: list_alloc(size, align).
constexpr uint32_t kListAlign = 32;
MC_HD inline uint32_t list_alloc(uint32_t size, uint32_t align) { return size > 1 ? (size + align - 1) / align * align : 0; }

// THE load-time size rule: what a key that the file lists with `fileSize` locations keeps.  The two rules that look at the size alone:
MC_HD inline uint32_t size_after_rules(uint32_t fileSize, uint32_t rmOver, uint32_t maxLocs)
{
    uint32_t size = fileSize;
    if (rmOver && size > rmOver) size = 0;           // bucket emptied, key kept without values = never matches (host_hashmap.hpp:480-495)
    if (maxLocs && size > maxLocs) size = maxLocs;   // keep the FIRST n values (:454-466)
    return size;
}
MC_HD inline uint32_t effective_size(uint32_t key, uint32_t fileSize, const LoadFilter& lf)
{
    uint32_t size = size_after_rules(fileSize, lf.rmOver, lf.maxLocs);
    if (lf.shardCnt > 1 && key_owner(key, lf.shardCnt) != lf.shardIdx) size = 0;   // Mode K: another GPU's key
    return size;
}

// ---- host only: one batch of the file (keys u32 | sizes u8 | packed values {window u32, target u16|u32}) -----------------------------
enum class MergeStatus { Ok, TableFull, BucketTooLarge, TargetTooLarge };
struct MergeCounters { uint64_t keysStored = 0, locations = 0; uint32_t maxProbe = 1; };   // keys in the table, locations this part added, longest probe sequence

// One batch of part `part` into the host table of a multi-part database.  All parts share ONE table: a feature that occurs in several
// parts gets the concatenation of its per-part buckets, with the part number folded into the target id ((part << 24) | target), so
// that sorting by the stored key yields "per-part sorted lists concatenated in part order" -- the intended result of
// host_hashmap.hpp:695-723 -- with a single lookup per feature.  A bucket of one location keeps it in its payload, longer ones are runs
// of `store` (a merged bucket's run is written anew at the end; the old one stays behind unused).
inline MergeStatus merge_part_batch(std::vector<TableBucket>& buckets, std::vector<uint64_t>& store, uint32_t part, const uint32_t* keys,
                                    const uint8_t* sizes, const uint8_t* values, uint64_t n, uint32_t targetBytes, uint32_t rmOver,
                                    uint32_t maxLocs, MergeCounters& c)
{
    const uint32_t nbuckets = (uint32_t)buckets.size();
    const size_t vb = 4 + targetBytes;
    bool badTarget = false;
    auto decode = [&](const uint8_t* p) -> uint64_t {
        uint32_t win; std::memcpy(&win, p, 4);
        uint32_t tgt = 0;
        if (targetBytes == 2) { uint16_t t; std::memcpy(&t, p + 4, 2); tgt = t; } else std::memcpy(&tgt, p + 4, 4);
        badTarget = badTarget || tgt >= (1u << 24);
        return ((uint64_t)(tgt | part << 24) << 32) | win;
    };
    for (uint64_t i = 0; i < n; values += sizes[i] * vb, ++i) {
        const uint32_t size = size_after_rules(sizes[i], rmOver, maxLocs);
        if (size == 0) continue;
        // walk the key's probe sequence: an earlier part may already hold the key; otherwise it goes into the first bucket with a free slot
        const uint32_t key = keys[i], home = (uint32_t)(((uint64_t)mix32(key) * nbuckets) >> 32);
        uint32_t cur = home, probe = 1, slot = kSlotsPerBucket;
        TableBucket* grp = nullptr;
        bool found = false;
        for (;; ++probe) {
            grp = &buckets[cur];
            for (uint32_t j = 0; j < kSlotsPerBucket && !found; ++j) {
                if (!grp->size[j]) { if (slot == kSlotsPerBucket) slot = j; }
                else if (grp->key[j] == key) { slot = j; found = true; }
            }
            if (slot < kSlotsPerBucket) break;
            if (probe > nbuckets) return MergeStatus::TableFull;
            cur = next_bucket(home, cur, probe, nbuckets);
        }
        if (probe > c.maxProbe) c.maxProbe = probe;
        // new bucket = the locations of earlier parts (if any) followed by this part's; two and more are a run at the store's end
        const uint32_t s0 = found ? grp->size[slot] : 0;
        if (s0 + size > 0xFFFFu) return MergeStatus::BucketTooLarge;
        const uint64_t p0 = grp->payload[slot], off = store.size();
        if (s0 == 1) store.push_back(p0);                       // (an inline payload is re-homed)
        else for (uint32_t t = 0; t < s0; ++t) { const uint64_t v = store[p0 + t]; store.push_back(v); }
        for (uint32_t t = 0; t < size && s0 + size > 1; ++t) store.push_back(decode(values + t * vb));
        grp->key[slot] = key;
        grp->size[slot] = (uint16_t)(s0 + size);
        grp->payload[slot] = s0 + size > 1 ? off : decode(values);
        c.keysStored += !found;
        c.locations += size;
    }
    return badTarget ? MergeStatus::TargetTooLarge : MergeStatus::Ok;
}

// Mode T (mc_config.target_shard_*): the values of a batch that lie in the target range [lo, hi) move to the front of the batch's value
// array, bucket after bucket; a bucket is first cut as the whole table would cut it (size_after_rules), so that the device's own size
// rules find nothing more to do.  A bucket none of whose locations are in range keeps its key with size 0 (the table build skips it).
// Returns the number of values that stay (sizes[] updated).
inline uint64_t cut_batch_values(uint8_t* sizes, uint8_t* vals, uint32_t nkeys, uint32_t targetBytes, uint32_t lo, uint32_t hi,
                                 uint32_t rmOver, uint32_t maxLocs)
{
    const size_t vb = 4 + targetBytes;
    const uint8_t* src = vals;
    uint8_t* dst = vals;
    uint64_t kept = 0;
    for (uint32_t i = 0; i < nkeys; ++i) {
        const uint32_t fileSize = sizes[i], eff = size_after_rules(fileSize, rmOver, maxLocs);
        uint32_t n = 0;
        for (uint32_t j = 0; j < eff; ++j) {
            const uint8_t* v = src + (size_t)j * vb;
            uint32_t tgt = (uint32_t)v[4] | ((uint32_t)v[5] << 8);
            if (targetBytes == 4) tgt |= ((uint32_t)v[6] << 16) | ((uint32_t)v[7] << 24);
            if (tgt >= lo && tgt < hi) {
                if (dst != v) std::memmove(dst, v, vb);
                dst += vb; ++n;
            }
        }
        src += (size_t)fileSize * vb;
        sizes[i] = (uint8_t)n;
        kept += n;
    }
    return kept;
}

}  // namespace mcamd
