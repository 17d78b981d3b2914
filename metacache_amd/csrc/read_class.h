// metacache_amd/csrc/read_class.h -- the hand-over of the query path: which kernel finishes a read the lane kernels cannot (its CLASS),
// the work-list record that names it, and the limits of the kernels that take the lists.  No HIP header: a plain host compiler can
// include it (tests/cpp/read_class_check.cpp).  Who writes and reads which list: the table in kernels.h.
#pragma once

#include <cstdint>

#if !defined(MC_HD) && defined(__HIPCC__)
#define MC_HD __host__ __device__
#elif !defined(MC_HD)
#define MC_HD
#endif

namespace mcamd {

constexpr uint32_t kMaxHitsPerQuery = (1u << 20) - 1;  // packed candidate fields are 20 bits wide
constexpr uint32_t kLdsCap = 256;         // location lists up to this length are sorted in LDS
constexpr uint32_t kMid64 = 64, kMid128 = 128;   // mid_cands_kernel: lists up to 64 are sorted in the registers of 4 lanes, up to 128 of 8 ...
constexpr uint32_t kMidMax = 256;         // ... and this is the longest list it takes (16 lanes)
constexpr uint32_t kHashMax = 1024, kHashEnt = 256, kHashWin = 8;   // hash_cands_kernel: longest list, entries, maxWindowsInRange
constexpr uint32_t kBigEnt = 64;          // big_filter_kernel: found features per query, one lane each ...
constexpr uint32_t kBigEPL = 3;           // ... or up to three per lane in its second instance (reads and pairs of 5 .. 10 windows: 2 x 250 bp, 500 bp)
constexpr uint32_t kGwSmallH = 2048;      // compact store: reads with more locations take gw_filter_kernel's instance with the larger filters
static_assert(kMidMax <= kLdsCap, "segment_hits: no list of mid_cands_kernel needs a segment in HBM");

// counter slots of ws.midCount and the lists of ws.midList (table: kernels.h)
constexpr uint32_t kCntMid64 = 0, kCntMid128 = 1, kCntMid256 = 2, kCntHash512 = 3, kCntHash1024 = 4, kCntChunks = 5, kCntWaveSketch = 6,
                   kCntWaveCands = 7, kCntHash256 = 8, kCntFilter = 9, kCntSecond = 10, kCntStream = 12, kCntSorted = 13, kCnt512 = 14,
                   kCnt1024 = 15, kCntOverflow = 16, kCntSortedBig = 18;
enum WorkList : uint32_t { kListMid64, kListMid128, kListMid256, kListHash512, kListHash1024, kListHash256, kListFilter, kListFiltered, kWorkLists };
constexpr uint32_t kClassWave = 6, kClassFilter = 7;
MC_HD constexpr uint32_t class_counter(uint32_t c) { return c < 5 ? c : c == 5 ? kCntHash256 : kCntFilter; }
MC_HD constexpr uint32_t class_list(uint32_t c) { return c == kClassFilter ? kListFilter : c; }

// ---- the work-list record {query, first entry slot, entries | locations << kRecEntBits, maxWindowsInRange} (midList words x, y, z, w) ----
constexpr uint32_t kRecEntBits = 12, kRecEntMax = (1u << kRecEntBits) - 1;
static_assert(kMaxHitsPerQuery <= (0xFFFFFFFFu >> kRecEntBits), "a read's locations fit the record's bits above the entries");
struct WorkRecord { uint32_t query, first, packed, maxWin; };
MC_HD constexpr WorkRecord work_record(uint32_t q, uint32_t first, uint32_t entries, uint32_t H, uint32_t maxWin)
{
    return WorkRecord{q, first, entries | (H << kRecEntBits), maxWin};
}
MC_HD constexpr uint32_t rec_entries(uint32_t z) { return z & kRecEntMax; }
MC_HD constexpr uint32_t rec_hits(uint32_t z) { return z >> kRecEntBits; }

// ---- the rule ----
// bigMin: Workspace::bigMin; gwGap: DeviceTable::gwGap; compact: the table has the compact location store (DeviceTable::values32)
struct ClassLimits { uint32_t bigMin, gwGap; bool compact; };

// kClassFilter = the filtered path (filter first): lists beyond bigMin locations -- and beyond kMid64, which are sorted in registers --
// 8-byte store: from at most kBigEnt * kBigEPL found features, window ranges the counting kernel takes (H has no upper bound of its own
//   here: it is the load-time limit of the lists' lengths that keeps kBigEnt * kBigEPL lists inside the record's bits);
// compact store: any number of entries the record can name, any window range the gap between two targets covers; filtered lists the
//   counting kernels do not take are sorted (gw_sorted_cands_kernel).
MC_HD constexpr bool filter_takes(uint32_t H, uint32_t entries, uint32_t maxWin, ClassLimits l)
{
    return H > l.bigMin && H > kMid64 &&
           (l.compact ? (entries <= kRecEntMax && maxWin <= l.gwGap && H <= kMaxHitsPerQuery) : (entries <= kBigEnt * kBigEPL && maxWin <= kHashWin));
}
// The class of a read with H locations from `entries` hand-over entries.  Up to kMid64 locations the register sort wins (1.6 vs 2 ns
// per list); beyond, counting (hash_cands_kernel) where it can take the read, else the sort (measured per list: 3.3 vs 4.7 ns at
// 129 .. 256).  Longer lists and wide window ranges that the filtered path does not take are the wave kernels'.
MC_HD constexpr uint32_t read_class(uint32_t H, uint32_t entries, uint32_t maxWin, ClassLimits l)
{
    const bool hashOK = entries <= kHashEnt && maxWin <= kHashWin;
    return filter_takes(H, entries, maxWin, l) ? kClassFilter
         : H <= kMid64 ? kListMid64
         : H <= kMid128 ? (hashOK ? kListHash256 : kListMid128)
         : H <= kMidMax ? (hashOK ? kListHash256 : kListMid256)
         : (H <= kHashMax && hashOK) ? (H <= kHashMax / 2 ? kListHash512 : kListHash1024)
         : kClassWave;
}
// kCntSecond: is a read of kClassFilter one of those the filter's second instance runs for
MC_HD constexpr bool filter_second(uint32_t H, uint32_t entries, bool compact) { return compact ? H > kGwSmallH : entries > kBigEnt; }
// Workspace::hitScan: the locations that need a segment in HBM -- only the wave kernels' lists beyond what they sort in LDS
// (a read beyond kMaxHitsPerQuery has no segment at all)
MC_HD constexpr uint32_t segment_hits(uint32_t H, uint32_t cls) { return cls == kClassWave && H > kLdsCap && H <= kMaxHitsPerQuery ? H : 0u; }

}  // namespace mcamd
