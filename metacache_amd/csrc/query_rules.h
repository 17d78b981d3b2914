// metacache_amd/csrc/query_rules.h -- the host's plan of ONE batch (query_pipe.cpp): what the caller's flags ask for, whether the lane path
// takes the batch, in which order the lane stage's kernels run, whether the host looks at the work lists' counters, what follows from
// them (wave kernel first, filtered path, deferred tail, who looks at the sorted class), and the sizes of the pipe's sketch buffers and
// filter pool.  Pure functions of integers and booleans -- what a HIP-side helper knows (lane_path_supported, lane_candidates_supported,
// big_filter_grid, sizeof(TableBucket)) comes in as a value.  No HIP header: a plain host compiler can include it; the rules as they
// stood before they were gathered here are the model of tests/cpp/query_rules_check.cpp, which a change of a rule has to change too.
#pragma once

#include "../../include/metacache_amd.h"   // MC_WANT_*, MC_DEFER_TAIL
#include "read_class.h"                    // the counter slots (kCnt*)

#include <algorithm>
#include <cstdint>

namespace mcamd {

// query_on_pipe, internal (the slots, which see every read on the host): no single read is longer than one lane takes -- the chunk lanes'
// kernels (launched for their work list, which would be empty) are left out.  Masked out of mc_query_device's flags.
constexpr int kQueryNoLongReads = 1 << 24;

// ---- what the caller wants ----
// MC_WANT_PARTIAL_HITS: the location lists as they are (unsorted), lane path allowed -- a key shard's side of Mode K; the queries the
// lane path does not take go through the wave kernels as with MC_WANT_ALLHITS (their lists come out sorted, which is allowed)
// MC_WANT_PARTIAL_NUMBERS: the same, and the lists are left as the 4-byte global window numbers they are stored as (mc_partial_numbers)
// MC_WANT_ALLHITS switches both off: the sorted lists of every read, wave kernels only.
struct QueryWants {
    bool allhits = false;       // the wave kernels keep their location lists (MC_WANT_ALLHITS, or partial lists)
    bool partial = false, numbers = false, features = false, deferTail = false, noLongReads = false;
};
constexpr QueryWants query_wants(int flags)
{
    const bool sorted = (flags & MC_WANT_ALLHITS) != 0;
    const bool numbers = (flags & MC_WANT_PARTIAL_NUMBERS) != 0 && !sorted;
    const bool partial = ((flags & MC_WANT_PARTIAL_HITS) != 0 || numbers) && !sorted;
    return QueryWants{sorted || partial, partial, numbers, (flags & MC_WANT_FEATURES) != 0, (flags & MC_DEFER_TAIL) != 0, (flags & kQueryNoLongReads) != 0};
}
// the exact wave kernel finishes its reads' candidates itself (no lists kept, no taxon key to sort along)
constexpr bool wave_fuses_candidates(QueryWants w, bool taxkey) { return !w.allhits && !taxkey; }

// ---- the lane path: one lane per short read for sketching and candidates (top candidates only: sorted lists and more candidates than a
// lane keeps go through the wave kernels).  sketchOk / candsOk: lane_path_supported(sp) / lane_candidates_supported(K) ----
constexpr bool lane_path_takes(bool sketchOk, bool candsOk, bool useLanePath, QueryWants w) { return sketchOk && useLanePath && (!w.allhits || w.partial) && candsOk; }

// ---- the lane stage's order ----
struct LaneSwitches { int quadLookup, fuseLane, filterLookup, gwFuse; uint32_t keyShards; };   // mc_set_tuning's switches (-1: by the rule), cfg.key_shard_count
struct LaneTable { uint64_t nbuckets; uint32_t bucketBytes; bool compact, direct; };           // the first part: buckets, sizeof(TableBucket), store, direct index
struct BatchShape { uint32_t n; bool windowsPerRead; uint32_t uniformWindows; };               // reads; max_win given per read, else the one range of all
enum class LaneOrder { FilterLookup, Fused, Apart };
struct LaneStage { LaneOrder order; bool maskFeatures; };
constexpr uint32_t kLookMaxReads = 1u << 20;    // larger batches skip the host's look at the counters and launch everything
// Fused: sketching + probing in ONE kernel where the lookups wait for HBM (tables beyond the infinity cache: quad-cooperative fetches) -- the
// sketching of some waves runs under the waiting of others (5.27 -> 5.08 ms per 5 x 10^6 reads at full scale); small tables keep
// the two kernels (the ALU phase at the probe kernel's occupancy cost 5 % on configs[1]).  "lane_fusion" / MC_LANE_FUSION: 0 / 1 force it.
// (A key shard's side of Mode K masks the features it does not own between the two: not fused.)
// FilterLookup ("filter_lookup"): the lookups of reads of up to 64 features inside the filter kernel (gw_filter_count_kernel<LOOKUP>, behind
// the wave kernel's rejoin); the lane kernel only sketches, the mid / hash kernels wait for the filter's work lists.  Every kernel is launched
// without a look at the counters.  -1: tables whose direct index the size rule built (bucket table of 8 GiB or more), on batches that
// skip the host's look anyway (MC_DEFER_TAIL or more than 2^20 reads); 1: wherever a direct index exists (tests, A/B runs); 0: never.
// (auto only for the batches it was measured on and won: one window range for all reads, of at most 3 windows -- single reads of up to
// two windows.  Batches with a window range per read (long reads, mixed lengths) were measured 1.5 ms per step SLOWER with it, read pairs
// (range 4) have not been measured: both keep the old order.  docs/LAB_NOTEBOOK_r07.md section 5)
constexpr LaneStage lane_stage(QueryWants w, LaneSwitches sw, LaneTable t, BatchShape b)
{
    const bool maskFeatures = w.partial && !w.features && sw.keyShards > 1;
    const bool quadTable = sw.quadLookup >= 0 ? sw.quadLookup != 0 : t.nbuckets * 64ull > (1ull << 30);
    const bool fuseSketch = !maskFeatures && (sw.fuseLane >= 0 ? sw.fuseLane != 0 : quadTable);
    const bool noHostLook = w.deferTail || b.n > kLookMaxReads;
    const bool shortSingles = !b.windowsPerRead && b.uniformWindows <= 3u;
    const bool sizeBuiltIndex = t.nbuckets * t.bucketBytes >= (8ull << 30);
    const bool filterLookup = t.compact && t.direct && !w.partial && !w.allhits && !maskFeatures && sw.gwFuse == 1 &&
                              (sw.filterLookup > 0 || (sw.filterLookup < 0 && noHostLook && shortSingles && sizeBuiltIndex));
    return LaneStage{filterLookup ? LaneOrder::FilterLookup : fuseSketch ? LaneOrder::Fused : LaneOrder::Apart, maskFeatures};
}

// ---- which instance of gw_filter_count_kernel<LOOKUP> walks the batch's reads ----
// The kernel has instances compiled for ONE window range and ONE candidate count (round 11: the frame, the neighbour windows and the K
// rounds are constants of their code).  A batch gets one when its reads share a window range (no range per read) of 2 or 3 windows and it
// asks for 1 or 2 candidates per read -- the reference's defaults for single reads of up to 224 bp; {0, 0}: the instance for any batch.
struct LookupShape { uint32_t maxWin, k; };
constexpr bool operator==(LookupShape a, LookupShape b) { return a.maxWin == b.maxWin && a.k == b.k; }
constexpr LookupShape lookup_shape(bool windowsPerRead, uint32_t uniformWindows, uint32_t maxCand)
{
    const bool fixed = !windowsPerRead && (uniformWindows == 2u || uniformWindows == 3u) && (maxCand == 1u || maxCand == 2u);
    return fixed ? LookupShape{uniformWindows, maxCand} : LookupShape{0u, 0u};
}
// the name under which mc_timing_get counts the launches of the picked instance (tests look at it; no kernel is timed under it)
constexpr const char* lookup_shape_name(LookupShape f)
{
    return f.maxWin == 3u ? (f.k == 2u ? "gw_filter_lookup_w3_k2" : "gw_filter_lookup_w3_k1")
         : f.maxWin == 2u ? (f.k == 2u ? "gw_filter_lookup_w2_k2" : "gw_filter_lookup_w2_k1") : "gw_filter_lookup_any";
}

// ---- the work lists' counters as the host knows them ----
// small batches take one look at the work lists and launch only the kernels with work (a launch costs as much as such a batch's kernel:
// 0.37 -> 0.32 ms per 65 536 reads); large ones skip the round trip and launch everything.  MC_DEFER_TAIL: no look either -- the caller has
// another batch to enqueue; partial lists: no candidate kernels at all, the wave kernels for the rest.
constexpr uint32_t kPlanCounters = 16;          // (= kHostCounters, kernels.h: the slots launch_flag_count_host copies)
struct HostCounters {
    uint32_t w[kPlanCounters];
    bool all;                                   // nobody looked: every kernel is launched
    constexpr uint32_t operator[](uint32_t slot) const { return w[slot]; }
};
constexpr HostCounters counters_all() { return HostCounters{{1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1}, true}; }
constexpr HostCounters counters_none()
{
    HostCounters c{{}, false};
    c.w[kCntWaveSketch] = c.w[kCntWaveCands] = 1;
    return c;
}
inline HostCounters counters_seen(const uint32_t* words)
{
    HostCounters c{{}, false};
    std::copy(words, words + kPlanCounters, c.w);
    return c;
}
constexpr HostCounters counters_unseen(QueryWants w) { return w.partial ? counters_none() : counters_all(); }
constexpr bool host_looks(QueryWants w, uint32_t n, LaneOrder order) { return !w.partial && n <= kLookMaxReads && !w.deferTail && order != LaneOrder::FilterLookup; }

// ---- what follows from the counters (lane path) ----
struct TailPlan {
    bool waveFirst = false;     // compact store: the wave kernel's sketching and probing first, so that its reads can join the filtered path
    bool streamOrder = false;   // reads beyond kGwSmallH locations may come: the stream filter's order scratch is needed
    bool defer = false;         // MC_DEFER_TAIL holds: everything the host has to look at device counters for waits for mc_query_finish
    bool waveWork = true;       // the wave tail runs (always without the lane path; big_cands hands a few queries on to the wave kernels)
    bool sortedInTail = false;  // small batches: the sorted class's counter is looked at together with the wave tail's total (one round trip for both)
    bool filtered = false, second = false, deferSorted = false;   // the filtered path runs; with its second instance; leaves its sorted class to a later step
    bool tailSortedPath = false;   // (deferred) mc_query_finish runs the sorted class
};
constexpr TailPlan tail_plan(QueryWants w, bool compact, uint32_t n, const HostCounters& c)
{
    TailPlan p;
    p.waveFirst = compact && !w.partial && c[kCntWaveSketch] != 0;
    p.streamOrder = compact && !w.partial && n <= kLookMaxReads && (c.all || c[kCntSecond] != 0);
    p.defer = w.deferTail && c.all && !w.features;
    p.waveWork = w.partial || c[kCntWaveSketch] != 0 || c[kCntWaveCands] != 0 || c[kCntFilter] != 0;
    p.filtered = c[kCntFilter] != 0 || p.waveFirst;
    p.sortedInTail = !c.all && !p.defer && compact && p.waveWork && p.filtered;
    p.second = c[kCntSecond] != 0;
    p.deferSorted = p.defer || p.sortedInTail;
    p.tailSortedPath = compact && p.filtered;
    return p;
}

// ---- the pipe's sketch sizes: windows <= chars/stride + 2 per sequence (row 1), so the sketch buffers can be sized without a sync ----
struct SketchSizes { uint64_t maxWindows, nfeat; bool fits; };   // fits: the feature index stays inside 32 bits
constexpr SketchSizes sketch_sizes(uint32_t n, uint64_t numChars, uint32_t stride, uint32_t s)
{
    const uint64_t maxWindows = numChars / stride + 4ull * n + 1;
    return SketchSizes{maxWindows, maxWindows * s, maxWindows * s <= 0xFFFFFFF0ull};
}

// ---- the pool of the filtered location lists: one slice per wave of the filter kernels' grid (grid: big_filter_grid blocks of 4 waves),
// compact store: behind the slices an OVERFLOW region for filtered lists that may not fit their wave's slice (the longest reads of a
// batch keep 10^5 numbers), reserved with one atomic per such read (kCntOverflow).  Entries are 32-bit indices: both clamped. ----
struct PoolSizes { uint64_t poolCap, ovfCap; };
constexpr uint64_t kPoolMax = 0xFFFFFFF0ull;
constexpr PoolSizes filter_pool(uint64_t demand, uint32_t grid, uint64_t perWave, bool overflow)
{
    const uint64_t poolCap = std::min<uint64_t>(kPoolMax, std::max<uint64_t>(demand, (uint64_t)grid * 4 * perWave));
    return PoolSizes{poolCap, overflow ? std::min<uint64_t>(kPoolMax - poolCap, std::max<uint64_t>(poolCap / 4, 8ull << 20)) : 0};
}
// per wave: one full batch of gw_filter_kernel (2 112 numbers); long reads keep up to 65 535
constexpr uint64_t wave_slice(uint64_t perRead) { return std::min<uint64_t>(131072, std::max<uint64_t>(4096, perRead)); }
// mean list of a 2-window read beyond 64 locations (tables whose features have few locations each never produce filtered lists: a token
// pool; a full pool sends lists to the wave kernel)
inline bool long_lists(uint64_t locs, uint64_t keys, uint32_t s) { return (double)locs / (double)std::max<uint64_t>(keys, 1) * 2.0 * s > 64.0; }
// a batch of reads: 448 per 150 bp read = 3 per base (longer reads collect -- and keep -- in proportion)
constexpr PoolSizes batch_pool(uint32_t n, uint64_t numChars, bool longLists, uint32_t grid, bool compact)
{
    return filter_pool(longLists ? std::max<uint64_t>((uint64_t)n * 448, numChars * 3) : (uint64_t)n * 8, grid, wave_slice(64 * (numChars / std::max<uint32_t>(n, 1))), compact);
}
// Mode K, owner side: the union of 8-byte lists (no overflow region), the received window numbers (totalIn of them)
constexpr PoolSizes owner_lists_pool(uint32_t n, uint32_t grid) { return filter_pool((uint64_t)n * 448, grid, 1024, false); }
constexpr PoolSizes owner_numbers_pool(uint32_t n, uint64_t totalIn, uint32_t grid)
{
    return filter_pool(std::max<uint64_t>((uint64_t)n * 448, totalIn / 2), grid, wave_slice(totalIn / std::max<uint32_t>(n, 1)), true);
}

}  // namespace mcamd
