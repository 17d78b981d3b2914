// tests/cpp/query_rules_check.cpp -- host check of csrc/query_rules.h: the host's batch plan against the expressions it was gathered
// from, written flat here exactly as they stood in context.cpp at commit 0978f76 (the line each came from is named beside it), over the
// full product of their inputs.  The model stays as the specification: a change of a rule changes it too.
// Stand-alone: tests/test_query_rules_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include "query_rules.h"
#include "table_rules.h"   // TableBucket

#include <algorithm>
#include <cstdio>

using namespace mcamd;

static int g_bad = 0;
// a part's line: "<part> ok: N cases" only where nothing of it differed
static void report(const char* part, uint64_t cases, int badBefore) { std::printf("%s %s: %llu cases\n", part, g_bad == badBefore ? "ok" : "BAD", (unsigned long long)cases); }
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static const int kFlagBits[6] = {MC_WANT_ALLHITS, MC_WANT_FEATURES, MC_WANT_PARTIAL_HITS, MC_WANT_PARTIAL_NUMBERS, MC_DEFER_TAIL, kQueryNoLongReads};
static int flags_of(int combo) { int f = 0; for (int b = 0; b < 6; ++b) if (combo >> b & 1) f |= kFlagBits[b]; return f; }

// ---- the model: context.cpp at 0978f76 ---------------------------------------------------------------------------------------------------
struct ModelWants { bool wantNumbers, wantPartial; int wantAllhits; bool wantFeatures; };
static ModelWants model_wants(int flags)
{
    const bool wantNumbers = (flags & MC_WANT_PARTIAL_NUMBERS) != 0 && !(flags & MC_WANT_ALLHITS);                          // :627
    const bool wantPartial = ((flags & MC_WANT_PARTIAL_HITS) != 0 || wantNumbers) && !(flags & MC_WANT_ALLHITS);            // :628
    const int wantAllhits = (flags & MC_WANT_ALLHITS) | (wantPartial ? 1 : 0);                                               // :629
    const bool wantFeatures = (flags & MC_WANT_FEATURES) != 0;                                                               // :630
    return ModelWants{wantNumbers, wantPartial, wantAllhits, wantFeatures};
}

// the context's switches and the first part as the model reads them
struct ModelCtx { bool useLanePath; int quadLookup, fuseLane, filterLookup, gwFuse; uint32_t key_shard_count; uint32_t nbuckets; bool compact, direct; };
struct ModelIn { const uint32_t* max_win; uint32_t max_win_uniform; };

struct ModelPlan {
    bool maskFeatures, fuseSketch, filterLookup, look;
    bool hcntIsAll, hcntIsNone;       // which array hcnt points at before the look (:739)
    bool waveDone, orderScratch, defer, waveWork, sortedInTail, filtered, second, deferSorted, tailSortedPath;
};
// hcnt / all: the pointers of :736-746 (hcnt == all: nobody looked)
static ModelPlan model_plan(int flags, const ModelCtx& ctx, const ModelIn& in, uint32_t n, const uint32_t* hcnt, const uint32_t* all)
{
    const ModelWants w = model_wants(flags);
    const bool wantPartial = w.wantPartial, wantFeatures = w.wantFeatures;
    const int wantAllhits = w.wantAllhits;
    ModelPlan m{};
    const bool maskFeatures = wantPartial && !wantFeatures && ctx.key_shard_count > 1;                                       // :699
    const bool quadTable = ctx.quadLookup >= 0 ? ctx.quadLookup != 0 : (uint64_t)ctx.nbuckets * 64ull > (1ull << 30);        // :700
    const bool fuseSketch = !maskFeatures && (ctx.fuseLane >= 0 ? ctx.fuseLane != 0 : quadTable);                            // :701
    const bool noHostLook = (flags & MC_DEFER_TAIL) != 0 || n > (1u << 20);                                                  // :706
    const bool shortSingles = in.max_win == nullptr && in.max_win_uniform <= 3u;                                             // :710
    const bool filterLookup = ctx.compact && ctx.direct && !wantPartial && !wantAllhits && !maskFeatures && ctx.gwFuse == 1 &&   // :711
                              (ctx.filterLookup > 0 || (ctx.filterLookup < 0 && noHostLook && shortSingles && (uint64_t)ctx.nbuckets * sizeof(TableBucket) >= (8ull << 30)));   // :712
    m.maskFeatures = maskFeatures; m.fuseSketch = fuseSketch; m.filterLookup = filterLookup;
    m.hcntIsNone = wantPartial; m.hcntIsAll = !wantPartial;                                                                  // :739
    m.look = !wantPartial && n <= (1u << 20) && !(flags & MC_DEFER_TAIL) && !filterLookup;                                   // :741
    bool waveDone = false;                                                                                                   // :756
    if (ctx.compact && !wantPartial && hcnt[kCntWaveSketch]) waveDone = true;                                                // :757, :761
    m.orderScratch = ctx.compact && !wantPartial && n <= (1u << 20) && (hcnt == all || hcnt[kCntSecond]);                    // :763
    const bool defer = (flags & MC_DEFER_TAIL) != 0 && hcnt == all && !wantFeatures;                                         // :773
    const bool waveWork = wantPartial || hcnt[kCntWaveSketch] != 0 || hcnt[kCntWaveCands] != 0 || hcnt[kCntFilter] != 0;     // :774
    const bool sortedInTail = hcnt != all && !defer && ctx.compact && waveWork && (hcnt[kCntFilter] || waveDone);            // :776
    m.filtered = hcnt[kCntFilter] || waveDone;                                                                               // :777
    m.second = hcnt[kCntSecond] != 0;                                                                                        // :779
    m.deferSorted = defer || sortedInTail;                                                                                   // :779
    m.tailSortedPath = ctx.compact && (hcnt[kCntFilter] || waveDone);                                                        // :786
    m.waveDone = waveDone; m.defer = defer; m.waveWork = waveWork; m.sortedInTail = sortedInTail;
    return m;
}

// ---- wants, the wave kernel's fusing, the lane-path condition of the three sites -----------------------------------------------------------
static void check_wants()
{
    const int bad0 = g_bad;
    uint64_t cases = 0;
    for (int combo = 0; combo < 64; ++combo) {
        const int flags = flags_of(combo);
        const ModelWants m = model_wants(flags);
        const QueryWants w = query_wants(flags);
        CHECK(w.numbers == m.wantNumbers && w.partial == m.wantPartial && w.allhits == (m.wantAllhits != 0) && w.features == m.wantFeatures, "wants, flags %x", flags);
        CHECK(w.deferTail == ((flags & MC_DEFER_TAIL) != 0) && w.noLongReads == ((flags & kQueryNoLongReads) != 0), "wants, flags %x", flags);
        for (int taxkey = 0; taxkey < 2; ++taxkey) {
            const bool fuse = !m.wantAllhits && !taxkey;                                                                     // :687
            CHECK(wave_fuses_candidates(w, taxkey != 0) == fuse, "fuse, flags %x taxkey %d", flags, taxkey);
            ++cases;
        }
    }
    report("wants", cases, bad0);
}

static void check_lane_path()
{
    const int bad0 = g_bad;
    uint64_t cases = 0;
    for (int combo = 0; combo < 64; ++combo)
        for (int use = 0; use < 2; ++use)
            for (int sk = 0; sk < 2; ++sk)
                for (int cd = 0; cd < 2; ++cd)
                    for (int copyAll = 0; copyAll < 2; ++copyAll) {
                        const int flags = flags_of(combo);
                        const ModelWants m = model_wants(flags);
                        const bool lane_path_supported = sk != 0, useLanePath = use != 0, lane_candidates_supported = cd != 0;
                        const bool wantAll = copyAll != 0;                                                                   // :1620
                        const bool query = lane_path_supported && useLanePath && (!m.wantAllhits || m.wantPartial) && lane_candidates_supported;   // :646
                        const bool slots = lane_path_supported && useLanePath && !wantAll && lane_candidates_supported;      // :1621
                        const bool pipes = lane_path_supported && useLanePath && lane_candidates_supported;                  // :1638
                        CHECK(lane_path_takes(sk != 0, cd != 0, use != 0, query_wants(flags)) == query, "lane path, flags %x", flags);
                        CHECK(lane_path_takes(sk != 0, cd != 0, use != 0, query_wants(copyAll ? MC_WANT_ALLHITS : 0)) == slots, "lane path of the slot pipes, copy_allhits %d", copyAll);
                        CHECK(lane_path_takes(sk != 0, cd != 0, use != 0, QueryWants{}) == pipes, "lane path of the query pipes");
                        ++cases;
                    }
    report("lane path", cases, bad0);
}

// ---- lane stage, the host's look, what follows from the counters ------------------------------------------------------------------------------
static void check_plan()
{
    const int bad0 = g_bad;
    uint64_t cases = 0;
    uint32_t all[kPlanCounters], none[kPlanCounters] = {};                                                                   // :736
    std::fill(all, all + kPlanCounters, 1u);                                                                                 // :737
    none[kCntWaveSketch] = none[kCntWaveCands] = 1;                                                                          // :738
    // the counters a batch may come with: nobody looked (all), partial lists (none), the host's words with the four slots the plan reads
    // zero and non-zero (the others: a value the plan must not read as theirs)
    uint32_t seen[16][kPlanCounters];
    const uint32_t slots[4] = {kCntWaveSketch, kCntWaveCands, kCntFilter, kCntSecond};
    for (uint32_t v = 0; v < 16; ++v) {
        for (uint32_t i = 0; i < kPlanCounters; ++i) seen[v][i] = (v * 7 + i) % 3;
        for (uint32_t s = 0; s < 4; ++s) seen[v][slots[s]] = (v >> s & 1) ? 1 + v * (s + 1) : 0;
    }
    const uint32_t someWindows[2] = {3, 5};
    const uint32_t bucketBorders[4] = {1u << 24, (1u << 24) + 1, (1u << 27) - 1, 1u << 27};   // nbuckets * 64 > 2^30; nbuckets * sizeof(TableBucket) >= 8 GiB
    static_assert(sizeof(TableBucket) == 64, "the borders above");
    const uint32_t reads[4] = {0, 1, 1u << 20, (1u << 20) + 1};
    const int gwFuses[4] = {0, 1, 5, 6};
    for (int combo = 0; combo < 64; ++combo)
    for (int store = 0; store < 4; ++store)                                             // compact or 8-byte store, direct index or none
    for (uint32_t shards = 1; shards <= 2; ++shards)
    for (int quad = -1; quad <= 1; ++quad)
    for (int fusion = -1; fusion <= 1; ++fusion)
    for (int lookup = -1; lookup <= 1; ++lookup)
    for (int gf = 0; gf < 4; ++gf)
    for (int nb = 0; nb < 4; ++nb)
    for (int ni = 0; ni < 4; ++ni)
    for (int win = 0; win < 3; ++win) {                                                 // a window range per read, or one range of 3 / of 4 for all
        const int flags = flags_of(combo);
        const ModelCtx ctx{true, quad, fusion, lookup, gwFuses[gf], shards, bucketBorders[nb], (store & 1) != 0, (store & 2) != 0};
        const ModelIn in{win == 0 ? someWindows : nullptr, win == 0 ? 0u : win == 1 ? 3u : 4u};
        const uint32_t n = reads[ni];
        const QueryWants w = query_wants(flags);
        const LaneStage stage = lane_stage(w, LaneSwitches{quad, fusion, lookup, gwFuses[gf], shards}, LaneTable{bucketBorders[nb], (uint32_t)sizeof(TableBucket), ctx.compact, ctx.direct},
                                           BatchShape{n, in.max_win != nullptr, in.max_win_uniform});
        const bool looks = host_looks(w, n, stage.order);
        const HostCounters unseen = counters_unseen(w);
        for (int c = 0; c < 18; ++c) {
            const uint32_t* hcnt = c == 0 ? all : c == 1 ? none : seen[c - 2];
            const ModelPlan m = model_plan(flags, ctx, in, n, hcnt, all);
            const LaneOrder order = m.filterLookup ? LaneOrder::FilterLookup : m.fuseSketch ? LaneOrder::Fused : LaneOrder::Apart;   // :714, :719, :723
            CHECK(stage.order == order && stage.maskFeatures == m.maskFeatures, "lane stage, flags %x store %d shards %u switches %d %d %d %d buckets %u n %u win %d",
                  flags, store, shards, quad, fusion, lookup, gwFuses[gf], bucketBorders[nb], n, win);
            CHECK(looks == m.look, "host look, flags %x n %u", flags, n);
            CHECK(unseen.all == m.hcntIsAll && std::equal(unseen.w, unseen.w + kPlanCounters, m.hcntIsNone ? none : all), "unseen counters, flags %x", flags);
            const HostCounters hc = c == 0 ? counters_all() : c == 1 ? counters_none() : counters_seen(seen[c - 2]);
            CHECK(hc.all == (hcnt == all) && std::equal(hc.w, hc.w + kPlanCounters, hcnt), "counters %d", c);
            const TailPlan p = tail_plan(w, ctx.compact, n, hc);
            CHECK(p.waveFirst == m.waveDone && p.streamOrder == m.orderScratch && p.defer == m.defer && p.waveWork == m.waveWork && p.sortedInTail == m.sortedInTail &&
                  p.filtered == m.filtered && p.second == m.second && p.deferSorted == m.deferSorted && p.tailSortedPath == m.tailSortedPath,
                  "tail plan, flags %x compact %d n %u counters %d", flags, (int)ctx.compact, n, c);
            ++cases;
        }
    }
    const TailPlan waveOnly;                                                            // without the lane path: :690, :691
    CHECK(waveOnly.waveWork && !waveOnly.sortedInTail && !waveOnly.defer && !waveOnly.filtered && !waveOnly.waveFirst, "wave-only plan");
    report("plan", cases, bad0);
}

// ---- the pipe's sketch sizes and the three pools -----------------------------------------------------------------------------------------------
static void check_sizes()
{
    const int bad0 = g_bad;
    uint64_t sketches = 0, pools = 0;
    const uint64_t reads[7] = {0, 1, 4096, 65536, 1u << 20, 5000000, 0xFFFFFFFFull};
    // characters of a batch / numbers received: from nothing up to where both clamps bite (3 per character: 2^32 at 1.43 x 10^9)
    const uint64_t amounts[12] = {0, 1, 149, 150 * 4096ull, 1ull << 24, 150 * 5000000ull, 1ull << 30, 1431655760ull, 1431655770ull, 1ull << 32, 1ull << 33, 1ull << 36};
    const uint32_t grids[3] = {1, 256, 2048};
    const struct { uint32_t stride, s; } sketch[3] = {{112, 16}, {49, 8}, {1, 32}};
    for (uint64_t nn : reads)
        for (uint64_t numChars : amounts) {
            const uint32_t n = (uint32_t)nn;
            for (const auto& sp : sketch) {
                const uint64_t maxWindows = numChars / sp.stride + 4ull * n + 1;                                             // :587
                const bool refused = maxWindows * sp.s > 0xFFFFFFF0ull;                                                      // :588
                const size_t nfeat = (size_t)maxWindows * sp.s;                                                              // :589
                const SketchSizes z = sketch_sizes(n, numChars, sp.stride, sp.s);
                CHECK(z.maxWindows == maxWindows && z.fits == !refused && z.nfeat == nfeat, "sketch sizes, n %u chars %llu", n, (unsigned long long)numChars);
                ++sketches;
            }
            for (uint32_t grid : grids)
                for (int compact = 0; compact < 2; ++compact)
                    for (int lists = 0; lists < 2; ++lists) {
                        // longLists on and off through its own expression: 200 / 2 locations per feature at 16 features per window
                        const uint64_t locs = lists ? 200000 : 2000, keys = 1000;
                        const uint32_t s = 16;
                        const bool longLists = (double)locs / (double)std::max<uint64_t>(keys, 1) * 2.0 * s > 64.0;          // :603
                        CHECK(longLists == (lists != 0) && long_lists(locs, keys, s) == longLists, "long lists");
                        {   // a batch of reads (size_pipe)
                            const uint64_t poolCap = std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>(longLists ? std::max<uint64_t>((uint64_t)n * 448, numChars * 3) : (uint64_t)n * 8,   // :605
                                                                                                          (uint64_t)grid * 4 * std::min<uint64_t>(131072, std::max<uint64_t>(4096, 64 * (numChars / std::max<uint32_t>(n, 1))))));   // :606
                            const uint64_t ovfCap = compact ? std::min<uint64_t>(0xFFFFFFF0ull - poolCap, std::max<uint64_t>(poolCap / 4, 8ull << 20)) : 0;   // :609
                            const PoolSizes z = batch_pool(n, numChars, longLists, grid, compact != 0);
                            CHECK(z.poolCap == poolCap && z.ovfCap == ovfCap, "batch pool, n %u chars %llu grid %u", n, (unsigned long long)numChars, grid);
                        }
                        {   // owner side, 8-byte lists: no overflow region
                            const uint64_t poolCap = std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>((uint64_t)n * 448, (uint64_t)grid * 4 * 1024));   // :881
                            const PoolSizes z = owner_lists_pool(n, grid);
                            CHECK(z.poolCap == poolCap && z.ovfCap == 0, "owner pool of 8-byte lists, n %u grid %u", n, grid);
                        }
                        {   // owner side, window numbers
                            const uint64_t totalIn = numChars;
                            const uint64_t avg = totalIn / std::max<uint32_t>(n, 1);                                          // :980
                            const uint64_t poolCap = std::min<uint64_t>(0xFFFFFFF0ull, std::max<uint64_t>(std::max<uint64_t>((uint64_t)n * 448, totalIn / 2),   // :981
                                                                                                          (uint64_t)grid * 4 * std::min<uint64_t>(131072, std::max<uint64_t>(4096, avg))));   // :982
                            const uint64_t ovfCap = std::min<uint64_t>(0xFFFFFFF0ull - poolCap, std::max<uint64_t>(poolCap / 4, 8ull << 20));   // :983
                            const PoolSizes z = owner_numbers_pool(n, totalIn, grid);
                            CHECK(z.poolCap == poolCap && z.ovfCap == ovfCap, "owner pool of window numbers, n %u numbers %llu grid %u", n, (unsigned long long)totalIn, grid);
                        }
                        ++pools;
                    }
        }
    report("sketch sizes and pools", sketches + pools, bad0);
}

int main()
{
    check_wants();
    check_lane_path();
    check_plan();
    check_sizes();
    if (g_bad) { std::printf("MISMATCH: %d in all\n", g_bad); return 1; }
    return 0;
}
