// metacache_amd/csrc/query_pipe.cpp -- the per-batch pipeline on a pipe: query_on_pipe and its steps (the plan: query_rules.h), the deferred
// tail, mc_query_device / mc_query_finish, and the owner side of Mode K on the same filtered path.  (Compiled with hipcc; the kernels live
// in kernels.hip and gw_kernels.hip; context, slots and timing: context.cpp.)
#include "context.h"
#include "rows_common.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

using namespace mcamd;

static_assert(kPlanCounters == kHostCounters, "query_rules.h plans on the counters launch_flag_count_host copies");

// the pinned words a batch's host round trips land in (Pipe::hTotal), made on the pipe's first use
static int ensure_host_words(mc_ctx* ctx, Pipe& P) { if (!P.hTotal) HIP_TRY(ctx, hipHostMalloc((void**)&P.hTotal, 128)); return MC_OK; }
// a Workspace that carries the context's tuning (mc_set_tuning), no buffers yet
static Workspace tuned_workspace(const mc_ctx* ctx)
{
    Workspace ws{};
    ws.filterBpc = ctx->filterBpc; ws.countBpc = ctx->countBpc; ws.gwFuse = ctx->gwFuse; ws.gwBigH = ctx->gwBigH; ws.gwMidH = ctx->gwMidH;
    return ws;
}
// the global window numbers of the compact store (mc_load_target_windows) for the kernels that decode them
static void set_window_numbering(const mc_ctx* ctx, DeviceTable& tab)
{
    tab.gwBase = ctx->dGwBase; tab.gwDir = ctx->dGwDir; tab.gwDirShift = ctx->gwDirShift; tab.gwGap = ctx->gwGap; tab.gwTargets = ctx->gwTargets;
}
// no table: the kernels that work on gathered lists take a DeviceTable and probe nothing
static DeviceTable no_table() { return DeviceTable{nullptr, nullptr, 0, 0xFFFFFFFFu, 1}; }
// the owner side of Mode K on the filtered path: ONE entry per read (step D finds a read's entry at winOff[q] * s = q)
static SketchParams one_entry_per_read() { return SketchParams{16, 1, 16, 1}; }
// The Workspace's pointers into the pipe's buffers as they stand, in one place: what every batch has (windows, probe results, statistics,
// flags, scans) and -- lists -- the lane path's work lists, the pool and the filtered path's tables with the context's bigMin.  Sizes
// (bigPoolCap, bigOvfCap) and what depends on the call (features, chunkList, partialLists) are the caller's; what a caller borrows for
// another purpose, or its kernels need null, it overrides after the call.
static void bind_workspace(Workspace& ws, const Pipe& P, const mc_ctx* ctx, bool lists)
{
    ws.winCount = (uint32_t*)P.bWinCount.p; ws.winOff = (uint32_t*)P.bWinOff.p; ws.psize = (uint32_t*)P.bPsize.p; ws.ppay = (uint64_t*)P.bPpay.p;
    ws.qstat = (QueryStat*)P.bQstat.p; ws.hitScan = (uint32_t*)P.bScanIn.p; ws.qflag = (uint32_t*)P.bQflag.p; ws.hitOff = (uint64_t*)P.bHitOff.p;
    ws.scanTmp = P.bScan.p; ws.stats = (uint64_t*)P.bStats.p;
    if (!lists) return;
    ws.midCount = (uint32_t*)P.bMid.p; ws.midList = reinterpret_cast<uint4*>(ws.midCount + kCounterWords);
    ws.bigMin = ctx->bigMin;
    ws.bigPool = (uint64_t*)P.bBigPool.p; ws.sliceFill = (uint32_t*)P.bSliceFill.p; ws.sideList = (uint32_t*)P.bSide.p;
}
// room for `entries` locations to be sorted: the lists, the sort's scratch (a second one only where a taxon key is sorted along)
static int ensure_sort_space(mc_ctx* ctx, Pipe& P, uint64_t entries, const uint32_t* taxkey, Workspace& ws)
{
    int rc = MC_OK;
    const size_t hb = (size_t)(entries + 1) * 8;
    if ((rc = ensure(ctx, P.bHits, hb)) || (rc = ensure(ctx, P.bCscr, hb)) || (taxkey && (rc = ensure(ctx, P.bCscr2, hb)))) return rc;
    ws.hits = (uint64_t*)P.bHits.p; ws.cscr = (uint64_t*)P.bCscr.p; ws.cscr2 = (uint64_t*)P.bCscr2.p;
    return MC_OK;
}
// what every candidate call hands back: the pipe's candidates and hit counts, the sorted location lists where the call delivers them
static void publish_results(mc_device_results* out, const Pipe& P, const Workspace& ws, bool withLists)
{
    out->cands = (const mc_candidate*)P.bCands.p; out->hit_counts = (const uint32_t*)P.bQstat.p;   // (QueryStat.hits: stride 4 words)
    out->hit_offsets = withLists ? ws.hitOff : nullptr;
    out->hits = withLists ? (const mc_location*)ws.hits : nullptr;
    out->features = nullptr; out->win_offsets = nullptr;
}

// the sorted class of the filtered path: filtered lists the counting kernels do not take (long reads: thousands of numbers, wide window
// ranges) are sorted -- one segmented sort over the pool -- and scanned (gw_sorted_cands_kernel); the filter kernels counted them.
// The one place of the filtered path where the host looks at a device counter (how many such lists: the sort's segment count).
static int run_sorted_tail(mc_ctx* ctx, Pipe& P, BatchRun& r, bool counterCopied)
{
    int rc = MC_OK;
    Workspace& ws = r.ws;
    const uint32_t n = r.b.n;
    hipStream_t st = r.st;
    if ((rc = ensure_host_words(ctx, P))) return rc;
    uint32_t* nsorted = reinterpret_cast<uint32_t*>(P.hTotal + 9);
    if (!counterCopied) launch_words_to_host(nsorted, ws.midCount + kCntSorted, 1, st);
    HIP_TRY(ctx, traced_sync(st));
    {   // MC_GW_DIAG=1: the batch's work-list counters on stderr (the classes of the filtered path)
        static const bool diag = [] { const char* e = std::getenv("MC_GW_DIAG"); return e && e[0] == '1'; }();
        if (diag) {
            uint32_t mc[kCounterWords];
            HIP_TRY(ctx, hipMemcpy(mc, ws.midCount, sizeof mc, hipMemcpyDeviceToHost));
            std::fprintf(stderr, "[gw diag] n %u filtered %u | stream filter %u | counted apart: 257..512 %u, 513..1024 %u | sorted %u\n",
                         n, mc[kCntFilter], mc[kCntStream], mc[kCnt512], mc[kCnt1024], mc[kCntSorted]);
        }
    }
    if (!*nsorted) return MC_OK;
    if ((rc = ensure(ctx, P.bBigPool2, r.poolEntries * 4))) return rc;
    ws.bigPool2 = (uint32_t*)P.bBigPool2.p;
    const uint32_t nseg = std::min(*nsorted, n);
    // the sorted class longest list first: the segmented sort (a block per segment) and the scan (a wave per list) take them in this order
    size_t ordBytes = 0;
    if (launch_gw_order(kSideSorted, ws, n, nseg, nullptr, ordBytes, st) != 0) return fail(ctx, MC_ERR_HIP, "ordering of the sorted lists: size query failed");
    if ((rc = ensure(ctx, P.bOrder, (size_t)3 * std::max<uint32_t>(n, 1) * 4 + ordBytes + 256))) return rc;
    size_t tmpBytes = 0;
    if (launch_gw_segsort(nullptr, tmpBytes, (const uint32_t*)ws.bigPool, ws.bigPool2, r.poolEntries, ws, n, nseg, ctx->gwBits, st) != 0)
        return fail(ctx, MC_ERR_HIP, "segmented sort: size query failed");
    if ((rc = ensure(ctx, P.bSortTmp, tmpBytes + 256))) return rc;
    {
        ScopedTimer t(ctx, "gw_sort", st);
        if (launch_gw_order(kSideSorted, ws, n, nseg, (uint32_t*)P.bOrder.p, ordBytes, st) != 0) return fail(ctx, MC_ERR_HIP, "ordering of the sorted lists failed");
        if (!P.sortSide.stream) {
            if (hipStreamCreateWithFlags(&P.sortSide.stream, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&P.sortSide.fork, hipEventDisableTiming) != hipSuccess ||
                hipEventCreateWithFlags(&P.sortSide.join, hipEventDisableTiming) != hipSuccess) P.sortSide = GwSortSide{};
        }
        if (launch_gw_segsort(P.bSortTmp.p, tmpBytes, (const uint32_t*)ws.bigPool, ws.bigPool2, r.poolEntries, ws, n, nseg, ctx->gwBits, st, &P.sortSide) != 0)
            return fail(ctx, MC_ERR_HIP, "segmented sort failed");
    }
    { ScopedTimer t(ctx, "gw_sorted_cands", st); launch_big_cands(FilterStep::SortedCands, r.b, r.sp, r.tab, ws, r.K, r.taxkey, r.cands, st); }
    return MC_OK;
}

// The filtered candidate path on the work list the probing kernels (or, on the owner side of Mode K, owner_entries_kernel) left
// in kListFilter: filter -> counting -> [segmented sort -> scan of the sorted lists].
// second (8-byte store): reads beyond the first filter's reach take its second instance.
// deferSorted: the sorted class is left to the caller (mc_query_finish runs run_sorted_tail).
// The path's first step alone: the filter (compact store, "filter_lookup": followed by gw_filter_count_kernel<LOOKUP> inside the SAME pair of
// timer events -- the timer's count stays one per batch).  The caller launches what waits for the LOOKUP instance's work lists (the mid / hash
// kernels) between this and run_filtered_path(.., filterDone = true).
static void run_filter_step(mc_ctx* ctx, BatchRun& r)
{
    ScopedTimer t(ctx, r.compact ? (r.ws.gwFuse ? "gw_filter_count" : "gw_filter") : "big_filter", r.st);
    launch_big_cands(FilterStep::Filter, r.b, r.sp, r.tab, r.ws, r.K, r.taxkey, r.cands, r.st);
    if (r.compact && r.ws.filterLookup) {
        launch_big_cands(FilterStep::FilterLookup, r.b, r.sp, r.tab, r.ws, r.K, r.taxkey, r.cands, r.st);
        if (ctx->timing) {                                         // which LOOKUP instance the launcher's rule picked: a launch count, no events
            std::lock_guard<std::mutex> l(ctx->timerMtx);
            ++ctx->timers[lookup_shape_name(lookup_shape(r.b.maxWin != nullptr, r.b.maxWinUniform, r.K))].launches;
        }
    }
}

static int run_filtered_path(mc_ctx* ctx, Pipe& P, BatchRun& r, bool second, bool deferSorted = false, bool filterDone = false)
{
    // timers carry the kernels' own names, one kernel each (a bench line's dominant "kernel" must be one): compact store gw_filter_count_kernel
    // (or gw_filter_kernel with "gw_fuse" 0), gw_filter2, gw_compact (+ the ordering of the stream filter's reads), gw_filter_stream<fine>,
    // <mid>, gw_filter_stream (+ the second compaction), gw_count_kernel<9>, <10>, <11>; 8-byte store: big_*
    // (compact store: gw_filter_kernel itself may leave reads to the second kernel -- it counts them on the device, after the
    // host's look at the counters: always launched, returns at once with nothing to do)
    if (!filterDone) run_filter_step(ctx, r);
    const bool compact = r.compact, always = true, compactOnly = compact, wideSecond = !compact && second;   // when a step runs
    const struct { FilterStep step; const char* timer; bool when; } steps[] = {
        {FilterStep::PairFilter, "gw_filter2", compactOnly},
        {FilterStep::Compact, "gw_compact", compactOnly},
        {FilterStep::StreamFine, "gw_filter_stream_fine", compactOnly},
        {FilterStep::StreamMid, "gw_filter_stream_mid", compactOnly},
        {FilterStep::Stream, "gw_filter_stream", compactOnly},
        {FilterStep::BigFilter2, "big_filter_2", wideSecond},
        {FilterStep::Count, compact ? "gw_count" : "big_count", always},
        {FilterStep::Count512, "gw_count_512", compactOnly},
        {FilterStep::Count1024, compact ? "gw_count_1024" : "big_count_2", always},
    };
    for (const auto& s : steps)
        if (s.when) { ScopedTimer t(ctx, s.timer, r.st); launch_big_cands(s.step, r.b, r.sp, r.tab, r.ws, r.K, r.taxkey, r.cands, r.st); }
    if (compact && !deferSorted) return run_sorted_tail(ctx, P, r, false);
    return MC_OK;
}

// What the lane path did not finish goes through the exact wave kernels (long reads, duplicate hashes, reads the filtered path handed
// back, -allhits, ...): sketch + probe unless done, segments for their location lists (the host sizes them: one round trip), sort + candidates.
// sortedIsMine (small batches whose filtered path left its sorted class to this call): the host's look at that class's counter shares this
// call's one round trip -- the wave kernels' sketching and the scan go out first; in the rare batch that has sorted lists they run again
// behind run_sorted_tail (query_kernel takes the reads still flagged for it: a second pass finds only what the sorted class handed back).
static int run_wave_tail(mc_ctx* ctx, Pipe& P, BatchRun& r, bool sortedIsMine = false)
{
    int rc = MC_OK;
    Workspace& ws = r.ws;
    const BatchView& b = r.b;
    const uint32_t n = b.n;
    hipStream_t st = r.st;
    if ((rc = ensure_host_words(ctx, P))) return rc;
    auto sketch_and_scan = [&]() {
        if (!r.skipWaveSketch) { ScopedTimer t(ctx, "query_wave", st); launch_query(b, r.sp, r.tab, r.fuse, r.wantAllhits, ws, r.K, r.cands, st); }
        ScopedTimer t(ctx, "scan", st);
        // (how many locations need a segment in HBM: the total goes to pinned host memory with the scan)
        launch_scan_u32(ws.hitScan, 1, n, nullptr, ws.hitOff, ws.scanTmp, st, P.hTotal);
    };
    sketch_and_scan();
    uint32_t* nsorted = reinterpret_cast<uint32_t*>(P.hTotal + 9);
    if (sortedIsMine) launch_words_to_host(nsorted, ws.midCount + kCntSorted, 1, st);
    HIP_TRY(ctx, traced_sync(st));
    if (sortedIsMine && *nsorted) {
        if ((rc = run_sorted_tail(ctx, P, r, true))) return rc;
        sketch_and_scan();
        HIP_TRY(ctx, traced_sync(st));
    }
    const uint64_t totalHits = *P.hTotal;
    if ((rc = ensure_sort_space(ctx, P, totalHits, r.taxkey, ws))) return rc;
    if (r.wantNumbers && ((rc = ensure(ctx, P.bNumbers, (size_t)(totalHits + 8) * 4)) || (rc = ensure(ctx, P.bCounts, (size_t)(n + 1) * 4)))) return rc;
    if (r.wantPartial && r.lanePath && !r.wantNumbers) { ScopedTimer t(ctx, "gather_lists", st); launch_gather_lists(b, r.sp, r.tab, ws, nullptr, st); }
    { ScopedTimer t(ctx, "sort_candidates", st); launch_sort_candidates(b, r.sp, r.tab, ws, r.taxkey, r.K, r.wantAllhits, r.cands, st); }
    if (r.wantNumbers) {
        // what the wave kernels left in ws.hits -> numbers, then the lane path's (and the chunk lanes') lists straight from the table
        { ScopedTimer t(ctx, "pack_numbers", st); launch_pack_other_reads(b, r.tab, ws, (uint32_t*)P.bNumbers.p, (uint32_t*)P.bCounts.p, st); }
        if (r.lanePath) { ScopedTimer t(ctx, "gather_lists", st); launch_gather_lists(b, r.sp, r.tab, ws, (uint32_t*)P.bNumbers.p, st); }
        P.numbersN = n; P.numbersTotal = totalHits;
    }
    return MC_OK;
}

// the rare classes of a batch whose main kernels mc_query_device(MC_DEFER_TAIL) enqueued: sorted lists, then the exact wave kernels
int mcamd::finish_on_pipe(mc_ctx* ctx, Pipe& P)
{
    Pipe::Tail& tl = P.tail;
    if (!tl.pending) return MC_OK;
    tl.pending = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(tl.mainDone));
    int rc = MC_OK;
    tl.run.wantAllhits = false; tl.run.wantPartial = false; tl.run.wantNumbers = false; tl.run.lanePath = true;   // (only top candidates on the lane path are deferred)
    if (tl.sortedPath && (rc = run_sorted_tail(ctx, P, tl.run, true))) return rc;
    if ((rc = run_wave_tail(ctx, P, tl.run))) return rc;
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

// A call takes pipe P: the device, pipe1's stream on its first use, the tail of a batch the caller deferred on P and never asked for (it
// still owns the workspace this call is about to reuse), and the stream the call enqueues on -- the caller's, else the pipe's own
int mcamd::enter_pipe(mc_ctx* ctx, Pipe& P, void* streamv, hipStream_t& st)
{
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (&P == &ctx->pipe1 && !ctx->pipe1.stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->pipe1.stream, hipStreamNonBlocking));
    if (const int rc = finish_on_pipe(ctx, P)) return rc;
    st = streamv ? (hipStream_t)streamv : P.stream;
    return MC_OK;
}

// A pipe's buffers whose sizes follow from the batch's size (n queries, numChars characters) and the table's mean list length alone --
// everything mc_query_device needs before its first host round trip.  mc_open_database calls this for every slot pipe WHILE the file
// loads (reserve_slot_pipes): a hipMalloc of memory another process has just given back takes 100-200 ms per 600 MB, and eight pipes
// growing their pools inside the first batches made the same `mcq query` run take 81 or 390 ms per 10^7 reads.
int mcamd::size_pipe(mc_ctx* ctx, Pipe& P, uint32_t n, uint64_t numChars, bool wantFeatures, bool lanePath, uint64_t locs, uint64_t keys, PipeSizes& out)
{
    int rc = MC_OK;
    const SketchParams sp = ctx->querySketch;
    const uint32_t K = ctx->cfg.max_candidates;
    const SketchSizes sk = sketch_sizes(n, numChars, sp.stride, sp.s);
    if (!sk.fits) return fail(ctx, MC_ERR_UNSUPPORTED, "batch too large (feature index exceeds 32 bits)");
    const size_t nfeat = (size_t)sk.nfeat;
    if ((rc = ensure(ctx, P.bWinCount, (size_t)(n + 1) * 4))) return rc;
    if ((rc = ensure(ctx, P.bWinOff, (size_t)(n + 2) * 4))) return rc;
    // (the lane path delivers top candidates only: -allhits and K > 4 go through the wave kernels)
    if ((wantFeatures || lanePath) && (rc = ensure(ctx, P.bFeatures, nfeat * 4))) return rc;
    if ((rc = ensure(ctx, P.bPsize, nfeat * 4))) return rc;
    if ((rc = ensure(ctx, P.bPpay, nfeat * 8))) return rc;
    if ((rc = ensure(ctx, P.bQstat, (size_t)(n + 1) * sizeof(QueryStat)))) return rc;
    if ((rc = ensure(ctx, P.bScanIn, (size_t)(n + 1) * 4))) return rc;
    if ((rc = ensure(ctx, P.bQflag, (size_t)(n + 1) * 4))) return rc;
    if (lanePath && (rc = ensure(ctx, P.bMid, work_lists_bytes(n)))) return rc;
    // pool of the filtered location lists (big_filter_kernel -> big_count_kernel; compact store: with its overflow region): batch_pool
    const Part& T0 = ctx->parts[0];
    const uint32_t grid = big_filter_grid(n, T0.compact, ctx->filterBpc);
    const PoolSizes pool = batch_pool(n, numChars, long_lists(locs, keys, sp.s), grid, T0.compact);
    if (lanePath && (rc = ensure(ctx, P.bBigPool, (pool.poolCap + pool.ovfCap) * (T0.compact ? 4 : 8)))) return rc;   // the pool holds the table's location form
    if (lanePath && (rc = ensure(ctx, P.bSliceFill, (size_t)grid * 4 * 4 + 64))) return rc;
    if (lanePath && T0.compact && (rc = ensure(ctx, P.bSide, (size_t)kSideRows * std::max<uint32_t>(n, 1) * 4))) return rc;
    if (lanePath && (rc = ensure(ctx, P.bChunkList, (size_t)(sk.maxWindows + n + 1) * 8))) return rc;
    if ((rc = ensure(ctx, P.bHitOff, (size_t)(n + 2) * 8))) return rc;
    if ((rc = ensure(ctx, P.bScan, scan_tmp_bytes(n + 1)))) return rc;
    if ((rc = ensure(ctx, P.bStats, 64))) return rc;
    if ((rc = ensure(ctx, P.bCands, (size_t)std::max<uint32_t>(n, 1) * K * sizeof(mc_candidate)))) return rc;
    out.poolCap = pool.poolCap; out.ovfCap = pool.ovfCap; out.nfeat = nfeat;
    return MC_OK;
}

// the table as the batch's kernels see it: the first part's buckets and location store (compact: the window numbers)
static DeviceTable table_view(const mc_ctx* ctx)
{
    const Part& T = ctx->parts[0];
    const bool multiPart = ctx->parts.size() > 1;
    DeviceTable tab{T.dbuckets, T.dvalues, T.nbuckets, multiPart ? 0x00FFFFFFu : 0xFFFFFFFFu, T.maxProbe};
    if (T.compact) {
        tab.values = nullptr; tab.values32 = reinterpret_cast<const uint32_t*>(T.dvalues);
        set_window_numbering(ctx, tab);
    }
    tab.direct = T.ddirect;                                       // (the lane path's lookups; every other kernel goes through the buckets)
    return tab;
}

// windows per read and their scan; true (small batches): plan + scan + the clearing of the work-list counters `zero32` in one launch
static bool run_plan(mc_ctx* ctx, const BatchRun& r, uint32_t* zero32)
{
    ScopedTimer t(ctx, "plan", r.st);
    if (launch_plan_scan_small(r.b, r.sp, r.ws.winCount, r.ws.winOff, zero32, r.st)) return true;
    launch_plan(r.b, r.sp, r.ws.winCount, r.st);
    launch_scan_u32(r.ws.winCount, 1, r.b.n, r.ws.winOff, nullptr, r.ws.scanTmp, r.st);
    return false;
}

// short reads: one lane per query for sketching and candidates, cooperative probing in between -- in the order the plan chose (lane_stage)
static void run_lane_stage(mc_ctx* ctx, BatchRun& r, LaneStage stage, size_t nfeat)
{
    const BatchView& b = r.b;
    const SketchParams& sp = r.sp;
    Workspace& ws = r.ws;
    hipStream_t st = r.st;
    const int quad = ctx->quadLookup;
    if (stage.order == LaneOrder::FilterLookup) {
        { ScopedTimer t(ctx, "sketch_lane", st); launch_sketch_lane(b, sp, ws, st); }
        { ScopedTimer t(ctx, "chunk_sketch", st); launch_chunk_sketch(b, sp, ws, st); }
        { ScopedTimer t(ctx, "chunk_probe", st); launch_chunk_probe(b, sp, r.tab, ws, quad, st); }
        { ScopedTimer t(ctx, "probe_cands", st); launch_probe_cands(b, sp, r.tab, ws, r.K, r.taxkey, r.cands, quad, st); }   // (reads of more than 64 features)
    } else if (stage.order == LaneOrder::Fused) {
        { ScopedTimer t(ctx, "sketch_probe", st); launch_sketch_probe_lane(b, sp, r.tab, ws, r.K, r.taxkey, r.cands, quad, st); }
        { ScopedTimer t(ctx, "chunk_sketch", st); launch_chunk_sketch(b, sp, ws, st); }
        { ScopedTimer t(ctx, "chunk_probe", st); launch_chunk_probe(b, sp, r.tab, ws, quad, st); }
    } else {
        { ScopedTimer t(ctx, "sketch_lane", st); launch_sketch_lane(b, sp, ws, st); }
        { ScopedTimer t(ctx, "chunk_sketch", st); launch_chunk_sketch(b, sp, ws, st); }
        // a key shard's side of Mode K: only the features this shard owns are looked up (the others cannot be in its table)
        if (stage.maskFeatures) {
            ScopedTimer t(ctx, "mask_features", st);
            launch_mask_foreign_features(ws.features, ws.winOff + b.n, sp.s, nfeat, ctx->cfg.key_shard_index, ctx->cfg.key_shard_count, st);
        }
        { ScopedTimer t(ctx, "chunk_probe", st); launch_chunk_probe(b, sp, r.tab, ws, quad, st); }
        { ScopedTimer t(ctx, "probe_cands", st); launch_probe_cands(b, sp, r.tab, ws, r.K, r.taxkey, r.cands, quad, st); }
    }
}

// the mid / hash kernels of the work lists that hold reads, as far as the host knows
static void run_mid_and_hash(mc_ctx* ctx, BatchRun& r, const HostCounters& cnt)
{
    hipStream_t st = r.st;
    if (cnt[kCntMid64]) { ScopedTimer t(ctx, "mid_cands_64", st); launch_mid_cands(kListMid64, r.b, r.tab, r.ws, r.K, r.taxkey, r.cands, st); }
    if (cnt[kCntMid128]) { ScopedTimer t(ctx, "mid_cands_128", st); launch_mid_cands(kListMid128, r.b, r.tab, r.ws, r.K, r.taxkey, r.cands, st); }
    if (cnt[kCntMid256]) { ScopedTimer t(ctx, "mid_cands_256", st); launch_mid_cands(kListMid256, r.b, r.tab, r.ws, r.K, r.taxkey, r.cands, st); }
    if (cnt[kCntHash256]) { ScopedTimer t(ctx, "hash_cands_256", st); launch_hash_cands(kListHash256, r.b, r.tab, r.ws, r.K, r.taxkey, r.cands, st); }
    if (cnt[kCntHash512]) { ScopedTimer t(ctx, "hash_cands_512", st); launch_hash_cands(kListHash512, r.b, r.tab, r.ws, r.K, r.taxkey, r.cands, st); }
    if (cnt[kCntHash1024]) { ScopedTimer t(ctx, "hash_cands_1024", st); launch_hash_cands(kListHash1024, r.b, r.tab, r.ws, r.K, r.taxkey, r.cands, st); }
}

// reads beyond kGwSmallH locations (long reads): the stream filter takes them longest first (launch_gw_order) -- its scratch
static int ensure_stream_order(mc_ctx* ctx, Pipe& P, Workspace& ws, uint32_t n, hipStream_t st)
{
    size_t ordBytes = 0;
    if (launch_gw_order(kSideStream, ws, n, n, nullptr, ordBytes, st) != 0) return fail(ctx, MC_ERR_HIP, "ordering of the stream filter's reads: size query failed");
    if (const int rc = ensure(ctx, P.bOrder, (size_t)3 * std::max<uint32_t>(n, 1) * 4 + ordBytes + 256)) return rc;
    ws.orderScratch = (uint32_t*)P.bOrder.p; ws.orderTemp = ordBytes;
    return MC_OK;
}

// MC_DEFER_TAIL (large batches on the lane path): everything the host has to look at device counters for -- the sorted class of the
// filtered path, the segment sizes of the exact wave kernels' leftovers -- waits for mc_query_finish; the call returns with the main
// kernels enqueued and NO synchronisation, so that the caller can enqueue the next batch on the other pipe first
static int store_deferred_tail(mc_ctx* ctx, Pipe& P, const BatchRun& run, bool sortedPath)
{
    Pipe::Tail& tl = P.tail;
    if (const int rc = ensure_host_words(ctx, P)) return rc;
    if (!tl.mainDone) HIP_TRY(ctx, hipEventCreateWithFlags(&tl.mainDone, hipEventDisableTiming));
    tl.sortedPath = sortedPath;
    if (tl.sortedPath) HIP_TRY(ctx, hipMemcpyAsync(reinterpret_cast<uint32_t*>(P.hTotal + 9), run.ws.midCount + kCntSorted, 4, hipMemcpyDeviceToHost, run.st));
    HIP_TRY(ctx, hipEventRecord(tl.mainDone, run.st));
    tl.run = run;
    tl.pending = true;
    return MC_OK;
}

int mcamd::query_on_pipe(mc_ctx* ctx, Pipe& P, const mc_device_batch* in, int lowestRank, int flags, mc_device_results* out, void* streamv)
{
    const QueryWants w = query_wants(flags);
    if (!ctx->tableReady) return fail(ctx, MC_ERR_STATE, "no database loaded (every part needs mc_load_begin .. mc_load_end)");
    if (!in->max_win && in->max_win_uniform < 1) return fail(ctx, MC_ERR_INVALID, "max_win or max_win_uniform required");
    if (w.numbers && (ctx->parts.size() != 1 || !ctx->parts[0].compact || !ctx->dGwBase))
        return fail(ctx, MC_ERR_UNSUPPORTED, "MC_WANT_PARTIAL_NUMBERS: the database has no global window numbers (compact location store)");
    hipStream_t st = nullptr;
    int rc = enter_pipe(ctx, P, streamv, st);
    if (rc) return rc;
    const uint32_t n = in->num_queries;
    P.numbersN = 0xFFFFFFFFu;
    const SketchParams sp = ctx->querySketch;
    const uint32_t K = ctx->cfg.max_candidates;
    const uint32_t* taxkey = nullptr;
    if ((rc = taxkey_for_rank(ctx, lowestRank, &taxkey))) return rc;

    // the pipe's buffers that depend on the batch's size alone (size_pipe; mc_open_database reserves them beside the file load)
    const bool lanePath = lane_path_takes(lane_path_supported(sp), lane_candidates_supported(K), ctx->useLanePath, w);
    const Part& T = ctx->parts[0];
    uint64_t locs = 0;
    for (auto& p : ctx->parts) locs += p.locations;
    PipeSizes sz{};
    if ((rc = size_pipe(ctx, P, n, in->num_chars, w.features, lanePath, locs, T.keysStored, sz))) return rc;

    BatchRun run{tuned_workspace(ctx)};
    Workspace& ws = run.ws;
    bind_workspace(ws, P, ctx, lanePath);
    ws.features = (w.features || lanePath) ? (uint32_t*)P.bFeatures.p : nullptr;
    if (lanePath) {
        ws.partialLists = w.partial ? 1u : 0u;
        ws.bigPoolCap = (uint32_t)sz.poolCap; ws.bigOvfCap = (uint32_t)sz.ovfCap;
        ws.chunkList = w.noLongReads ? nullptr : (uint2*)P.bChunkList.p;   // (null: no read is cut into chunks, the chunk launchers launch nothing)
    }
    run.b = BatchView{in->seq, in->qinfo, in->max_win, in->max_win_uniform, n}; run.sp = sp; run.tab = table_view(ctx);
    run.K = K; run.taxkey = taxkey; run.cands = P.bCands.p; run.st = st; run.poolEntries = sz.poolCap + sz.ovfCap;
    run.compact = T.compact; run.fuse = wave_fuses_candidates(w, taxkey != nullptr);
    run.wantAllhits = w.allhits; run.wantPartial = w.partial; run.wantNumbers = w.numbers; run.lanePath = lanePath;

    const bool countersCleared = run_plan(ctx, run, lanePath ? ws.midCount : nullptr);
    TailPlan plan;                                               // (without the lane path: the wave kernels take every read)
    if (lanePath) {
        if (!countersCleared) HIP_TRY(ctx, hipMemsetAsync(ws.midCount, 0, kCounterBytes, st));
        const LaneStage stage = lane_stage(w, LaneSwitches{ctx->quadLookup, ctx->fuseLane, ctx->filterLookup, ctx->gwFuse, ctx->cfg.key_shard_count},
                                           LaneTable{T.nbuckets, (uint32_t)sizeof(TableBucket), T.compact, T.ddirect != nullptr}, BatchShape{n, in->max_win != nullptr, in->max_win_uniform});
        const bool filterLookup = stage.order == LaneOrder::FilterLookup;
        ws.filterLookup = filterLookup ? 1u : 0u;
        run_lane_stage(ctx, run, stage, sz.nfeat);
        HostCounters cnt = counters_unseen(w);
        if (host_looks(w, n, stage.order)) {
            if ((rc = ensure_host_words(ctx, P))) return rc;
            uint32_t* words = reinterpret_cast<uint32_t*>(P.hTotal + 1);
            launch_flag_count_host(ws, n, words, st);
            HIP_TRY(ctx, traced_sync(st));
            cnt = counters_seen(words);
        }
        if (!filterLookup) run_mid_and_hash(ctx, run, cnt);
        plan = tail_plan(w, T.compact, n, cnt);
        if (plan.waveFirst) {
            { ScopedTimer t(ctx, "query_wave", st); launch_query(run.b, sp, run.tab, run.fuse, false, ws, K, run.cands, st); }
            launch_wave_rejoin(run.b, sp, run.tab, ws, st);
        }
        if (plan.streamOrder && (rc = ensure_stream_order(ctx, P, ws, n, st))) return rc;
        if (plan.filtered) {
            if (filterLookup) { run_filter_step(ctx, run); run_mid_and_hash(ctx, run, cnt); }     // (the mid / hash kernels' lists are the LOOKUP instance's)
            if ((rc = run_filtered_path(ctx, P, run, plan.second, plan.deferSorted, filterLookup))) return rc;
        }
        run.skipWaveSketch = plan.waveFirst;                     // (the wave kernels' sketching and probing has run already)
    } else {
        HIP_TRY(ctx, hipMemsetD32Async((hipDeviceptr_t)ws.qflag, 1, n, st));     // every query: needs sketch + probe
    }
    if (plan.defer) rc = store_deferred_tail(ctx, P, run, plan.tailSortedPath);
    else if (plan.waveWork) rc = run_wave_tail(ctx, P, run, plan.sortedInTail);
    if (rc) return rc;
    HIP_TRY(ctx, hipGetLastError());
    P.lastN = n;
    publish_results(out, P, ws, w.allhits && !plan.defer);
    out->features = ws.features; out->win_offsets = ws.winOff;
    return MC_OK;
}

extern "C" {

int mc_query_device(mc_ctx* ctx, const mc_device_batch* in, int lowestRank, int flags, mc_device_results* out, void* streamv)
{
    if (!ctx || !in || !out) return MC_ERR_INVALID;
    flags &= ~mcamd::kQueryNoLongReads;                           // (internal: the caller of this entry point has not seen the reads)
    return query_on_pipe(ctx, (flags & MC_SECOND_PIPE) ? ctx->pipe1 : ctx->pipe0, in, lowestRank, flags, out, streamv);
}

int mc_query_finish(mc_ctx* ctx, int flags)
{
    if (!ctx) return MC_ERR_INVALID;
    return finish_on_pipe(ctx, (flags & MC_SECOND_PIPE) ? ctx->pipe1 : ctx->pipe0);
}

int mc_last_batch_stats(mc_ctx* ctx, uint64_t stats[8])
{
    if (!ctx) return MC_ERR_INVALID;
    std::memset(stats, 0, 64);
    Pipe& P = ctx->pipe0;
    hipStream_t st = nullptr;
    if (const int rc = enter_pipe(ctx, P, nullptr, st)) return rc;
    if (!P.bStats.p || !P.bQstat.p) return MC_OK;
    Workspace ws = tuned_workspace(ctx);
    bind_workspace(ws, P, ctx, P.bMid.p != nullptr);
    launch_batch_stats(ws, P.lastN, ctx->stream);
    HIP_TRY(ctx, hipMemcpyAsync(stats, ws.stats, 64, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return MC_OK;
}

uint32_t mc_key_owner(uint32_t feature, uint32_t shardCount) { return key_owner(feature, shardCount); }

int mc_candidates_from_hits(mc_ctx* ctx, const mc_device_hits* in, int lowestRank, mc_device_results* out, void* streamv)
{
    if (!ctx || !in || !out || !in->hit_offsets) return MC_ERR_INVALID;
    if (!in->max_win && in->max_win_uniform < 1) return fail(ctx, MC_ERR_INVALID, "max_win or max_win_uniform required");
    Pipe& P = ctx->pipe0;
    hipStream_t st = nullptr;
    int rc = enter_pipe(ctx, P, streamv, st);
    if (rc) return rc;
    const uint32_t n = in->num_queries;
    const uint32_t K = ctx->cfg.max_candidates;
    const uint32_t* taxkey = nullptr;
    if ((rc = taxkey_for_rank(ctx, lowestRank, &taxkey))) return rc;
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, in->hit_offsets + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, traced_sync(st));
    Workspace ws = tuned_workspace(ctx);
    if ((rc = ensure_sort_space(ctx, P, total, taxkey, ws))) return rc;
    if ((rc = ensure(ctx, P.bHitOff, (size_t)(n + 2) * 8)) || (rc = ensure(ctx, P.bQstat, (size_t)(n + 1) * sizeof(QueryStat))) ||
        (rc = ensure(ctx, P.bCands, (size_t)std::max<uint32_t>(n, 1) * K * sizeof(mc_candidate))))
        return rc;
    // the lists are sorted in place: work on a copy inside the context
    if (total) HIP_TRY(ctx, hipMemcpyAsync(P.bHits.p, in->hits, total * 8, hipMemcpyDeviceToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(P.bHitOff.p, in->hit_offsets, (size_t)(n + 1) * 8, hipMemcpyDeviceToDevice, st));
    ws.hitOff = (uint64_t*)P.bHitOff.p; ws.qstat = (QueryStat*)P.bQstat.p;
    BatchView b{nullptr, nullptr, in->max_win, in->max_win_uniform, n};
    DeviceTable tab = no_table();
    {
        ScopedTimer t(ctx, "cands_from_hits", st);
        launch_cands_from_hits(b, tab, ws, taxkey, K, P.bCands.p, st);
    }
    HIP_TRY(ctx, hipGetLastError());
    P.lastN = 0;
    publish_results(out, P, ws, true);
    return MC_OK;
}

// Mode K, owner side in one call: union of the sources' partial lists (device side, no host round trip), then rows 8-10 on it
int mc_candidates_from_partial_hits(mc_ctx* ctx, const mc_device_partial_hits* in, int lowestRank, mc_device_results* out, void* streamv)
{
    if (!ctx || !in || !out || !in->counts || (!in->hits && in->total_hits) || in->num_sources < 1) return MC_ERR_INVALID;
    if (!in->max_win && in->max_win_uniform < 1) return fail(ctx, MC_ERR_INVALID, "max_win or max_win_uniform required");
    Pipe& P = ctx->pipe0;
    hipStream_t st = nullptr;
    int rc = enter_pipe(ctx, P, streamv, st);
    if (rc) return rc;
    const uint32_t n = in->num_queries, S = in->num_sources;
    const uint32_t K = ctx->cfg.max_candidates;
    const uint32_t* taxkey = nullptr;
    if ((rc = taxkey_for_rank(ctx, lowestRank, &taxkey))) return rc;
    Workspace ws = tuned_workspace(ctx);
    if ((rc = ensure_sort_space(ctx, P, in->total_hits, taxkey, ws))) return rc;
    if ((rc = ensure(ctx, P.bHitOff, (size_t)(n + 2) * 8)) || (rc = ensure(ctx, P.bQstat, (size_t)(n + 1) * sizeof(QueryStat))) ||
        (rc = ensure(ctx, P.bCands, (size_t)std::max<uint32_t>(n, 1) * K * sizeof(mc_candidate))) ||
        (rc = ensure(ctx, P.bScanIn, (size_t)(n + 1) * 4)) || (rc = ensure(ctx, P.bScan, scan_tmp_bytes(n + 1))) ||
        (rc = ensure(ctx, P.bPpay, ((size_t)S * (n + 2) + n + 1) * 8)) || (rc = ensure(ctx, P.bPsize, (size_t)(n + 1) * 4)) ||
        (rc = ensure(ctx, P.bWinOff, (size_t)(n + 2) * 4)) || (rc = ensure(ctx, P.bWinCount, (size_t)(n + 1) * 4)) ||
        (rc = ensure(ctx, P.bQflag, (size_t)(n + 1) * 4)) || (rc = ensure(ctx, P.bMid, work_lists_bytes(n))))
        return rc;
    const uint64_t poolCap = owner_lists_pool(n, big_filter_grid(n, false, ctx->filterBpc)).poolCap;
    if ((rc = ensure(ctx, P.bBigPool, poolCap * 8))) return rc;
    // srcStart (union) and the one-entry-per-read tables of the filtered path share bPpay: [S * (n + 2)] u64 | [n] u64
    uint64_t* srcStart = (uint64_t*)P.bPpay.p;
    launch_union_partial(in->counts, S, n, reinterpret_cast<const uint64_t*>(in->hits), (uint32_t*)P.bScanIn.p, srcStart, (uint64_t*)P.bHitOff.p,
                         (uint64_t*)P.bHits.p, P.bScan.p, st);
    ws.hitOff = (uint64_t*)P.bHitOff.p; ws.qstat = (QueryStat*)P.bQstat.p;
    BatchView b{nullptr, nullptr, in->max_win, in->max_win_uniform, n};
    // Long united lists (RefSeq scale: 1 300 locations per read) take the filtered path of the replicated mode instead of a sort: the union
    // buffer stands in for the table's location store, a read's whole list is ONE entry of it (rounds of 16 / 64 locations); what the
    // filter cannot take (more than 16 384 locations, wide window ranges) and what it hands back goes through the sort as before.
    const bool filtered = lane_candidates_supported(K) && ctx->useLanePath;
    if (filtered) {
        bind_workspace(ws, P, ctx, true);
        ws.bigPoolCap = (uint32_t)poolCap;
        ws.ppay = srcStart + (size_t)S * (n + 2);                              // (behind the union's srcStart in bPpay)
        ws.hitScan = (uint32_t*)P.bWinCount.p;                                 // (bScanIn holds the union's counts)
        ws.sliceFill = nullptr; ws.sideList = nullptr;                         // (one filter instance, no compact store's side tables: neither buffer is made here)
        HIP_TRY(ctx, hipMemsetAsync(ws.midCount, 0, kCounterBytes, st));
        launch_owner_classify(b, ws, std::max<uint32_t>(ctx->bigMin, 256u), st);
        DeviceTable utab{nullptr, ws.hits, 0, 0xFFFFFFFFu, 1};
        const SketchParams one = one_entry_per_read();
        { ScopedTimer t(ctx, "big_filter", st); launch_big_cands(FilterStep::Filter, b, one, utab, ws, K, taxkey, P.bCands.p, st); }
        { ScopedTimer t(ctx, "big_count", st); launch_big_cands(FilterStep::Count, b, one, utab, ws, K, taxkey, P.bCands.p, st); }
        { ScopedTimer t(ctx, "big_count_2", st); launch_big_cands(FilterStep::Count1024, b, one, utab, ws, K, taxkey, P.bCands.p, st); }
    }
    DeviceTable tab = no_table();
    {
        ScopedTimer t(ctx, "cands_from_hits", st);
        launch_cands_from_hits(b, tab, ws, taxkey, K, P.bCands.p, st);
    }
    HIP_TRY(ctx, hipGetLastError());
    P.lastN = 0;
    publish_results(out, P, ws, true);
    return MC_OK;
}

// ---- Mode K with 4-byte locations on the wire (keyshard.hip) --------------------------------------------------------------------------
// shard side: the partial lists of the last mc_query_device(MC_WANT_PARTIAL_HITS) call as global window numbers + per-read counts
int mc_partial_numbers(mc_ctx* ctx, const mc_device_results* res, uint32_t n, const uint32_t* cutQueries, uint32_t numCuts, uint64_t* cutOffsets,
                       mc_device_partial_numbers* out, void* streamv)
{
    if (!ctx || !res || !out || (numCuts && (!cutQueries || !cutOffsets))) return MC_ERR_INVALID;
    if (!res->hit_offsets) return fail(ctx, MC_ERR_STATE, "mc_partial_numbers: the results hold no location lists (MC_WANT_PARTIAL_HITS)");
    if (ctx->parts.size() != 1 || !ctx->parts[0].compact || !ctx->dGwBase)
        return fail(ctx, MC_ERR_UNSUPPORTED, "mc_partial_numbers: the database has no global window numbers (compact location store)");
    // (the pipe whose batch these results are: a caller with two batches in flight -- keyset.cpp's lanes -- runs the shards' lookups on either)
    Pipe& P = (ctx->pipe1.bHitOff.p && res->hit_offsets == (const uint64_t*)ctx->pipe1.bHitOff.p) ? ctx->pipe1 : ctx->pipe0;
    hipStream_t st = nullptr;
    int rc = enter_pipe(ctx, P, streamv, st);
    if (rc) return rc;
    for (uint32_t i = 0; i < numCuts; ++i) {
        if (cutQueries[i] > n) return fail(ctx, MC_ERR_INVALID, "mc_partial_numbers: cut beyond the batch");
        HIP_TRY(ctx, hipMemcpyAsync(&cutOffsets[i], res->hit_offsets + cutQueries[i], 8, hipMemcpyDeviceToHost, st));
    }
    uint64_t total = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&total, res->hit_offsets + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, traced_sync(st));                    // the one host round trip of the exchange: its split sizes
    if (P.numbersN == n && P.numbersTotal == total && res->hit_offsets == (const uint64_t*)P.bHitOff.p) {
        // mc_query_device(MC_WANT_PARTIAL_NUMBERS) left the numbers and the counts where they belong
    } else {
        if ((rc = ensure(ctx, P.bNumbers, (size_t)(total + 8) * 4)) || (rc = ensure(ctx, P.bCounts, (size_t)(n + 1) * 4))) return rc;
        DeviceTable tab = no_table();
        set_window_numbering(ctx, tab);
        {
            ScopedTimer t(ctx, "pack_numbers", st);
            launch_pack_numbers(reinterpret_cast<const uint64_t*>(res->hits), res->hit_offsets, total, n, tab, (uint32_t*)P.bNumbers.p, (uint32_t*)P.bCounts.p, st);
        }
        HIP_TRY(ctx, hipGetLastError());
    }
    out->counts = (const uint32_t*)P.bCounts.p;
    out->numbers = (const uint32_t*)P.bNumbers.p;
    out->total = total;
    return MC_OK;
}

// owner side: rows 8-10 on the pieces the key shards sent for this rank's reads, where they lie in the receive buffer
int mc_candidates_from_partial_numbers(mc_ctx* ctx, const mc_device_partial_numbers_in* in, int lowestRank, mc_device_results* out, void* streamv)
{
    return mc_candidates_from_partial_numbers_on(ctx, in, lowestRank, 0, out, streamv);
}

int mc_candidates_from_partial_numbers_on(mc_ctx* ctx, const mc_device_partial_numbers_in* in, int lowestRank, int flags, mc_device_results* out, void* streamv)
{
    if (!ctx || !in || !out || !in->counts || !in->source_offsets || in->num_sources < 1 || in->num_sources > 64) return MC_ERR_INVALID;
    if (!in->max_win && in->max_win_uniform < 1) return fail(ctx, MC_ERR_INVALID, "max_win or max_win_uniform required");
    if (ctx->parts.size() != 1 || !ctx->parts[0].compact || !ctx->dGwBase)
        return fail(ctx, MC_ERR_UNSUPPORTED, "mc_candidates_from_partial_numbers: the database has no global window numbers (compact location store)");
    const uint32_t n = in->num_queries, S = in->num_sources;
    const uint32_t K = ctx->cfg.max_candidates;
    if (!lane_candidates_supported(K)) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_candidates_from_partial_numbers: max_candidates above 4");
    if ((uint64_t)n * S > 0xFFFFFFF0ull) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_candidates_from_partial_numbers: batch too large");
    const uint64_t totalIn = in->source_offsets[S];
    if (totalIn && !in->numbers) return MC_ERR_INVALID;
    Pipe& P = (flags & MC_SECOND_PIPE) ? ctx->pipe1 : ctx->pipe0;
    hipStream_t st = nullptr;
    int rc = enter_pipe(ctx, P, streamv, st);
    if (rc) return rc;
    const uint32_t* taxkey = nullptr;
    if ((rc = taxkey_for_rank(ctx, lowestRank, &taxkey))) return rc;
    const uint32_t grid = big_filter_grid(n, true, ctx->filterBpc);
    const PoolSizes pool = owner_numbers_pool(n, totalIn, grid);
    const uint64_t poolCap = pool.poolCap, ovfCap = pool.ovfCap;
    if ((rc = ensure(ctx, P.bPsize, ((size_t)n * S + 4) * 4)) || (rc = ensure(ctx, P.bPpay, ((size_t)n * S + (size_t)S * (n + 2) + 4) * 8)) ||
        (rc = ensure(ctx, P.bQstat, (size_t)(n + 1) * sizeof(QueryStat))) || (rc = ensure(ctx, P.bQflag, (size_t)(n + 1) * 4)) ||
        (rc = ensure(ctx, P.bScanIn, (size_t)(n + 1) * 4)) || (rc = ensure(ctx, P.bScan, scan_tmp_bytes(n + 1))) ||
        (rc = ensure(ctx, P.bHitOff, (size_t)(n + 2) * 8)) || (rc = ensure(ctx, P.bMid, work_lists_bytes(n))) ||
        (rc = ensure(ctx, P.bBigPool, (poolCap + ovfCap) * 4)) || (rc = ensure(ctx, P.bSliceFill, (size_t)grid * 4 * 4 + 64)) ||
        (rc = ensure(ctx, P.bSide, (size_t)kSideRows * std::max<uint32_t>(n, 1) * 4)) ||
        (rc = ensure(ctx, P.bCands, (size_t)std::max<uint32_t>(n, 1) * K * sizeof(mc_candidate))))
        return rc;
    BatchRun run{tuned_workspace(ctx)};
    Workspace& ws = run.ws;
    bind_workspace(ws, P, ctx, true);
    ws.bigPoolCap = (uint32_t)poolCap; ws.bigOvfCap = (uint32_t)ovfCap;
    uint64_t* srcStart = ws.ppay + (size_t)n * S + 2;                 // [S][n + 1] exclusive scans of the sources' counts
    BatchView b{nullptr, nullptr, in->max_win, in->max_win_uniform, n};
    // the receive buffer stands in for the table's location store
    DeviceTable tab = no_table();
    tab.values32 = in->numbers;
    set_window_numbering(ctx, tab);
    KeyshardBases bases{};
    for (uint32_t s = 0; s < S; ++s) bases.b[s] = in->source_offsets[s];
    HIP_TRY(ctx, hipMemsetAsync(ws.midCount, 0, kCounterBytes, st));
    {
        ScopedTimer t(ctx, "owner_entries", st);
        for (uint32_t s = 0; s < S; ++s) launch_scan_u32(in->counts + (size_t)s * n, 1, n, nullptr, srcStart + (size_t)s * (n + 1), ws.scanTmp, st);
        launch_owner_entries(b, tab, ws, in->counts, srcStart, bases, S, st);
    }
    run.b = b; run.sp = one_entry_per_read(); run.tab = tab; run.K = K; run.taxkey = taxkey; run.cands = P.bCands.p; run.st = st;
    run.poolEntries = poolCap + ovfCap; run.compact = true;
    if ((rc = run_filtered_path(ctx, P, run, true))) return rc;
    // what is left (short lists, reads the filtered path handed back): decoded to (target, window) lists and sorted
    launch_scan_u32(ws.hitScan, 1, n, nullptr, ws.hitOff, ws.scanTmp, st);
    if ((rc = ensure_host_words(ctx, P))) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(P.hTotal, ws.hitOff + n, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(P.hTotal + 10, ws.midCount + kCntFilter, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, traced_sync(st));
    ctx->ownerStats[0] += n; ctx->ownerStats[1] += *reinterpret_cast<const uint32_t*>(P.hTotal + 10); ctx->ownerStats[2] += totalIn; ctx->ownerStats[3] += *P.hTotal;
    if ((rc = ensure_sort_space(ctx, P, *P.hTotal, taxkey, ws))) return rc;
    { ScopedTimer t(ctx, "decode_union", st); launch_decode_union(b, tab, ws, in->counts, srcStart, bases, S, st); }
    const DeviceTable none = no_table();
    // (owner_entries_kernel wrote every read's statistics: locations and sources whichever kernel finishes the read, a read beyond kMaxHitsPerQuery included)
    { ScopedTimer t(ctx, "cands_from_hits", st); launch_cands_from_hits(b, none, ws, taxkey, K, P.bCands.p, st, true); }
    HIP_TRY(ctx, hipGetLastError());
    P.lastN = 0;
    publish_results(out, P, ws, false);
    return MC_OK;
}

int mc_owner_stats(const mc_ctx* ctx, uint64_t stats[4])
{
    if (!ctx || !stats) return MC_ERR_INVALID;
    for (int i = 0; i < 4; ++i) stats[i] = ctx->ownerStats[i];
    return MC_OK;
}

// Mode P / part groups: per-part candidate lists of the same reads (device pointers, [n][max_candidates] each, in part order) -> one list
// per read, as if the parts had been queried one after the other with one candidate list (candidate_generation.hpp:172-231).  Target ids
// must be the database's own (mc_open_database with single_part keeps them), lowest_rank > 0 uses this context's lineages.
int mc_merge_part_candidates(mc_ctx* ctx, const mc_candidate* const* lists, uint32_t numLists, uint32_t n, int lowestRank, mc_candidate* out, void* streamv)
{
    if (!ctx || !lists || !out || numLists == 0) return MC_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = streamv ? (hipStream_t)streamv : ctx->stream;
    const uint32_t* taxkey = nullptr;
    int rc = taxkey_for_rank(ctx, lowestRank, &taxkey);
    if (rc) return rc;
    const uint32_t K = ctx->cfg.max_candidates;
    // more than 16 lists: in rounds, the merged list of a round leads the next one (the insert is sequential anyway)
    const void* ptrs[16];
    uint32_t done = 0;
    bool lead = false;
    while (done < numLists) {
        uint32_t m = 0;
        if (lead) ptrs[m++] = out;
        while (m < 16 && done < numLists) ptrs[m++] = lists[done++];
        if (launch_merge_parts(ptrs, m, n, K, taxkey, out, st) != 0) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_merge_part_candidates: max_candidates above 4");
        lead = true;
    }
    HIP_TRY(ctx, hipGetLastError());
    return MC_OK;
}

}  // extern "C"
