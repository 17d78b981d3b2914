// metacache_amd/csrc/table_load.cpp -- everything that BUILDS a context's query table: mc_load_*, the chunk routine behind it, the builder
// (builder.hip) and the file loader (dbload.cpp).  One part: on the device, batch by batch (table_build.hip); several: merged on the host (table_rules.h).
#include "context.h"
#include "devcache.h"

#include <algorithm>
#include <cstdlib>

using namespace mcamd;

// The loader knows what the lists would take with every list on a line of its own (table_rules.h list_alloc): alignment is switched on
// where that is wanted ("list_align"), the table has the compact store, and the padded store is affordable.  Before the first chunk.
void mcamd::announce_store(mc_ctx* ctx, uint64_t paddedEntries)
{
    Part& T = ctx->parts[0];
    if (T.dvalues || !T.compact || ctx->listAlignWant == 0 || paddedEntries == 0) return;
    const uint64_t plain = T.dvaluesCap;
    if (ctx->listAlignWant != 1 && paddedEntries > plain + plain / 2 + (1u << 20)) return;
    // Decision and allocation are ONE step per process: several loads run side by side on a device (a part group loads two parts at a
    // time while the previous group is still resident), and each would judge the padded store affordable against the same free memory.
    // A padded store that cannot be had is not an error -- the table falls back to the plain one.
    static std::mutex decide;
    std::lock_guard<std::mutex> lk(decide);
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return;
    // (inside a part group the other parts of the group still have to fit: only the padding beyond the plain store counts against a
    // share of what is free: listAlignShare, 1 outside part sets -- partset.cpp sets it through open_hints)
    const uint64_t extra = paddedEntries > plain ? (paddedEntries - plain) * 4 : 0;
    const bool affordable = (paddedEntries + 4) * 4 + (4ull << 30) < freeB && extra <= (uint64_t)((double)freeB * ctx->listAlignShare);
    if (!affordable) return;
    void* p = nullptr;
    if (big_malloc(&p, (paddedEntries + 1 + 4) * sizeof(uint32_t)) != hipSuccess) { (void)hipGetLastError(); return; }
    T.dvalues = reinterpret_cast<uint64_t*>(p);
    T.listAlign = kListAlign; T.expectStore = paddedEntries; T.dvaluesCap = paddedEntries + 1;
    ctx->storesPlaced.fetch_add(1, std::memory_order_release);
}

// buckets for `nkeys` keys at a load factor: an even number, two buckets per line; 0: more than a 32-bit bucket index reaches
static uint32_t bucket_count(uint64_t nkeys, double loadFactor)
{
    uint64_t nb = (uint64_t)((double)nkeys / (kSlotsPerBucket * loadFactor)) + 2;
    nb += nb & 1;
    return nb > 0xFFFFFFF0ull ? 0u : (uint32_t)nb;
}
static const char* const kTooManyBuckets = "table too large for 32-bit bucket index";

// the bucket table of a single-part context whose mc_load_begin left it open (Mode T), for `nkeys` keys at the context's load factor;
// nkeys = 0: for all keys the part announced
// (big_malloc: the tables of a part group come back from the tables of the group before it, devcache.h)
int mcamd::allocate_buckets(mc_ctx* ctx, uint64_t nkeys)
{
    Part& T = ctx->parts[0];
    if (T.dbuckets) return MC_OK;
    if (nkeys == 0 || nkeys > T.expectKeys) nkeys = T.expectKeys;
    const uint32_t nb = bucket_count(nkeys, ctx->loadFactor);
    if (!nb) return fail(ctx, MC_ERR_UNSUPPORTED, kTooManyBuckets);
    T.nbuckets = nb;
    HIP_TRY(ctx, big_malloc((void**)&T.dbuckets, (size_t)nb * sizeof(TableBucket)));
    HIP_TRY(ctx, hipMemsetAsync(T.dbuckets, 0, (size_t)nb * sizeof(TableBucket), ctx->stream));
    return MC_OK;
}
// the location store, with the first chunk that is loaded
int mcamd::allocate_values(mc_ctx* ctx)
{
    Part& T = ctx->parts[0];
    if (T.dvalues) return MC_OK;
    // (+ 4 entries: the filter reads the compact lists 16 bytes at a time, a list's last load may reach 3 entries past its end)
    HIP_TRY(ctx, big_malloc((void**)&T.dvalues, (T.dvaluesCap + 4) * (T.compact ? sizeof(uint32_t) : sizeof(uint64_t))));
    ctx->storesPlaced.fetch_add(1, std::memory_order_release);
    return MC_OK;
}

// ---- one chunk of a single-part database whose batch arrays are already in device memory (keys u32 | sizes u8 | packed values), in two
// steps that only ENQUEUE on the context's stream.  bLdCounters: [0] keys stored, [1] locations kept, [2] (as two u32) longest probe
// sequence | table-full flag, [3] a location outside the announced range.  The scratch arrays are reused chunk after chunk: the
// stream's order protects them.  fromFile: the pipelined loader's chunks, which have their own words (and MC_ERR_NOMEM) for a failure.
static int grow_scratch(mc_ctx* ctx, DevBuf& b, size_t bytes)
{
    // (growing a scratch array the stream may still be reading: drain it first -- happens a few times per load, the sizes settle at once)
    if (bytes > b.cap && b.p) (void)hipStreamSynchronize(ctx->stream);
    return ensure(ctx, b, bytes);
}
static LoadFilter load_filter(const mc_ctx* ctx) { return LoadFilter{ctx->cfg.max_locations_per_feature, ctx->cfg.remove_overpopulated, ctx->cfg.key_shard_index, ctx->cfg.key_shard_count, ctx->parts[0].listAlign}; }
// checks, bucket table, scratch; per key its file size and what it takes in the store (table_prep), and both running sums:
// bLdStoreOff[nb] = what the chunk adds to the location store
static int chunk_prepare(mc_ctx* ctx, const uint32_t* dkeys, const uint8_t* dsizes, uint32_t nb, uint64_t fileVals, bool fromFile)
{
    Part& P = ctx->parts[0];
    if (P.keysLoaded + nb > P.expectKeys) return fail(ctx, MC_ERR_INVALID, fromFile ? "database file: more keys than its header announces" : "mc_load_batch: more keys than announced");
    if (fileVals >= (1ull << 32)) return fail(ctx, MC_ERR_INVALID, fromFile ? "database file: a chunk holds 2^32 or more locations" : "load_chunk_device: chunk too large");
    if (int rc = allocate_buckets(ctx, 0)) return fromFile ? MC_ERR_NOMEM : rc;
    int rc = 0;
    if ((rc = grow_scratch(ctx, ctx->bLdFileSz, (size_t)nb * 4)) || (rc = grow_scratch(ctx, ctx->bLdStoreSz, (size_t)nb * 4)) ||
        (rc = grow_scratch(ctx, ctx->bLdFileOff, (size_t)(nb + 2) * 4)) || (rc = grow_scratch(ctx, ctx->bLdStoreOff, (size_t)(nb + 2) * 4)) ||
        (rc = grow_scratch(ctx, ctx->bLdScan, scan_tmp_bytes(nb + 1))))
        return fromFile ? fail(ctx, MC_ERR_NOMEM, "database load: cannot allocate the table-build scratch") : rc;
    auto* fileSz = (uint32_t*)ctx->bLdFileSz.p; auto* storeSz = (uint32_t*)ctx->bLdStoreSz.p;
    launch_table_prep(dkeys, dsizes, nb, load_filter(ctx), fileSz, storeSz, (unsigned long long*)ctx->bLdCounters.p, ctx->stream);
    launch_scan_u32(fileSz, 1, nb, (uint32_t*)ctx->bLdFileOff.p, nullptr, ctx->bLdScan.p, ctx->stream);
    launch_scan_u32(storeSz, 1, nb, (uint32_t*)ctx->bLdStoreOff.p, nullptr, ctx->bLdScan.p, ctx->stream);
    return MC_OK;
}
// location store, room for `stored` more entries; slots claimed (table_insert), the lists copied (table_values, plain or compact)
static int chunk_insert(mc_ctx* ctx, const uint32_t* dkeys, const uint8_t* dsizes, const uint8_t* dvals, uint32_t nb, uint64_t fileVals, uint64_t stored, bool fromFile)
{
    Part& P = ctx->parts[0];
    if (int rc = allocate_values(ctx)) return fromFile ? fail(ctx, MC_ERR_NOMEM, "database load: cannot allocate the location store") : rc;
    if (P.valuesStored + stored > P.dvaluesCap) return fail(ctx, MC_ERR_INVALID, fromFile ? "database file: more values than its header announces" : "mc_load_batch: more values than announced");
    const uint32_t tb = ctx->cfg.target_id_bytes;
    const LoadFilter lf = load_filter(ctx);
    auto* fileOff = (const uint32_t*)ctx->bLdFileOff.p; auto* storeOff = (const uint32_t*)ctx->bLdStoreOff.p;
    auto* flags = (unsigned int*)((unsigned long long*)ctx->bLdCounters.p + 2);   // [0] longest probe, [1] table full, [2] range error
    const GwLayout gwl = P.compact ? GwLayout{ctx->dGwBase, ctx->gwTargets, ctx->gwGap} : GwLayout{};
    launch_table_insert(dkeys, dsizes, nb, lf, fileOff, storeOff, dvals, tb, P.valuesStored, P.dbuckets, P.nbuckets, flags, flags + 1, ctx->stream, gwl, flags + 2);
    if (P.compact)
        launch_table_values_compact(dkeys, dsizes, nb, lf, fileOff, storeOff, dvals, tb, fileVals, reinterpret_cast<uint32_t*>(P.dvalues) + P.valuesStored,
                                    gwl, flags + 2, ctx->stream);
    else
        launch_table_values(dkeys, dsizes, nb, lf, fileOff, storeOff, dvals, tb, fileVals, P.dvalues + P.valuesStored, ctx->stream);
    if (fromFile && hipGetLastError() != hipSuccess) return fail(ctx, MC_ERR_HIP, "database load: a table-build kernel failed to launch");
    HIP_TRY(ctx, hipGetLastError());
    P.valuesStored += stored;
    P.keysLoaded += nb;
    return MC_OK;
}

// mc_load_batch after its upload, and the builder directly: what the chunk adds to the store is read back from the device (the one
// round trip), and the call returns when the chunk is in -- the caller's staging buffers are free again
int mcamd::load_chunk_device(mc_ctx* ctx, const uint32_t* dkeys, const uint8_t* dsizes, const uint8_t* dvals, uint32_t nb, uint64_t fileVals)
{
    if (!ctx || ctx->parts.size() != 1 || !ctx->parts[0].loading) return fail(ctx, MC_ERR_STATE, "load_chunk_device: single-part load only");
    if (int rc = chunk_prepare(ctx, dkeys, dsizes, nb, fileVals, false)) return rc;
    uint32_t stored = 0;
    HIP_TRY(ctx, hipMemcpyAsync(&stored, (const uint32_t*)ctx->bLdStoreOff.p + nb, 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, traced_sync(ctx->stream));
    if (int rc = chunk_insert(ctx, dkeys, dsizes, dvals, nb, fileVals, stored, false)) return rc;
    HIP_TRY(ctx, traced_sync(ctx->stream));
    return MC_OK;
}

// The pipelined loader's chunks (<= 2^22 keys, < 2^32 file values) WITHOUT any synchronisation -- its overlap of reads, copies and
// kernels rests on that: `stored` comes from the host, a pure function of the chunk's keys and sizes (dbload.cpp)
int mcamd::load_chunk_device_async(mc_ctx* ctx, const uint32_t* dkeys, const uint8_t* dsizes, const uint8_t* dvals, uint32_t nb, uint64_t fileVals, uint64_t stored)
{
    if (int rc = chunk_prepare(ctx, dkeys, dsizes, nb, fileVals, true)) return rc;
    return chunk_insert(ctx, dkeys, dsizes, dvals, nb, fileVals, stored, true);
}

static int allocate_table(mc_ctx* ctx)
{
    Part& T = ctx->parts[0];
    uint64_t nkeys = 0, nvalues = 0;
    for (auto& p : ctx->parts) { nkeys += p.expectKeys; nvalues += p.expectValues; }
    if (ctx->cfg.key_shard_count > 1) {
        // Mode K: this context keeps ~1/count of the keys (hashed: near uniform) and of the locations (lumpier: wider margin;
        // running out fails loudly in load_chunk_device)
        if (ctx->parts.size() > 1) return fail(ctx, MC_ERR_UNSUPPORTED, "key sharding needs a single-part database");
        const uint64_t c = ctx->cfg.key_shard_count;
        nkeys = std::min<uint64_t>(nkeys, nkeys / c + nkeys / (8 * c) + 4096);
        nvalues = std::min<uint64_t>(nvalues, nvalues / c + nvalues / (3 * c) + (1u << 16));
    }
    const uint32_t nb = bucket_count(nkeys, ctx->loadFactor);
    if (!nb) return fail(ctx, MC_ERR_UNSUPPORTED, kTooManyBuckets);
    T.nbuckets = nb;
    if (ctx->parts.size() > 1) { T.hbuckets.assign((size_t)nb, TableBucket{}); return MC_OK; }   // merged on the host
    T.dvaluesCap = nvalues + 1; T.compact = false;
    if (!ctx->targetWindows.empty() && ctx->compactAllowed) {
        // global window numbers: gwBase[0] = gap, gwBase[t + 1] = gwBase[t] + windows(t) + gap; 0xFFFFFFFF stays free (the kernels' "no location")
        uint32_t gap = kGwGap;
        if (const char* e = std::getenv("MC_GW_GAP")) gap = (uint32_t)std::max(8, std::atoi(e));   // tests: reads whose window range exceeds the gap
        const size_t nt = ctx->targetWindows.size();
        uint64_t total = gap;
        for (uint32_t w : ctx->targetWindows) total += (uint64_t)w + gap;
        if (total < 0xFFFFFFFFull) {
            std::vector<uint32_t> base(nt + 1);
            base[0] = gap;
            for (size_t t = 0; t < nt; ++t) base[t + 1] = base[t] + ctx->targetWindows[t] + gap;
            uint32_t shift = 6;
            while (((total >> shift) + 2) > (1ull << 22)) ++shift;            // directory of at most 4 M entries
            const size_t nd = (size_t)(total >> shift) + 2;
            std::vector<uint32_t> dir(nd);
            size_t t = 0;
            for (size_t blk = 0; blk < nd; ++blk) {                            // dir[blk] = target whose numbers (gap included) hold max(blk << shift, gap)
                const uint64_t g = std::max<uint64_t>((uint64_t)blk << shift, gap);
                while (t + 1 < nt && g >= base[t + 1]) ++t;
                dir[blk] = (uint32_t)t;
            }
            HIP_TRY(ctx, hipMalloc((void**)&ctx->dGwBase, (nt + 1) * 4));
            HIP_TRY(ctx, hipMalloc((void**)&ctx->dGwDir, nd * 4));
            HIP_TRY(ctx, hipMemcpy(ctx->dGwBase, base.data(), (nt + 1) * 4, hipMemcpyHostToDevice));
            HIP_TRY(ctx, hipMemcpy(ctx->dGwDir, dir.data(), nd * 4, hipMemcpyHostToDevice));
            ctx->gwDirShift = shift; ctx->gwGap = gap; ctx->gwTargets = (uint32_t)nt; ctx->gwBits = bits_for((uint32_t)total);
            T.compact = true;
        }
    }
    // (the location store is allocated with the first chunk -- allocate_values: a loader that knows the lists' sizes announces the
    // padded total first, announce_store)
    // (Mode T: the buckets wait for the loader's estimate of the keys that have a location in the range: it calls allocate_buckets)
    if (ctx->cfg.target_shard_count <= 1) { if (int rc = allocate_buckets(ctx, nkeys)) return rc; }
    if (int rc = ensure(ctx, ctx->bLdCounters, 4 * sizeof(unsigned long long))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(ctx->bLdCounters.p, 0, 4 * sizeof(unsigned long long), ctx->stream));
    return MC_OK;
}

// One batch of the file (host memory): upload in chunks, insert on the device.
static int load_batch_device(mc_ctx* ctx, const uint32_t* keys, const uint8_t* sizes, const uint8_t* values, uint64_t n)
{
    const uint32_t vb = 4 + ctx->cfg.target_id_bytes;
    hipStream_t st = ctx->stream;
    const uint64_t kChunk = 1ull << 22;                       // keys per launch: file values of a chunk stay below 2^32
    for (uint64_t done = 0; done < n;) {
        const uint32_t nb = (uint32_t)std::min<uint64_t>(kChunk, n - done);
        uint64_t fileVals = 0;
        for (uint32_t i = 0; i < nb; ++i) fileVals += sizes[done + i];
        int rc = 0;
        if ((rc = ensure(ctx, ctx->bLdKeys, (size_t)nb * 4)) || (rc = ensure(ctx, ctx->bLdSizes, nb)) ||
            (rc = ensure(ctx, ctx->bLdVals, fileVals * vb + 16)))
            return rc;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bLdKeys.p, keys + done, (size_t)nb * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(ctx->bLdSizes.p, sizes + done, nb, hipMemcpyHostToDevice, st));
        if (fileVals) HIP_TRY(ctx, hipMemcpyAsync(ctx->bLdVals.p, values, fileVals * vb, hipMemcpyHostToDevice, st));
        rc = load_chunk_device(ctx, (const uint32_t*)ctx->bLdKeys.p, (const uint8_t*)ctx->bLdSizes.p, (const uint8_t*)ctx->bLdVals.p, nb, fileVals);
        if (rc) return rc;
        values += fileVals * vb;
        done += nb;
    }
    return MC_OK;
}

// The direct-address index of a finished single-part table (kernels.h DeviceTable::direct): 2^32 entries of 8 bytes = 32 GiB beside the
// buckets.  Built where the lookups are bound by random requests -- bucket tables of 8 GiB and more -- and the device has the room
// (the index, and 40 GB more for the batches' workspaces); "direct_index" 1 / MC_DIRECT_INDEX=1 asks for it whatever the table's
// size, 0 never.  A payload that does not fit its 48 bits (targets or windows beyond 2^24 in a single location) drops it again.
int mcamd::build_direct_index(mc_ctx* ctx)
{
    Part& T = ctx->parts[0];
    if (T.ddirect || !T.dbuckets || ctx->directWant == 0) return MC_OK;
    if (ctx->directWant < 0 && (uint64_t)T.nbuckets * sizeof(TableBucket) < (8ull << 30)) return MC_OK;
    const size_t bytes = kDirectEntries * 8;
    size_t freeB = 0, totalB = 0;
    if (hipMemGetInfo(&freeB, &totalB) != hipSuccess) return MC_OK;
    if (freeB < bytes + (ctx->directWant > 0 ? (4ull << 30) : (40ull << 30))) return MC_OK;
    void* p = nullptr;
    if (big_malloc(&p, bytes) != hipSuccess) { (void)hipGetLastError(); return MC_OK; }
    unsigned int* dflag = nullptr;
    unsigned int flag = 1;
    hipStream_t st = ctx->stream;
    if (hipMalloc((void**)&dflag, 4) == hipSuccess && hipMemsetAsync(dflag, 0, 4, st) == hipSuccess && hipMemsetAsync(p, 0, bytes, st) == hipSuccess) {
        launch_direct_index(T.dbuckets, T.nbuckets, (uint64_t*)p, dflag, st);
        if (hipMemcpyAsync(&flag, dflag, 4, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) flag = 1;
    }
    if (dflag) (void)hipFree(dflag);
    if (flag) { (void)hipGetLastError(); (void)big_free(p); return MC_OK; }
    T.ddirect = (uint64_t*)p;
    return MC_OK;
}

// A table that came through mc_load_* (not mc_open_database, whose loader reserves beside the file load): the slot pipes' workspaces are
// sized now, once, for full (united) batches.  Left to the first batches every pipe grew its ~25 buffers batch by batch -- a hipFree (which waits
// for the whole device) and a hipMalloc each: the first seconds of 32 threads on a fresh context ran at 3-100 Mreads/min instead of 5 000.
// (A failure here is not one: the first batch asks again.)
static void reserve_pipes_after_load(mc_ctx* ctx)
{
    if (ctx->pipes.empty() || ctx->reserveByLoader.load(std::memory_order_acquire) || std::getenv("MC_NO_RESERVE")) return;
    uint64_t locs = 0;
    for (auto& p : ctx->parts) locs += p.locations;
    std::string keep = ctx->err;
    (void)mcamd::reserve_slot_pipes(ctx, locs, ctx->parts[0].keysStored, false);
    (void)hipGetLastError();
    ctx->err = keep;
}

extern "C" {

int mc_load_target_windows(mc_ctx* ctx, const uint32_t* windows, uint64_t numTargets)
{
    if (!ctx || (!windows && numTargets)) return MC_ERR_INVALID;
    for (auto& p : ctx->parts) if (p.announced) return fail(ctx, MC_ERR_STATE, "mc_load_target_windows: call it before mc_load_begin");
    if (numTargets >= 0xFFFFFFFFull) return fail(ctx, MC_ERR_INVALID, "mc_load_target_windows: too many targets");
    ctx->targetWindows.assign(windows, windows + numTargets);
    ++ctx->windowsVersion;
    return MC_OK;
}

// the same announcement when only bounds are known: targets 0 .. maxTarget, each with maxWindow + 1 windows
int mc_load_location_range(mc_ctx* ctx, uint32_t maxTarget, uint32_t maxWindow)
{
    if (!ctx) return MC_ERR_INVALID;
    for (auto& p : ctx->parts) if (p.announced) return fail(ctx, MC_ERR_STATE, "mc_load_location_range: call it before mc_load_begin");
    ctx->targetWindows.clear();
    if (((uint64_t)maxTarget + 1) * ((uint64_t)maxWindow + 1 + kGwGap) < 0xFFFFFFFFull) ctx->targetWindows.assign((size_t)maxTarget + 1, maxWindow + 1);
    ++ctx->windowsVersion;
    return MC_OK;
}

int mc_load_begin(mc_ctx* ctx, uint32_t part, uint64_t nkeys, uint64_t nvalues)
{
    if (!ctx) return MC_ERR_INVALID;
    if (part >= ctx->parts.size()) return fail(ctx, MC_ERR_INVALID, "mc_load_begin: part out of range");
    Part& P = ctx->parts[part];
    if (P.announced) return fail(ctx, MC_ERR_STATE, "mc_load_begin: part already announced");
    if (ctx->cfg.target_shard_count > 1 && !ctx->tgtRangeSet)
        return fail(ctx, MC_ERR_UNSUPPORTED, "target shards are cut from a database file (mc_open_database), not from mc_load_batch arrays");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    P.expectKeys = nkeys; P.expectValues = nvalues;
    P.announced = true; P.loading = true;
    return ctx->parts.size() == 1 ? allocate_table(ctx) : MC_OK;
}

int mc_load_batch(mc_ctx* ctx, uint32_t part, const uint32_t* keys, const uint8_t* sizes, const void* values, uint64_t n)
{
    if (!ctx) return MC_ERR_INVALID;
    if (part >= ctx->parts.size() || !ctx->parts[part].loading) return fail(ctx, MC_ERR_STATE, "mc_load_batch: call mc_load_begin first");
    Part& P = ctx->parts[part];
    Part& T = ctx->parts[0];
    const bool multi = ctx->parts.size() > 1;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (multi && T.hbuckets.empty()) {
        for (auto& q : ctx->parts)
            if (!q.announced) return fail(ctx, MC_ERR_STATE, "multi-part load: call mc_load_begin for EVERY part before the first mc_load_batch");
        if (int rc = allocate_table(ctx)) return rc;
    }
    if (P.keysLoaded + n > P.expectKeys) return fail(ctx, MC_ERR_INVALID, "mc_load_batch: more keys than announced");
    if (!multi) return load_batch_device(ctx, keys, sizes, static_cast<const uint8_t*>(values), n);
    // several parts: buckets of one feature are merged across parts on the host, the table goes up in mc_load_end
    MergeCounters c{T.keysStored, P.locations, T.maxProbe};
    const MergeStatus ms = merge_part_batch(T.hbuckets, ctx->hvalues, part, keys, sizes, static_cast<const uint8_t*>(values), n, ctx->cfg.target_id_bytes,
                                            ctx->cfg.remove_overpopulated, ctx->cfg.max_locations_per_feature, c);
    T.keysStored = c.keysStored; P.locations = c.locations; T.maxProbe = c.maxProbe;
    if (ms == MergeStatus::TableFull) return fail(ctx, MC_ERR_NOMEM, "hash table full");
    if (ms == MergeStatus::BucketTooLarge) return fail(ctx, MC_ERR_UNSUPPORTED, "merged bucket exceeds 65535 locations");
    if (ms == MergeStatus::TargetTooLarge) return fail(ctx, MC_ERR_UNSUPPORTED, "multi-part databases need target ids < 2^24");
    P.keysLoaded += n;
    return MC_OK;
}

int mc_load_end(mc_ctx* ctx, uint32_t part)
{
    if (!ctx) return MC_ERR_INVALID;
    if (part >= ctx->parts.size() || !ctx->parts[part].loading) return fail(ctx, MC_ERR_STATE, "mc_load_end: nothing being loaded");
    Part& P = ctx->parts[part];
    Part& T = ctx->parts[0];
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    P.loading = false; P.ready = true;
    for (auto& q : ctx->parts) if (!q.ready) return MC_OK;     // the table goes to the device when the last part is in
    if (ctx->parts.size() == 1) {                              // built on the device: fetch the counters, drop the staging
        unsigned long long c[4] = {0, 0, 0, 0};
        HIP_TRY(ctx, hipMemcpy(c, ctx->bLdCounters.p, sizeof(c), hipMemcpyDeviceToHost));
        T.keysStored = c[0]; P.locations = c[1];
        T.maxProbe = std::max<uint32_t>(1u, (uint32_t)(c[2] & 0xFFFFFFFFull));
        const bool full = (c[2] >> 32) != 0;
        DevBuf* st[] = {&ctx->bLdKeys, &ctx->bLdSizes, &ctx->bLdVals, &ctx->bLdFileSz, &ctx->bLdStoreSz, &ctx->bLdFileOff, &ctx->bLdStoreOff,
                        &ctx->bLdScan};
        for (auto* b : st) { if (b->p) (void)hipFree(b->p); b->p = nullptr; b->cap = 0; }
        if (full) return fail(ctx, MC_ERR_NOMEM, "hash table full");
        if (c[3]) { ctx->locRangeViolated = true; return fail(ctx, MC_ERR_INVALID, "a location lies outside the range announced with mc_load_target_windows / mc_load_location_range"); }
        ctx->tableReady = true;
        (void)build_direct_index(ctx);                            // (a lookup structure beside the buckets: not having it is not an error)
        reserve_pipes_after_load(ctx);
        return MC_OK;
    }
    if (T.hbuckets.empty()) { int rc = allocate_table(ctx); if (rc) return rc; }
    T.dvaluesCap = ctx->hvalues.size() + 1;
    HIP_TRY(ctx, hipMalloc((void**)&T.dvalues, T.dvaluesCap * sizeof(uint64_t)));
    if (!ctx->hvalues.empty())
        HIP_TRY(ctx, hipMemcpy(T.dvalues, ctx->hvalues.data(), ctx->hvalues.size() * 8, hipMemcpyHostToDevice));
    T.valuesStored = ctx->hvalues.size();
    std::vector<uint64_t>().swap(ctx->hvalues);
    const size_t bytes = T.hbuckets.size() * sizeof(TableBucket);
    HIP_TRY(ctx, hipMalloc((void**)&T.dbuckets, bytes));
    HIP_TRY(ctx, hipMemcpy(T.dbuckets, T.hbuckets.data(), bytes, hipMemcpyHostToDevice));
    std::vector<TableBucket>().swap(T.hbuckets);
    ctx->tableReady = true;
    reserve_pipes_after_load(ctx);
    return MC_OK;
}

}  // extern "C"
