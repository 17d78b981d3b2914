// metacache_amd/csrc/context.cpp -- host side of the C ABI: context, tuning, timing, the host slots with their coalescer, the pipes'
// reservations (the per-batch pipeline: query_pipe.cpp, its plan: query_rules.h; table loading: table_load.cpp).  (Compiled with hipcc;
// the kernels live in kernels.hip.)
#include "context.h"
#include "devcache.h"
#include "rows_common.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <thread>

using namespace mcamd;

static thread_local std::string g_createError;
// a helper thread that works on a context beside its owner (reserve_slot_pipes) must not write ctx->err: its failures stay its own
static thread_local bool t_quietErrors = false;
static thread_local std::string* t_errSink = nullptr;         // a dispatcher thread of the slot coalescer keeps its errors for the slots it carries
int mcamd::fail(mc_ctx* ctx, int code, const std::string& msg)
{
    if (t_errSink) { *t_errSink = msg; return code; }
    if (t_quietErrors) return code;
    if (ctx) ctx->err = msg; else g_createError = msg;
    return code;
}

int mcamd::ensure(mc_ctx* ctx, DevBuf& b, size_t bytes)
{
    if (bytes <= b.cap) return MC_OK;
    static const bool trace = std::getenv("MC_ALLOC_TRACE") != nullptr;      // allocations of 20 ms (MC_ALLOC_TRACE=<ms>) and more go to stderr
    static const double traceMs = [] { const char* e = std::getenv("MC_ALLOC_TRACE"); const double v = e ? std::atof(e) : 0; return v > 1.0 ? v : (e && e[0] == '0' ? 0.0 : 20.0); }();
    timespec t0{}, t1{}, t2{};
    if (trace) clock_gettime(CLOCK_MONOTONIC, &t0);
    if (b.p) HIP_TRY(ctx, hipFree(b.p));
    if (trace) clock_gettime(CLOCK_MONOTONIC, &t1);
    b.p = nullptr; b.cap = 0;
    size_t want = bytes + std::min<size_t>(bytes / 4, (size_t)512 << 20) + 256;   // head-room: fewer re-allocations (a quarter, at most 512 MB: the pools of a 2.5 M-pair batch are 11 GB each)
    HIP_TRY(ctx, dev_malloc(&b.p, want));
    b.cap = want;
    if (trace) {
        clock_gettime(CLOCK_MONOTONIC, &t2);
        const double f = (t1.tv_sec - t0.tv_sec) * 1e3 + (t1.tv_nsec - t0.tv_nsec) / 1e6, m = (t2.tv_sec - t1.tv_sec) * 1e3 + (t2.tv_nsec - t1.tv_nsec) / 1e6;
        if (f + m >= traceMs) std::fprintf(stderr, "mc ensure: %.1f MB: hipFree of the old buffer %.1f ms, hipMalloc %.1f ms\n", want / 1e6, f, m);
    }
    return MC_OK;
}

namespace {

// ---- MC_SUBMIT_TRACE=1: where the host spends a slot batch (sums over all threads, printed by mc_destroy) -----------------------
static const bool g_submitTrace = std::getenv("MC_SUBMIT_TRACE") != nullptr;
static std::atomic<uint64_t> g_trace[8];   // ns: [0] waiting for a free pipe, [1] enqueueing H2D, [2] query_on_pipe in all, [3] of it inside hipStreamSynchronize,
                                           //     [4] enqueueing D2H; [5] batches, [6] hipStreamSynchronize calls
static inline uint64_t trace_now() { timespec t; clock_gettime(CLOCK_MONOTONIC, &t); return (uint64_t)t.tv_sec * 1000000000ull + (uint64_t)t.tv_nsec; }

// ---- the runtime's slow submission state: calls that only ENQUEUE -- hipMemcpyAsync of a pinned buffer -- take milliseconds
// apiece once the HIP runtime's direct dispatch (AMD_DIRECT_DISPATCH, on by default) has gone into it, process by process, under many
// submitting threads.  The slot paths time exactly these calls (two clock reads per batch); a window of 32 batches whose enqueues
// averaged more than 0.5 ms each leaves a warning that names the switch: mc_runtime_warning(), and one line on stderr.
static std::atomic<uint64_t> g_enqNs{0}, g_enqCalls{0}, g_enqBatches{0};
static std::atomic<bool> g_enqWarned{false};
static std::mutex g_warnMu;
static std::string g_warning;
static void note_enqueues(uint64_t ns, uint32_t calls)
{
    if (g_enqWarned.load(std::memory_order_relaxed)) return;
    const uint64_t n = g_enqNs.fetch_add(ns) + ns, c = g_enqCalls.fetch_add(calls) + calls, b = g_enqBatches.fetch_add(1) + 1;
    if (b < 32) return;
    g_enqNs = 0; g_enqCalls = 0; g_enqBatches = 0;                 // (windows: racing updates only blur a window's edge)
    if (c == 0 || n / c < 500000ull) return;
    const char* dd = std::getenv("AMD_DIRECT_DISPATCH");
    if (dd && dd[0] == '0') return;                               // (already off: something else is slow)
    if (g_enqWarned.exchange(true)) return;
    char msg[400];
    std::snprintf(msg, sizeof msg, "metacache_amd: HIP calls that only enqueue (hipMemcpyAsync of pinned batches) take %.1f ms each in this process -- the HIP runtime's direct "
                  "dispatch does this under many submitting threads; start the process with AMD_DIRECT_DISPATCH=0 (the runtime reads it before main)", (double)(n / c) / 1e6);
    { std::lock_guard<std::mutex> l(g_warnMu); g_warning = msg; }
    std::fprintf(stderr, "%s\n", msg);
}

// ---- timing (ScopedTimer: rows_common.h) -------------------------------------------------
void collect_timers(mc_ctx* ctx)
{
    for (auto& kv : ctx->timers) {
        for (auto& pr : kv.second.pending) {
            (void)hipEventSynchronize(pr.second);
            float ms = 0;
            if (hipEventElapsedTime(&ms, pr.first, pr.second) == hipSuccess) { kv.second.ms += ms; kv.second.launches++; }
            ctx->eventPool.push_back(pr.first); ctx->eventPool.push_back(pr.second);
        }
        kv.second.pending.clear();
    }
}

}  // namespace

void mcamd::set_global_error(const std::string& msg) { g_createError = msg; }
mcamd::OpenHints& mcamd::open_hints() { static thread_local OpenHints h; return h; }

hipError_t mcamd::traced_sync(hipStream_t st)
{
    if (!g_submitTrace) return hipStreamSynchronize(st);
    const uint64_t t0 = trace_now();
    const hipError_t e = hipStreamSynchronize(st);
    g_trace[3] += trace_now() - t0; ++g_trace[6];
    return e;
}

extern "C" {

void mc_config_default(mc_config* c)
{
    std::memset(c, 0, sizeof(*c));
    c->device = 0;
    c->kmerlen = 16; c->sketchlen = 16; c->winlen = 127; c->winstride = 112;   // options.hpp:102, options.cpp:625
    c->max_candidates = 2;                                                      // options.hpp:257
    c->target_id_bytes = 4;
    c->num_parts = 1;
    c->max_locations_per_feature = 0;
    c->remove_overpopulated = 0;
    c->max_load_factor = 0.3f;   // few full buckets => most lookups end after one line (measured: 0.5 -> 0.3 is 8 % on the probing kernel)
                                 // (the reference CPU map uses 0.8, host_hashmap.hpp:159-161; -max-load-fac overrides)
    c->num_slots = 1;
    c->slot_max_queries = 1u << 16;
    c->slot_max_chars = 1u << 24;
    c->copy_allhits = 0;
    c->single_part = -1;
    c->key_shard_index = 0; c->key_shard_count = 1;
    c->target_shard_index = 0; c->target_shard_count = 1;
}

const char* mc_last_error(const mc_ctx* ctx) { return ctx ? ctx->err.c_str() : g_createError.c_str(); }

static void co_dispatch(mc_ctx* ctx, mcamd::CoDispatcher* D);
static void co_run(mc_ctx* ctx, mcamd::CoDispatcher* D, const std::vector<uint32_t>& mine, int lowest);

int mc_create(const mc_config* cfg, mc_ctx** out)
{
    if (!cfg || !out) return fail(nullptr, MC_ERR_INVALID, "mc_create: null argument");
    *out = nullptr;
    if (cfg->kmerlen < 1 || cfg->kmerlen > 16) return fail(nullptr, MC_ERR_UNSUPPORTED, "kmerlen must be 1..16 (kmer_type = uint32_t)");
    if (cfg->sketchlen < 1 || cfg->sketchlen > kMaxSketch) return fail(nullptr, MC_ERR_UNSUPPORTED, "sketchlen must be 1..32");
    if (cfg->winlen < cfg->kmerlen || cfg->winlen > kMaxWinLen) return fail(nullptr, MC_ERR_UNSUPPORTED, "winlen must be kmerlen..1024");
    if (cfg->winstride < 1) return fail(nullptr, MC_ERR_INVALID, "winstride must be >= 1");
    if (cfg->target_id_bytes != 2 && cfg->target_id_bytes != 4) return fail(nullptr, MC_ERR_INVALID, "target_id_bytes must be 2 or 4");
    if (cfg->num_parts < 1 || cfg->num_parts > 255) return fail(nullptr, MC_ERR_UNSUPPORTED, "num_parts must be 1..255");
    if (cfg->max_candidates < 1) return fail(nullptr, MC_ERR_INVALID, "max_candidates must be >= 1");
    if (cfg->key_shard_count > 1 && cfg->key_shard_index >= cfg->key_shard_count) return fail(nullptr, MC_ERR_INVALID, "key_shard_index out of range");
    if (cfg->target_shard_count > 1) {
        if (cfg->target_shard_index >= cfg->target_shard_count) return fail(nullptr, MC_ERR_INVALID, "target_shard_index out of range");
        if (cfg->key_shard_count > 1) return fail(nullptr, MC_ERR_UNSUPPORTED, "target shards and key shards cannot be combined");
        if (cfg->num_parts > 1) return fail(nullptr, MC_ERR_UNSUPPORTED, "target shards need a single part per context (single_part)");
    }

    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev < 1) return fail(nullptr, MC_ERR_HIP, "no usable HIP device (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail(nullptr, MC_ERR_INVALID, "device ordinal out of range");

    auto* ctx = new mc_ctx;
    ctx->cfg = *cfg;
    ctx->device = cfg->device;
    ctx->querySketch = SketchParams{cfg->kmerlen, cfg->sketchlen, cfg->winlen, cfg->winstride};
    ctx->targetSketch = ctx->querySketch;
    ctx->loadFactor = (cfg->max_load_factor > 0.05f && cfg->max_load_factor <= 0.99f) ? cfg->max_load_factor : 0.3f;
    ctx->parts.resize(cfg->num_parts);
    if (const char* e = std::getenv("MC_NO_LANE_PATH")) ctx->useLanePath = !(e[0] == '1');   // debugging aid
    if (const char* e = std::getenv("MC_LANE_FUSION")) ctx->fuseLane = e[0] == '1' ? 1 : 0;   // (default: by table size)
    ctx->listAlignWant = mcamd::open_hints().listAlign; ctx->listAlignShare = mcamd::open_hints().listAlignShare;
    ctx->directWant = mcamd::open_hints().directIndex;
    if (const char* e = std::getenv("MC_DIRECT_INDEX")) ctx->directWant = e[0] == '1' ? 1 : 0;
    if (const char* e = std::getenv("MC_LIST_ALIGN")) ctx->listAlignWant = e[0] == '1' ? 1 : 0;   // (default: where the padded store is affordable)
    if (const char* e = std::getenv("MC_GW_FUSE")) ctx->gwFuse = e[0] == '5' ? 5 : e[0] == '6' ? 6 : e[0] == '1' ? 1 : 0;   // (5 / 6: the fused kernel's five- / six-waves-per-SIMD instances)
    if (const char* e = std::getenv("MC_QUAD_LOOKUP")) ctx->quadLookup = e[0] == '1' ? 1 : 0;   // tests
    if (const char* e = std::getenv("MC_COMPACT_LOCATIONS")) ctx->compactAllowed = e[0] != '0';   // tests / tuning
    if (const char* e = std::getenv("MC_BIG_MIN")) ctx->bigMin = (uint32_t)std::max(0, std::atoi(e));   // tests / tuning
    if (hipSetDevice(ctx->device) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return fail(nullptr, MC_ERR_HIP, "cannot create HIP stream");
    }
    ctx->pipe0.stream = ctx->stream;
    // host slots
    ctx->slots.resize(cfg->num_slots);
    const size_t K = cfg->max_candidates;
    for (auto& s : ctx->slots) {
        const size_t nq = cfg->slot_max_queries, nc = (size_t)cfg->slot_max_chars + 16;
        bool ok = hipHostMalloc((void**)&s.hseq, nc) == hipSuccess && hipHostMalloc((void**)&s.hqinfo, nq * 16) == hipSuccess &&
                  hipHostMalloc((void**)&s.hmaxwin, nq * 4) == hipSuccess && hipMalloc((void**)&s.dseq, nc) == hipSuccess &&
                  hipMalloc((void**)&s.dqinfo, nq * 16) == hipSuccess && hipMalloc((void**)&s.dmaxwin, nq * 4) == hipSuccess &&
                  hipHostMalloc((void**)&s.hcands, nq * K * sizeof(mc_candidate)) == hipSuccess &&
                  hipHostMalloc((void**)&s.hqstat, nq * sizeof(QueryStat)) == hipSuccess &&
                  hipHostMalloc((void**)&s.hhitcounts, nq * 4) == hipSuccess &&
                  hipHostMalloc((void**)&s.hhitoff, (nq + 1) * 8) == hipSuccess && hipEventCreate(&s.done) == hipSuccess;
        if (!ok) { mc_destroy(ctx); return fail(nullptr, MC_ERR_NOMEM, "cannot allocate slot buffers"); }
    }
    uint32_t npipes = std::min<uint32_t>(cfg->num_slots, 8);
    if (const char* e = std::getenv("MC_PIPES")) npipes = std::max(1, std::atoi(e));
    // Slots that are submitted side by side go to the device as ONE batch (slot coalescer, below): several slots, top candidates only.
    // MC_SLOT_COALESCE=0: every slot its own batch on a pipe it borrows, as before round 6.
    // Slots of 8 192 reads and fewer (the reference's 4 096): there a batch per slot is bound by its launches (at 16 384 reads per slot united and
    // apart are level: 4 133 / 5 402 / 6 136 / 7 279 against 3 479 / 6 000 / 6 537 / 6 535 Mreads/min with 4 / 8 / 16 / 32 threads).  Larger slots keep a batch
    // each on a pipe they borrow -- united they gain nothing (10 554 against 10 618 Mreads/min at 65 536 reads per slot) and `mcq`, whose 32
    // workers run under AMD_DIRECT_DISPATCH=0, lost a third of its query phase (97 against 68 ms per 10^7 reads at 30 Gbp, profiles/r06_e2e_matrix02.json).
    // MC_SLOT_COALESCE=1 / 0 forces either.
    ctx->coalesce = cfg->num_slots >= 2 && !cfg->copy_allhits && cfg->slot_max_queries <= 8192;
    if (const char* e = std::getenv("MC_SLOT_COALESCE")) ctx->coalesce = cfg->num_slots >= 2 && !cfg->copy_allhits && e[0] != '0';
    if (ctx->coalesce) {
        // dispatchers: one united batch each in flight: few submitters find a free one at once (their slots go alone), many find them busy and
        // their slots wait together.  FIVE: the runtime runs a process' streams on four hardware queues, and pipes that share one take turns
        // (a united batch's chain of ~25 steps: 715 / 770 / 1 014 us with 4 / 6 / 8 pipes).  Same box, 4 096-read slots, 8 / 16 / 32 threads:
        // 4 pipes 2 960 / 4 010-4 070 / 5 400-5 470, five 3 350 / 4 530-4 550 / 5 790-5 920, six 3 070-3 140 / 3 940-4 120 / 5 380-5 490,
        // eight 3 030-3 060 / 3 930-3 960 / 5 320-5 400 Mreads/min (docs/LAB_NOTEBOOK_r06.md section 5b).  MC_PIPES / MC_SLOT_DISPATCHERS override.
        if (!std::getenv("MC_PIPES")) npipes = std::min<uint32_t>(npipes, 5);
        if (const char* e = std::getenv("MC_SLOT_DISPATCHERS")) npipes = (uint32_t)std::min(8, std::max(1, std::atoi(e)));
        // what a united batch may hold: up to 2^18 reads (beyond that the kernels run at their large-batch rate anyway), character offsets are 32 bits
        ctx->coMaxQueries = (uint32_t)std::max<uint64_t>(cfg->slot_max_queries, std::min<uint64_t>(1u << 18, (uint64_t)cfg->num_slots * cfg->slot_max_queries));
        ctx->coMaxChars = std::max<uint64_t>(cfg->slot_max_chars, std::min<uint64_t>(1ull << 30, (uint64_t)cfg->num_slots * cfg->slot_max_chars));
    }
    for (uint32_t i = 0; i < npipes && i < cfg->num_slots; ++i) {
        Pipe* p = new Pipe;
        ctx->pipes.push_back(p);
        if (hipStreamCreateWithFlags(&p->stream, hipStreamNonBlocking) != hipSuccess) { mc_destroy(ctx); return fail(nullptr, MC_ERR_HIP, "cannot create HIP stream"); }
        if (!ctx->coalesce) ctx->freePipes.push_back(p);
    }
    if (ctx->coalesce) {
        for (Pipe* p : ctx->pipes) {
            auto* d = new mcamd::CoDispatcher;
            d->pipe = p;
            bool ok = true;
            for (int k = 0; k < 2 && ok; ++k)
                ok = hipHostMalloc((void**)&d->hq[k], (size_t)ctx->coMaxQueries * 20) == hipSuccess &&
                     hipEventCreateWithFlags(&d->staged[k], hipEventDisableTiming) == hipSuccess;
            for (int k = 0; k < 4 && ok; ++k) ok = hipEventCreateWithFlags(&d->done[k], hipEventDisableTiming) == hipSuccess;
            ctx->coDisp.push_back(d);
            if (!ok) { mc_destroy(ctx); return fail(nullptr, MC_ERR_NOMEM, "cannot allocate the slot coalescer's staging"); }
        }
        ctx->coFree = ctx->coDisp;
        for (auto* d : ctx->coDisp) d->th = std::thread(co_dispatch, ctx, d);
    }
    *out = ctx;
    return MC_OK;
}

void mc_destroy(mc_ctx* ctx)
{
    if (g_submitTrace && ctx && g_trace[5].load())
        std::fprintf(stderr, "mc submit trace: %llu batches; ms summed over the submitting threads: waiting for a pipe %.1f, H2D enqueue %.1f, query %.1f (of it %.1f in %llu hipStreamSynchronize calls), D2H enqueue %.1f\n",
                     (unsigned long long)g_trace[5].load(), g_trace[0] / 1e6, g_trace[1] / 1e6, g_trace[2] / 1e6, g_trace[3] / 1e6, (unsigned long long)g_trace[6].load(), g_trace[4] / 1e6);
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (!ctx->coDisp.empty()) {                                     // the slot coalescer's dispatchers: let them finish what they carry, then go
        { std::lock_guard<std::mutex> l(ctx->coMu); ctx->coStop = true; }
        ctx->coCv.notify_all();
        for (auto* d : ctx->coDisp) if (d->th.joinable()) d->th.join();
        for (auto* d : ctx->coDisp) {
            if (d->pipe && d->pipe->stream) (void)hipStreamSynchronize(d->pipe->stream);
            for (int k = 0; k < 2; ++k) { if (d->hq[k]) (void)hipHostFree(d->hq[k]); if (d->hmw[k]) (void)hipHostFree(d->hmw[k]); if (d->staged[k]) (void)hipEventDestroy(d->staged[k]); }
            for (int k = 0; k < 4; ++k) if (d->done[k]) (void)hipEventDestroy(d->done[k]);
            for (DevBuf* b : {&d->dseq, &d->dqinfo, &d->dmaxwin}) if (b->p) (void)hipFree(b->p);
            delete d;
        }
        ctx->coDisp.clear();
    }
    // every stream that may still run kernels on the tables: the context's, both pipes', the slots' (callers' own streams: theirs to wait for)
    if (ctx->pipe0.tail.pending || ctx->pipe1.tail.pending) { ctx->pipe0.tail.pending = false; ctx->pipe1.tail.pending = false; }   // (a deferred tail nobody asked for is dropped)
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->pipe0.stream) (void)hipStreamSynchronize(ctx->pipe0.stream);
    if (ctx->pipe1.stream) (void)hipStreamSynchronize(ctx->pipe1.stream);
    for (Pipe* p : ctx->pipes) if (p->stream) (void)hipStreamSynchronize(p->stream);
    if (ctx->buildHold) { big_cache_hold(-1); ctx->buildHold = false; }   // (a table build that was abandoned before mc_build_table_end)
    for (auto& p : ctx->parts) { if (p.dbuckets) (void)big_free(p.dbuckets); if (p.dvalues) (void)big_free(p.dvalues); if (p.ddirect) (void)big_free(p.ddirect); }
    free_align_works(ctx);
    free_classify_state(ctx);
    free_coverage_state(ctx);
    free_target_hits_state(ctx);
    free_evaluate_state(ctx);
    free_format_state(ctx);
    free_parse_state(ctx);
    free_cut_state(ctx);
    free_targets_state(ctx);
    free_merge_results_state(ctx);
    free_inflate_state(ctx);
    free_taxmap_state(ctx);
    for (auto& kv : ctx->taxkeyDev) (void)hipFree(kv.second);
    if (ctx->dGwBase) (void)hipFree(ctx->dGwBase);
    if (ctx->dGwDir) (void)hipFree(ctx->dGwDir);
    auto free_pipe = [](Pipe& P, bool ownStream) {
        if (P.stream) (void)hipStreamSynchronize(P.stream);
        if (P.hTotal) (void)hipHostFree(P.hTotal);
        if (P.tail.mainDone) (void)hipEventDestroy(P.tail.mainDone);
        if (P.sortSide.stream) { (void)hipStreamSynchronize(P.sortSide.stream); (void)hipStreamDestroy(P.sortSide.stream); }
        if (P.sortSide.fork) (void)hipEventDestroy(P.sortSide.fork);
        if (P.sortSide.join) (void)hipEventDestroy(P.sortSide.join);
        for (DevBuf* b : P.buffers()) if (b->p) (void)hipFree(b->p);
        if (ownStream && P.stream) (void)hipStreamDestroy(P.stream);
    };
    free_pipe(ctx->pipe0, false);
    free_pipe(ctx->pipe1, true);
    for (Pipe* p : ctx->pipes) { free_pipe(*p, true); delete p; }
    ctx->pipes.clear(); ctx->freePipes.clear();
    DevBuf* bufs[] = {&ctx->bLdKeys, &ctx->bLdSizes, &ctx->bLdVals, &ctx->bLdFileSz, &ctx->bLdStoreSz, &ctx->bLdFileOff, &ctx->bLdStoreOff,
                      &ctx->bLdScan, &ctx->bLdCounters};
    for (auto* b : bufs) if (b->p) (void)hipFree(b->p);
    for (auto& s : ctx->slots) {
        if (s.hseq) (void)hipHostFree(s.hseq); if (s.hqinfo) (void)hipHostFree(s.hqinfo); if (s.hmaxwin) (void)hipHostFree(s.hmaxwin);
        if (s.dseq) (void)hipFree(s.dseq); if (s.dqinfo) (void)hipFree(s.dqinfo); if (s.dmaxwin) (void)hipFree(s.dmaxwin);
        for (void* p : {(void*)s.draw, s.dparseWs, s.dmatesWs, (void*)s.dhdr, (void*)s.dnames, (void*)s.dnameoff, (void*)s.dstatus}) if (p) (void)hipFree(p);
        if (s.hhdr) (void)hipHostFree(s.hhdr); if (s.hstatus) (void)hipHostFree(s.hstatus);
        for (void* p : {s.dhdrWs, (void*)s.dhdrText, (void*)s.dhdrOff}) if (p) (void)hipFree(p);
        if (s.hhdrText) (void)hipHostFree(s.hhdrText); if (s.hhdrOff) (void)hipHostFree(s.hhdrOff);
        if (s.hcands) (void)hipHostFree(s.hcands); if (s.hqstat) (void)hipHostFree(s.hqstat);
        if (s.hhitcounts) (void)hipHostFree(s.hhitcounts); if (s.hhitoff) (void)hipHostFree(s.hhitoff);
        if (s.hhits) (void)hipHostFree(s.hhits); if (s.done) (void)hipEventDestroy(s.done);
    }
    collect_timers(ctx);
    for (auto e : ctx->eventPool) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

int mc_table_layout(const mc_ctx* ctx, uint64_t layout[4])
{
    if (!ctx || !layout || ctx->parts.empty()) return MC_ERR_INVALID;
    const Part& T = ctx->parts[0];
    layout[0] = (T.compact ? 4 : 8) | (T.ddirect ? 1ull << 32 : 0); layout[1] = (T.compact ? ctx->gwGap : 0) | ((uint64_t)T.listAlign << 32); layout[2] = T.nbuckets; layout[3] = T.valuesStored;
    return MC_OK;
}

int mc_target_range(const mc_ctx* ctx, uint64_t range[4])
{
    if (!ctx || !range) return MC_ERR_INVALID;
    range[0] = ctx->tgtRangeSet ? ctx->tgtLo : 0;
    range[1] = ctx->tgtRangeSet ? ctx->tgtHi : ctx->targetCount;
    range[2] = ctx->parts.empty() ? 0 : ctx->parts[0].keysStored;
    range[3] = 0;
    for (const auto& p : ctx->parts) range[3] += p.locations;
    return MC_OK;
}

int mc_set_lineages(mc_ctx* ctx, const uint32_t* lin, uint64_t numTargets)
{
    if (!ctx || !lin) return MC_ERR_INVALID;
    for (uint64_t i = 0; i < numTargets * MC_NUM_RANKS; ++i)
        if (lin[i] >= (1u << 24)) return fail(ctx, MC_ERR_UNSUPPORTED, "taxon index does not fit 24 bits");
    ctx->lineages.assign(lin, lin + numTargets * MC_NUM_RANKS);
    if (ctx->targetCount < numTargets) ctx->targetCount = numTargets;
    for (auto& kv : ctx->taxkeyDev) (void)hipFree(kv.second);
    ctx->taxkeyDev.clear();
    ++ctx->lineageVersion;
    return MC_OK;
}

int mc_db_info(const mc_ctx* ctx, uint64_t info[8])
{
    if (!ctx) return MC_ERR_INVALID;
    info[0] = ctx->targetSketch.k; info[1] = ctx->targetSketch.s; info[2] = ctx->targetSketch.w; info[3] = ctx->targetSketch.stride;
    info[4] = ctx->maxLocs; info[5] = ctx->targetCount; info[6] = ctx->parts.size();
    uint64_t loc = 0;
    for (auto& p : ctx->parts) loc += p.locations;
    info[7] = loc;
    return MC_OK;
}

}  // extern "C"

// taxkey[tgt] = lowest_ranked_ancestor(tgt, rank) as taxon index + 1 (taxonomy.hpp:1260-1267)
int mcamd::taxkey_for_rank(mc_ctx* ctx, int rank, const uint32_t** out)
{
    *out = nullptr;
    if (rank <= 0) return MC_OK;
    if (rank >= MC_NUM_RANKS) return fail(ctx, MC_ERR_INVALID, "lowest_rank out of range");
    std::lock_guard<std::mutex> lock(ctx->taxMtx);             // slots submit concurrently
    auto it = ctx->taxkeyDev.find(rank);
    if (it != ctx->taxkeyDev.end()) { *out = it->second; return MC_OK; }
    if (ctx->lineages.empty()) return fail(ctx, MC_ERR_STATE, "lowest_rank > sequence needs mc_set_lineages first");
    const uint64_t nt = ctx->lineages.size() / MC_NUM_RANKS;
    std::vector<uint32_t> tk(nt, 0);
    for (uint64_t t = 0; t < nt; ++t)
        for (int r = rank; r < MC_NUM_RANKS; ++r)
            if (ctx->lineages[t * MC_NUM_RANKS + r]) { tk[t] = ctx->lineages[t * MC_NUM_RANKS + r]; break; }
    uint32_t* d = nullptr;
    HIP_TRY(ctx, hipMalloc((void**)&d, std::max<uint64_t>(nt, 1) * 4));
    HIP_TRY(ctx, hipMemcpy(d, tk.data(), nt * 4, hipMemcpyHostToDevice));
    ctx->taxkeyDev[rank] = d;
    *out = d;
    return MC_OK;
}

extern "C" {

// tuning / test hook: the switches the MC_* environment variables set at mc_create, changeable on a live context (no batch in flight)
int mc_set_tuning(mc_ctx* ctx, const char* name, int64_t value)
{
    if (!ctx || !name) return MC_ERR_INVALID;
    const std::string n(name);
    if (n == "big_min") ctx->bigMin = (uint32_t)std::max<int64_t>(0, value);
    else if (n == "quad_lookup") ctx->quadLookup = value < 0 ? -1 : (value != 0);
    else if (n == "lane_path") ctx->useLanePath = value != 0;
    else if (n == "compact_locations") ctx->compactAllowed = value != 0;      // before mc_load_begin
    else if (n == "filter_bpc") ctx->filterBpc = (int)value;                  // blocks per CU of the filter kernels' persistent grids (0 = default); this context only
    else if (n == "count_bpc") ctx->countBpc = (int)value;
    else if (n == "direct_index") {                                // before the table is loaded; on a loaded table: 0 drops the index, 1 / -1 builds it now (by the rules above)
        ctx->directWant = value < 0 ? -1 : (value != 0);
        if (ctx->tableReady && ctx->parts.size() == 1) {
            Part& T = ctx->parts[0];
            HIP_TRY(ctx, hipSetDevice(ctx->device));
            const bool wanted = value > 0 || (value < 0 && (uint64_t)T.nbuckets * sizeof(TableBucket) >= (8ull << 30));
            if (!wanted && T.ddirect) { HIP_TRY(ctx, hipDeviceSynchronize()); (void)big_free(T.ddirect); T.ddirect = nullptr; }
            else if (wanted) (void)build_direct_index(ctx);
        }
    }
    else if (n == "list_align") ctx->listAlignWant = value < 0 ? -1 : (value != 0);   // before the table is loaded: lists of the compact store on lines of their own
    else if (n == "filter_lookup") ctx->filterLookup = value < 0 ? -1 : (value != 0);   // the lane path's direct-index lookups inside the filter kernel (-1: size-built index, batches without the host's look at the counters)
    else if (n == "lane_fusion") ctx->fuseLane = value < 0 ? -1 : (value != 0);   // sketch + probe of the lane path in one kernel (-1: where the lookups are quad-cooperative)
    else if (n == "gw_mid_h") ctx->gwMidH = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 32768));   // reads up to this many locations: the stream filter's small-filter instance (0 = none; default 8 192)
    else if (n == "gw_big_h") ctx->gwBigH = value <= 0 ? 0xFFFFFFFFu : (uint32_t)std::min<int64_t>(value, 0xFFFFFFFFll);   // reads beyond this many locations: the stream filter's fine-block instance (0 = none; default 32 768)
    else if (n == "gw_fuse") ctx->gwFuse = (value == 5 || value == 6) ? (int)value : (value != 0);                         // counting of short filtered lists inside the filter kernel: 1 (default) = fused, 0 = the two kernels apart
    else if (n == "align_scratch_mb") ctx->alignScratchMb = std::max<int64_t>(1, value);   // mc_align_semiglobal: device output + scratch of one sub-batch (default 512)
    else if (n == "coverage_load_first") ctx->coverageLoadFirst = value != 0;   // mc_coverage_add: 0 = every mask goes out as an atomic (the form it was measured against)
    else if (n == "target_hits_max_mb") ctx->targetHitsMaxMb = std::max<int64_t>(0, std::min<int64_t>(value, 1ll << 24));   // mc_target_hits_add(MC_TARGET_HITS_HOST): the log's largest size in MiB (default 8192)
    else if (n == "format_stage_rows") ctx->formatStageRows = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 1ll << 26));   // mc_format_mappings(MC_FORMAT_HOST): reads per staged piece (0 = default)
    else if (n == "format_stage_hits") ctx->formatStageHits = (uint64_t)std::max<int64_t>(0, std::min<int64_t>(value, 1ll << 30));   // mc_format_matches(MC_FORMAT_HOST): locations per staged piece (0 = default)
    else if (n == "evaluate_stage_rows") ctx->evaluateStageRows = (uint32_t)std::max<int64_t>(0, std::min<int64_t>(value, 1ll << 26));   // mc_evaluate_assignments(MC_EVALUATE_HOST): reads per staged piece (0 = default)
    else if (n == "inflate_stage_bytes") ctx->inflateStageBytes = (uint64_t)std::max<int64_t>(0, std::min<int64_t>(value, 1ll << 32));   // mc_inflate_blocks(MC_INFLATE_HOST): compressed bytes per staged piece (0 = default)
    else return fail(ctx, MC_ERR_INVALID, "mc_set_tuning: unknown switch '" + n + "'");
    return MC_OK;
}

int mc_synchronize(mc_ctx* ctx)
{
    if (!ctx) return MC_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return drain_query_streams(ctx);
}

int mc_query_wait(mc_ctx* ctx, int flags)
{
    if (!ctx) return MC_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = (flags & MC_SECOND_PIPE) ? ctx->pipe1.stream : ctx->stream;
    if (st) HIP_TRY(ctx, traced_sync(st));
    return MC_OK;
}

int mc_copy_results(mc_ctx* ctx, void* dst, const void* src, uint64_t bytes, int kind) { return mc_copy_results_on(ctx, dst, src, bytes, kind, nullptr); }

int mc_copy_results_on(mc_ctx* ctx, void* dst, const void* src, uint64_t bytes, int kind, void* stream)
{
    if (!ctx || !dst || !src) return MC_ERR_INVALID;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // kind: bit 0 = device -> host, bit 1 = host -> device (else device -> device); MC_SECOND_PIPE: on the second pipe's stream when no stream is given
    if ((kind & MC_SECOND_PIPE) && !stream && !ctx->pipe1.stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->pipe1.stream, hipStreamNonBlocking));
    hipStream_t st = stream ? (hipStream_t)stream : (kind & MC_SECOND_PIPE) ? ctx->pipe1.stream : ctx->stream;
    const hipMemcpyKind how = (kind & 1) ? hipMemcpyDeviceToHost : (kind & 2) ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, how, st));
    return MC_OK;
}

int mc_buffer_alloc(mc_ctx* ctx, uint64_t bytes, int kind, void** out)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!out || bytes == 0 || (kind != 0 && kind != 1)) return fail(ctx, MC_ERR_INVALID, "mc_buffer_alloc: no place for the pointer, no bytes or an unknown kind");
    *out = nullptr;
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_buffer_alloc: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const hipError_t e = kind == 0 ? hipMalloc(out, bytes) : hipHostMalloc(out, bytes);
    if (e != hipSuccess) { (void)hipGetLastError(); *out = nullptr; return fail(ctx, MC_ERR_NOMEM, std::string("mc_buffer_alloc: ") + hipGetErrorString(e)); }
    return MC_OK;
}

void mc_buffer_free(mc_ctx* ctx, void* p, int kind)
{
    if (!ctx || !p || (kind != 0 && kind != 1) || !ctx->stream) return;
    (void)hipSetDevice(ctx->device);
    if (kind == 0) (void)hipFree(p); else (void)hipHostFree(p);
}

int mc_timing_enable(mc_ctx* ctx, int on) { if (!ctx) return MC_ERR_INVALID; ctx->timing = on != 0; return MC_OK; }
int mc_timing_reset(mc_ctx* ctx)
{
    if (!ctx) return MC_ERR_INVALID;
    collect_timers(ctx);
    for (auto& kv : ctx->timers) { kv.second.ms = 0; kv.second.launches = 0; }
    return MC_OK;
}
int mc_timing_get(mc_ctx* ctx, const char* kernel, double* ms, uint64_t* launches)
{
    if (!ctx || !kernel) return MC_ERR_INVALID;
    collect_timers(ctx);
    auto it = ctx->timers.find(kernel);
    if (ms) *ms = it == ctx->timers.end() ? 0.0 : it->second.ms;
    if (launches) *launches = it == ctx->timers.end() ? 0 : it->second.launches;
    return MC_OK;
}

// ------------------------------------------------------------------------------------------------
// host batch slots
// ------------------------------------------------------------------------------------------------
int mc_batch_add(mc_ctx* ctx, uint32_t slot, const char* s1, uint32_t l1, const char* s2, uint32_t l2, uint32_t maxWin)
{
    if (!ctx || slot >= ctx->slots.size()) return MC_ERR_INVALID;
    Slot& S = ctx->slots[slot];
    if (S.submitted) return fail(ctx, MC_ERR_STATE, "mc_batch_add: slot is in flight, call mc_batch_wait + mc_batch_clear");
    if (S.raw) return fail(ctx, MC_ERR_STATE, "mc_batch_add: the slot holds a raw byte range (mc_batch_add_file_bytes), call mc_batch_submit");
    if (l2 == kNoTail) return fail(ctx, MC_ERR_INVALID, "sequence too long");
    const uint64_t need = ((uint64_t)l1 + 3) / 4 * 4 + ((uint64_t)l2 + 3) / 4 * 4;
    if (need > ctx->cfg.slot_max_chars) return fail(ctx, MC_ERR_INVALID, "query longer than the slot's character capacity");
    if (S.nq >= ctx->cfg.slot_max_queries || S.nchars + need > ctx->cfg.slot_max_chars) return MC_BATCH_FULL;
    uint32_t* qi = S.hqinfo + (size_t)S.nq * 4;
    qi[0] = (uint32_t)S.nchars; qi[1] = l1;
    if (l1) std::memcpy(S.hseq + S.nchars, s1, l1);
    S.nchars += ((uint64_t)l1 + 3) / 4 * 4;
    qi[2] = (uint32_t)S.nchars; qi[3] = l2;
    if (l2) std::memcpy(S.hseq + S.nchars, s2, l2);
    S.nchars += ((uint64_t)l2 + 3) / 4 * 4;
    S.hmaxwin[S.nq] = maxWin;
    if (l2 == 0 && l1 > S.maxSingle) S.maxSingle = l1;
    S.nq++;
    return MC_OK;
}

int64_t mc_batch_add_bulk(mc_ctx* ctx, uint32_t slot, const char* seqs, const uint64_t* offs, uint64_t n, uint64_t insertMax)
{
    if (!ctx || slot >= ctx->slots.size() || !seqs || !offs) return MC_ERR_INVALID;
    const uint64_t stride = ctx->targetSketch.stride ? ctx->targetSketch.stride : 1;
    uint64_t i = 0;
    for (; i < n; ++i) {
        const uint64_t len = offs[i + 1] - offs[i];
        if (len >= 0xFFFFFFF0ull) return fail(ctx, MC_ERR_INVALID, "sequence too long");
        const uint32_t maxWin = (uint32_t)(2 + std::max<uint64_t>(len, insertMax) / stride);
        const int rc = mc_batch_add(ctx, slot, seqs + offs[i], (uint32_t)len, nullptr, 0, maxWin);
        if (rc == MC_BATCH_FULL) break;
        if (rc < 0) return rc;
    }
    return (int64_t)i;
}

int mc_batch_add_file_bytes(mc_ctx* ctx, uint32_t slot, const char* bytes, uint64_t nbytes, int flags, uint64_t insertMax)
{
    if (!ctx || slot >= ctx->slots.size()) return MC_ERR_INVALID;
    if (!bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_batch_add_file_bytes: no bytes");
    if (flags & ~MC_PARSE_PAIRS) return fail(ctx, MC_ERR_INVALID, "mc_batch_add_file_bytes: unknown flag");
    Slot& S = ctx->slots[slot];
    if (S.submitted) return fail(ctx, MC_ERR_STATE, "mc_batch_add_file_bytes: slot is in flight, call mc_batch_wait + mc_batch_clear");
    if (S.nq || S.raw) return fail(ctx, MC_ERR_STATE, "mc_batch_add_file_bytes: the slot already holds reads");
    if (nbytes > ctx->cfg.slot_max_chars) return MC_BATCH_FULL;
    std::memcpy(S.hseq, bytes, nbytes);
    S.raw = true; S.rawBytes = nbytes; S.rawBytes2 = 0; S.rawFlags = flags; S.rawInsertMax = insertMax;
    return MC_OK;
}

int mc_batch_add_device_bytes(mc_ctx* ctx, uint32_t slot, const void* dbytes, uint64_t nbytes, int flags, uint64_t insertMax)
{
    if (!ctx || slot >= ctx->slots.size()) return MC_ERR_INVALID;
    if (!dbytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_batch_add_device_bytes: no bytes");
    if (flags & ~MC_PARSE_PAIRS) return fail(ctx, MC_ERR_INVALID, "mc_batch_add_device_bytes: unknown flag");
    Slot& S = ctx->slots[slot];
    if (S.submitted) return fail(ctx, MC_ERR_STATE, "mc_batch_add_device_bytes: slot is in flight, call mc_batch_wait + mc_batch_clear");
    if (S.nq || S.raw) return fail(ctx, MC_ERR_STATE, "mc_batch_add_device_bytes: the slot already holds reads");
    if (nbytes > ctx->cfg.slot_max_chars) return MC_BATCH_FULL;
    S.raw = true; S.rawDev = (const uint8_t*)dbytes; S.rawBytes = nbytes; S.rawBytes2 = 0; S.rawFlags = flags; S.rawInsertMax = insertMax;
    return MC_OK;
}

int mc_batch_add_file_mates(mc_ctx* ctx, uint32_t slot, const char* bytes1, uint64_t n1, const char* bytes2, uint64_t n2, uint64_t insertMax)
{
    if (!ctx || slot >= ctx->slots.size()) return MC_ERR_INVALID;
    if (!bytes1 || !bytes2 || n1 == 0 || n2 == 0) return fail(ctx, MC_ERR_INVALID, "mc_batch_add_file_mates: no bytes");
    Slot& S = ctx->slots[slot];
    if (S.submitted) return fail(ctx, MC_ERR_STATE, "mc_batch_add_file_mates: slot is in flight, call mc_batch_wait + mc_batch_clear");
    if (S.nq || S.raw) return fail(ctx, MC_ERR_STATE, "mc_batch_add_file_mates: the slot already holds reads");
    if (n1 > ctx->cfg.slot_max_chars || n2 > ctx->cfg.slot_max_chars || n1 + n2 > ctx->cfg.slot_max_chars) return MC_BATCH_FULL;
    std::memcpy(S.hseq, bytes1, n1);
    std::memcpy(S.hseq + n1, bytes2, n2);
    S.raw = true; S.rawBytes = n1; S.rawBytes2 = n2; S.rawFlags = 0; S.rawInsertMax = insertMax;
    return MC_OK;
}

// a raw slot's range to the device and through mc_parse_records on st; the stream is drained once, for the status: the query's launches
// need the number of reads.  Leaves the slot as mc_batch_add would have (nq, nchars, maxSingle) -- with no reads where the range was
// refused, or holds more than a slot takes (then status[4] says MC_PARSE_OVERFLOW)
static int raw_parse(mc_ctx* ctx, Slot& S, hipStream_t st)
{
    const uint64_t nq = ctx->cfg.slot_max_queries, nc = (uint64_t)ctx->cfg.slot_max_chars + 16;
    if (!S.draw) {
        HIP_TRY(ctx, hipMalloc((void**)&S.draw, nc));
        HIP_TRY(ctx, hipMalloc(&S.dparseWs, mc_parse_scratch_bytes(ctx->cfg.slot_max_chars)));
        HIP_TRY(ctx, hipMalloc((void**)&S.dhdr, nq * 16));
        HIP_TRY(ctx, hipMalloc((void**)&S.dnames, nc));
        HIP_TRY(ctx, hipMalloc((void**)&S.dnameoff, (nq + 1) * 8));
        HIP_TRY(ctx, hipMalloc((void**)&S.dstatus, 128));
        HIP_TRY(ctx, hipHostMalloc((void**)&S.hhdr, nq * 16));
        HIP_TRY(ctx, hipHostMalloc((void**)&S.hstatus, 128));
    }
    const bool mates = S.rawBytes2 != 0, pairs = mates || (S.rawFlags & MC_PARSE_PAIRS) != 0;
    const uint64_t at2 = (S.rawBytes + 15) / 16 * 16;                     // (the second range on the device: behind the first, at a multiple of 16; draw has 16 bytes to spare)
    const uint64_t matesWs = 2 * mc_parse_scratch_bytes(ctx->cfg.slot_max_chars) + mc_parse_mates_scratch_bytes(1, 1, (uint32_t)(2 * nq));   // (enough for every split of a slot's characters)
    if (mates && !S.dmatesWs) HIP_TRY(ctx, hipMalloc(&S.dmatesWs, matesWs));
    const uint32_t hdrRows = (uint32_t)(2 * nq);                           // (rows of dhdr)
    if (S.rawDev) {                                                        // (each on its own: a failed allocation is tried again by the next batch)
        if (!S.dhdrWs) HIP_TRY(ctx, hipMalloc(&S.dhdrWs, mc_parse_headers_scratch_bytes(hdrRows)));
        if (!S.dhdrText) HIP_TRY(ctx, hipMalloc((void**)&S.dhdrText, nc));
        if (!S.dhdrOff) HIP_TRY(ctx, hipMalloc((void**)&S.dhdrOff, ((uint64_t)hdrRows + 1) * 8));
        if (!S.hhdrText) HIP_TRY(ctx, hipHostMalloc((void**)&S.hhdrText, nc));   // (the headers are bytes of the range: the slot's character capacity holds them)
        if (!S.hhdrOff) HIP_TRY(ctx, hipHostMalloc((void**)&S.hhdrOff, ((uint64_t)hdrRows + 1) * 8));
    }
    if (S.rawDev) HIP_TRY(ctx, hipMemcpyAsync(S.draw, S.rawDev, S.rawBytes, hipMemcpyDeviceToDevice, st));
    else HIP_TRY(ctx, hipMemcpyAsync(S.draw, S.hseq, S.rawBytes, hipMemcpyHostToDevice, st));
    if (mates) HIP_TRY(ctx, hipMemcpyAsync(S.draw + at2, S.hseq + S.rawBytes, S.rawBytes2, hipMemcpyHostToDevice, st));
    mc_parse_output o{};
    o.hdr = S.dhdr; o.qinfo = S.dqinfo; o.seq = S.dseq; o.seq_capacity = nc; o.names = (char*)S.dnames; o.names_capacity = nc;
    o.name_off = S.dnameoff; o.max_win = S.dmaxwin; o.status = S.dstatus;
    o.max_records = (uint32_t)(pairs ? 2 * nq : nq);             // (qinfo, name_off and max_win take a row per QUERY)
    if (mates) {
        if (const int rc = mc_parse_mates(ctx, (const char*)S.draw, S.rawBytes, (const char*)S.draw + at2, S.rawBytes2, 0, S.rawInsertMax, &o, S.dmatesWs, matesWs, st)) return rc;
    } else
    if (const int rc = mc_parse_records(ctx, (const char*)S.draw, S.rawBytes, S.rawFlags, S.rawInsertMax, &o, S.dparseWs, mc_parse_scratch_bytes(ctx->cfg.slot_max_chars), st)) return rc;
    // (the headers' status: words 12 .. 15 of the slot's status, behind the 10 words that mc_parse_mates fills)
    if (S.rawDev) { if (const int rc = mcamd::enqueue_parse_headers(ctx, S.draw, (uint32_t)S.rawBytes, S.dhdr, S.dstatus, o.max_records, S.dhdrText, nc, S.dhdrOff, S.dstatus + 12, S.dhdrWs, st)) return rc; }
    HIP_TRY(ctx, hipMemcpyAsync(S.hstatus, S.dstatus, S.rawDev ? 128 : 64, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, traced_sync(st));
    uint64_t* status = S.hstatus;
    if (status[4] == MC_PARSE_OK && status[6] + 8 > ctx->cfg.slot_max_chars) status[4] = MC_PARSE_OVERFLOW;   // (a read the slot's loop would have refused)
    S.nq = 0; S.nchars = 0; S.maxSingle = 0;
    if (status[4] != MC_PARSE_OK) return MC_OK;
    S.nq = (uint32_t)status[1]; S.nchars = status[2] - 16;
    S.maxSingle = (uint32_t)std::min<uint64_t>(status[6], 0xFFFFFFFFull);   // (pairs: an upper bound of the half pair's length)
    HIP_TRY(ctx, hipMemcpyAsync(S.hhdr, S.dhdr, status[0] * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(ctx, hipMemcpyAsync(S.hqinfo, S.dqinfo, (size_t)S.nq * 16, hipMemcpyDeviceToHost, st));
    if (S.rawDev && status[14] == MC_PARSE_OK) {
        HIP_TRY(ctx, hipMemcpyAsync(S.hhdrOff, S.dhdrOff, (status[12] + 1) * 8, hipMemcpyDeviceToHost, st));
        if (status[13]) HIP_TRY(ctx, hipMemcpyAsync(S.hhdrText, S.dhdrText, status[13], hipMemcpyDeviceToHost, st));
    }
    return MC_OK;
}

static int submit_raw_coalesced(mc_ctx* ctx, Slot& S, int lowestRank);

// what the slot paths, which see every read on the host, tell query_on_pipe: no single read beyond a lane's reach (maxSingle: the longest)
static int slot_query_flags(uint32_t maxSingle) { return maxSingle <= mcamd::lane_max_len() ? mcamd::kQueryNoLongReads : 0; }
// ONE slot's batch: its n candidates and statistics to the slot's pinned buffers by one kernel (launch_deliver) instead of two copies
static void deliver_slot(const mc_ctx* ctx, Slot& S, const Pipe& P, const mc_device_results& res, uint32_t n, hipStream_t st)
{
    DeliverTable dt{};
    dt.e[0] = DeliverEntry{S.hcands, S.hqstat, 0u, n}; dt.n = 1;
    launch_deliver(dt, res.cands, P.bQstat.p, (uint32_t)ctx->cfg.max_candidates, st);
}

int mc_batch_records(mc_ctx* ctx, uint32_t slot, mc_batch_record_info* out)
{
    if (!ctx || slot >= ctx->slots.size() || !out) return MC_ERR_INVALID;
    Slot& S = ctx->slots[slot];
    if (!S.raw || !S.submitted || !S.hstatus) return fail(ctx, MC_ERR_STATE, "mc_batch_records: the slot holds no submitted raw range (mc_batch_add_file_bytes, mc_batch_submit, mc_batch_wait)");
    const bool ok = S.hstatus[4] == MC_PARSE_OK;
    out->verdict = (uint32_t)S.hstatus[4]; out->offence = S.hstatus[5];
    out->records = ok ? (uint32_t)S.hstatus[0] : 0; out->queries = ok ? (uint32_t)S.hstatus[1] : 0; out->half_pair = ok ? (uint32_t)S.hstatus[7] : 0;
    out->hdr = ok ? S.hhdr : nullptr; out->qinfo = ok ? S.hqinfo : nullptr;
    return MC_OK;
}

int mc_batch_headers(mc_ctx* ctx, uint32_t slot, const char** bytes, const uint64_t** off, uint64_t* records)
{
    if (!ctx || slot >= ctx->slots.size() || !bytes || !off || !records) return MC_ERR_INVALID;
    Slot& S = ctx->slots[slot];
    if (!S.raw || !S.submitted || !S.rawDev || !S.hstatus) return fail(ctx, MC_ERR_STATE, "mc_batch_headers: the slot holds no submitted device range (mc_batch_add_device_bytes, mc_batch_submit, mc_batch_wait)");
    const bool ok = S.hstatus[4] == MC_PARSE_OK && S.hstatus[14] == MC_PARSE_OK;
    *bytes = ok ? S.hhdrText : nullptr; *off = ok ? S.hhdrOff : nullptr; *records = ok ? S.hstatus[12] : 0;
    return MC_OK;
}

int mc_batch_submit(mc_ctx* ctx, uint32_t slot, int lowestRank)
{
    if (!ctx || slot >= ctx->slots.size()) return MC_ERR_INVALID;
    Slot& S = ctx->slots[slot];
    if (S.submitted) return fail(ctx, MC_ERR_STATE, "mc_batch_submit: slot already submitted");
    // every slot has its own stream and device workspace: batches of different slots overlap on the device (the reference orders
    // submissions with a mutex and overlaps through per-batch CUDA streams, database_query.hpp:110-113, query_batch.cu)
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (S.raw && ctx->coalesce) return submit_raw_coalesced(ctx, S, lowestRank);   // (never united with other slots)
    if (ctx->coalesce) {
        // hand the slot to the dispatchers: whatever is waiting when one of them comes free goes to the device as ONE batch
        S.submittedQueries = S.nq; S.coLowest = lowestRank; S.coRc = MC_OK; S.coEvent = false; S.coErr.clear();
        S.submitted = true;
        mcamd::CoDispatcher* D = nullptr;
        {
            std::lock_guard<std::mutex> l(ctx->coMu);
            if (S.nq == 0) S.coState = 3;
            else if (ctx->coPending.empty() && !ctx->coFree.empty()) {
                // nothing is waiting and a pipe is free: this slot goes out now, on the submitter's own thread -- no hand-over (a lone
                // submitter's batch takes what it took before there was a coalescer)
                D = ctx->coFree.back(); ctx->coFree.pop_back();
                S.coState = 2;
                ctx->coBatches++; ctx->coSlots++;
            }
            else { S.coState = 1; ctx->coPending.push_back(slot); }
        }
        if (D) {
            co_run(ctx, D, std::vector<uint32_t>{slot}, lowestRank);
            { std::lock_guard<std::mutex> l(ctx->coMu); ctx->coFree.push_back(D); }
            ctx->coCv.notify_one();
        } else if (S.nq) ctx->coCv.notify_one();
        return MC_OK;
    }
    const uint64_t tt0 = g_submitTrace ? trace_now() : 0;
    {
        std::unique_lock<std::mutex> lk(ctx->pipeMtx);
        ctx->pipeCv.wait(lk, [&] { return !ctx->freePipes.empty(); });
        S.pipe = ctx->freePipes.back();
        ctx->freePipes.pop_back();
    }
    const uint64_t tt1 = g_submitTrace ? trace_now() : 0;
    struct Giveback {                                           // an error on the way returns the pipe at once
        mc_ctx* c; Slot& s; bool armed = true;
        ~Giveback() { if (armed && s.pipe) { (void)hipStreamSynchronize(s.pipe->stream); std::lock_guard<std::mutex> l(c->pipeMtx); c->freePipes.push_back(s.pipe); s.pipe = nullptr; c->pipeCv.notify_one(); } }
    } giveback{ctx, S};
    Pipe& P = *S.pipe;
    hipStream_t st = P.stream;
    if (S.raw) { if (const int rc = raw_parse(ctx, S, st)) return rc; }   // (the reads are cut on the device, into the slot's device input)
    const uint32_t n = S.nq;
    S.submittedQueries = n;
    if (n == 0) { HIP_TRY(ctx, hipEventRecord(S.done, st)); S.submitted = true; return MC_OK; }
    const uint64_t te0 = trace_now();
    if (!S.raw) {
    HIP_TRY(ctx, hipMemcpyAsync(S.dseq, S.hseq, S.nchars + 16, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(S.dqinfo, S.hqinfo, (size_t)n * 16, hipMemcpyHostToDevice, st));
    HIP_TRY(ctx, hipMemcpyAsync(S.dmaxwin, S.hmaxwin, (size_t)n * 4, hipMemcpyHostToDevice, st));
    note_enqueues(trace_now() - te0, 3);
    }
    mc_device_batch in{S.dseq, S.dqinfo, S.dmaxwin, 0, n, S.nchars};
    mc_device_results res{};
    const int wantAll = ctx->cfg.copy_allhits ? 1 : 0;
    const uint64_t tt2 = g_submitTrace ? trace_now() : 0;
    int rc = query_on_pipe(ctx, P, &in, lowestRank, wantAll | slot_query_flags(S.maxSingle), &res, st);
    if (rc) return rc;
    const uint64_t tt3 = g_submitTrace ? trace_now() : 0;
    deliver_slot(ctx, S, P, res, n, st);
    if (wantAll) {
        HIP_TRY(ctx, hipMemcpyAsync(S.hhitoff, res.hit_offsets, (size_t)(n + 1) * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(ctx, traced_sync(st));
        const uint64_t total = S.hhitoff[n];
        if (total > S.hhitsCap) {
            if (S.hhits) HIP_TRY(ctx, hipHostFree(S.hhits));
            S.hhits = nullptr; S.hhitsCap = 0;
            HIP_TRY(ctx, hipHostMalloc((void**)&S.hhits, (total + total / 4 + 64) * sizeof(mc_location)));
            S.hhitsCap = total + total / 4 + 64;
        }
        if (total) HIP_TRY(ctx, hipMemcpyAsync(S.hhits, res.hits, total * sizeof(mc_location), hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(ctx, hipEventRecord(S.done, st));
    if (g_submitTrace) { const uint64_t tt4 = trace_now(); g_trace[0] += tt1 - tt0; g_trace[1] += tt2 - tt1; g_trace[2] += tt3 - tt2; g_trace[4] += tt4 - tt3; ++g_trace[5]; }
    S.submitted = true;
    giveback.armed = false;                                     // mc_batch_wait returns the pipe
    return MC_OK;
}

// ---- slot coalescer -----------------------------------------------------------------------------------------------------------------
// The reference's consumer threads submit batches of 4 096 reads (options.hpp:229-232) and order their submissions with a mutex
// (database_query.hpp:110-113).  Here a batch of that size is ~30 kernel launches and three host round trips for ~0.1 ms of device
// work: one batch per slot keeps the device waiting for the host.  So submissions are QUEUED, and a few dispatcher threads -- a pipe
// each -- take whatever is waiting (same lowest rank, up to coMaxQueries reads) as ONE device batch: every slot's characters go to
// their place in the united input (an H2D each, out of the slot's pinned buffer), the qinfo rows are rebased on the host, one
// query_on_pipe, and every slot's candidates and statistics come back into its own pinned buffers (`done` behind them).  Under load
// the united batches grow by themselves; a lone submitter pays a thread hand-over (~20 us).  Only these threads make HIP calls for
// the slots -- dozens of host threads enqueueing on eight streams is what sends the runtime's direct dispatch into its slow state.
// takes what is waiting (front of the queue, one lowest rank, up to the united batch's limits); coMu held
static void co_take(mc_ctx* ctx, std::vector<uint32_t>& mine, int& lowest)
{
    uint64_t nq = 0, nc = 0;
    lowest = ctx->slots[ctx->coPending.front()].coLowest;
    while (!ctx->coPending.empty()) {
        Slot& S = ctx->slots[ctx->coPending.front()];
        if (!mine.empty() && (S.coLowest != lowest || nq + S.nq > ctx->coMaxQueries || nc + S.nchars + 16 > ctx->coMaxChars)) break;
        nq += S.nq; nc += S.nchars;
        S.coState = 2;
        mine.push_back(ctx->coPending.front());
        ctx->coPending.pop_front();
    }
    ctx->coBatches++; ctx->coSlots += mine.size();
}
static void co_dispatch(mc_ctx* ctx, mcamd::CoDispatcher*)
{
    (void)hipSetDevice(ctx->device);
    std::vector<uint32_t> mine;
    for (;;) {
        mine.clear();
        int lowest = 0;
        mcamd::CoDispatcher* D = nullptr;
        {
            std::unique_lock<std::mutex> l(ctx->coMu);
            ctx->coCv.wait(l, [&] { return (ctx->coStop && ctx->coPending.empty()) || (!ctx->coPending.empty() && !ctx->coFree.empty()); });
            if (ctx->coPending.empty()) return;                    // (stop: nothing is waiting any more)
            D = ctx->coFree.back(); ctx->coFree.pop_back();
            co_take(ctx, mine, lowest);
        }
        co_run(ctx, D, mine, lowest);
        { std::lock_guard<std::mutex> l(ctx->coMu); ctx->coFree.push_back(D); }
        ctx->coCv.notify_one();                                     // (a pipe is free again: whoever waits for one)
    }
}

// one united batch on D's pipe, by the calling thread: a dispatcher, or the submitter itself when nothing was waiting and a pipe was free
static void co_run(mc_ctx* ctx, mcamd::CoDispatcher* D, const std::vector<uint32_t>& mine, int lowest)
{
    std::string err;
    std::string* const sinkBefore = t_errSink;
    t_errSink = &err;
    Pipe& P = *D->pipe;
    hipStream_t st = P.stream;
    const size_t K = ctx->cfg.max_candidates;
    {
        uint64_t nq = 0, nc = 0;
        uint32_t maxSingle = 0;
        for (uint32_t s : mine) { nq += ctx->slots[s].nq; nc += ctx->slots[s].nchars; }
        int rc = MC_OK;
        err.clear();
        const uint32_t k = D->turn++ & 1u;
        auto hip = [&](hipError_t e, const char* what) { if (e != hipSuccess && !rc) { rc = MC_ERR_HIP; err = std::string(what) + ": " + hipGetErrorString(e); } };
        if (D->stagedUsed[k]) hip(hipEventSynchronize(D->staged[k]), "hipEventSynchronize");   // (two united batches ago: long through)
        if (!rc) rc = ensure(ctx, D->dseq, nc + 64);
        if (!rc) rc = ensure(ctx, D->dqinfo, nq * 20);
        if (!rc) {
            const uint64_t ttA = g_submitTrace ? trace_now() : 0;
            uint64_t qb = 0, cb = 0, enq = 0;
            // the rows of the queries and their window limits in ONE pinned buffer and one copy: [nq x 16 bytes | nq x 4 bytes]
            uint32_t* hq = D->hq[k]; uint32_t* hmw = hq + nq * 4;
            for (uint32_t s : mine) {
                Slot& S = ctx->slots[s];
                const bool last = s == mine.back();
                if (last) std::memset(S.hseq + S.nchars, 0, 16);   // (the united input ends with 16 zero bytes: they travel with the last slot's characters)
                const uint64_t te0 = trace_now();
                hip(hipMemcpyAsync((uint8_t*)D->dseq.p + cb, S.hseq, S.nchars + (last ? 16 : 0), hipMemcpyHostToDevice, st), "hipMemcpyAsync");
                enq += trace_now() - te0;
                if (S.maxSingle > maxSingle) maxSingle = S.maxSingle;
                for (uint32_t j = 0; j < S.nq; ++j) {
                    const uint32_t* q = S.hqinfo + (size_t)j * 4;
                    uint32_t* o = hq + (qb + j) * 4;
                    o[0] = q[0] + (uint32_t)cb; o[1] = q[1]; o[2] = q[2] + (uint32_t)cb; o[3] = q[3];
                }
                std::memcpy(hmw + qb, S.hmaxwin, (size_t)S.nq * 4);
                qb += S.nq; cb += S.nchars;
            }
            hip(hipMemcpyAsync(D->dqinfo.p, hq, nq * 20, hipMemcpyHostToDevice, st), "hipMemcpyAsync");
            hip(hipEventRecord(D->staged[k], st), "hipEventRecord");
            D->stagedUsed[k] = true;
            note_enqueues(enq, (uint32_t)mine.size());
            if (g_submitTrace) g_trace[1] += trace_now() - ttA;
        }
        mc_device_results res{};
        if (!rc) {
            mc_device_batch in{(const uint8_t*)D->dseq.p, (const uint32_t*)D->dqinfo.p, (const uint32_t*)D->dqinfo.p + nq * 4, 0, (uint32_t)nq, nc};
            // (MC_SLOT_DEFER=1: deferred tail, finished at once -- the main kernels go out without a look at the work lists' counters: two
            // host round trips less per united batch, every kernel of the path launched whether it has work or not.  Measured at 4 096
            // reads per slot, 32 threads: 4 019 against 4 189 Mreads/min for the synchronous call, profiles/r06_slot_path.json: off)
            static const bool defer = [] { const char* e = std::getenv("MC_SLOT_DEFER"); return e && e[0] == '1'; }();
            const uint64_t ttB = g_submitTrace ? trace_now() : 0;
            rc = query_on_pipe(ctx, P, &in, lowest, (defer ? MC_DEFER_TAIL : 0) | slot_query_flags(maxSingle), &res, st);
            if (!rc && defer) rc = finish_on_pipe(ctx, P);
            if (g_submitTrace) { g_trace[2] += trace_now() - ttB; ++g_trace[5]; }
        }
        if (!rc) {
            const uint64_t ttC = g_submitTrace ? trace_now() : 0;
            // every slot's candidates and statistics into its own pinned buffers: one kernel per sixteen slots (launch_deliver) -- two copies
            // per slot at ~15 us each were half a united batch's time on the stream --, then the slots' events behind it
            uint64_t qb = 0;
            DeliverTable dt{};
            for (uint32_t s : mine) {
                Slot& S = ctx->slots[s];
                dt.e[dt.n++] = DeliverEntry{S.hcands, S.hqstat, (uint32_t)qb, S.nq};
                if (dt.n == kDeliverMax) { launch_deliver(dt, res.cands, P.bQstat.p, (uint32_t)K, st); dt.n = 0; }
                qb += S.nq;
            }
            launch_deliver(dt, res.cands, P.bQstat.p, (uint32_t)K, st);
            hip(hipGetLastError(), "deliver_kernel");
            hipEvent_t ev = D->done[D->doneTurn++ & 3u];
            hip(hipEventRecord(ev, st), "hipEventRecord");
            for (uint32_t s : mine) ctx->slots[s].coDoneEv = ev;
            if (g_submitTrace) g_trace[4] += trace_now() - ttC;
        }
        if (rc) (void)hipStreamSynchronize(st);                     // (whatever was enqueued is through before the slots' buffers go back to their owners)
        {
            std::lock_guard<std::mutex> l(ctx->coMu);
            for (uint32_t s : mine) { Slot& S = ctx->slots[s]; S.coRc = rc; S.coErr = err; S.coEvent = rc == MC_OK; S.coState = 3; }
        }
        ctx->coDoneCv.notify_all();
    }
    t_errSink = sinkBefore;
}

// a raw slot of a context whose slots are united: it goes alone, on a dispatcher's pipe that the submitter borrows, and is THROUGH when
// this returns (its reads are known only after the device has cut them: there is nothing to unite it by)
static int submit_raw_coalesced(mc_ctx* ctx, Slot& S, int lowestRank)
{
    mcamd::CoDispatcher* D = nullptr;
    {
        std::unique_lock<std::mutex> l(ctx->coMu);
        while (ctx->coFree.empty()) ctx->coCv.wait_for(l, std::chrono::microseconds(200));   // (coCv wakes ONE waiter, which may be a dispatcher: look again)
        D = ctx->coFree.back(); ctx->coFree.pop_back();
    }
    Pipe& P = *D->pipe;
    hipStream_t st = P.stream;
    int rc = raw_parse(ctx, S, st);
    const uint32_t n = S.nq;
    if (!rc && n) {
        mc_device_batch in{S.dseq, S.dqinfo, S.dmaxwin, 0, n, S.nchars};
        mc_device_results res{};
        rc = query_on_pipe(ctx, P, &in, lowestRank, slot_query_flags(S.maxSingle), &res, st);
        if (!rc) deliver_slot(ctx, S, P, res, n, st);
    }
    const hipError_t e = hipStreamSynchronize(st);
    if (!rc && e != hipSuccess) rc = fail(ctx, MC_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
    { std::lock_guard<std::mutex> l(ctx->coMu); ctx->coFree.push_back(D); }
    ctx->coCv.notify_one();
    if (rc) return rc;
    S.submittedQueries = n; S.coRc = MC_OK; S.coEvent = false; S.coErr.clear();
    { std::lock_guard<std::mutex> l(ctx->coMu); S.coState = 3; }
    S.submitted = true;
    return MC_OK;
}

static void release_pipe(mc_ctx* ctx, Slot& S)
{
    if (!S.pipe) return;
    std::lock_guard<std::mutex> l(ctx->pipeMtx);
    ctx->freePipes.push_back(S.pipe);
    S.pipe = nullptr;
    ctx->pipeCv.notify_one();
}

int mc_batch_wait(mc_ctx* ctx, uint32_t slot, mc_results* out)
{
    if (!ctx || slot >= ctx->slots.size() || !out) return MC_ERR_INVALID;
    Slot& S = ctx->slots[slot];
    if (!S.submitted) return fail(ctx, MC_ERR_STATE, "mc_batch_wait: slot not submitted");
    if (ctx->coalesce) {
        { std::unique_lock<std::mutex> l(ctx->coMu); ctx->coDoneCv.wait(l, [&] { return S.coState == 3; }); }
        if (S.coRc) return fail(ctx, S.coRc, S.coErr);
        if (S.coEvent) HIP_TRY(ctx, hipEventSynchronize(S.coDoneEv));
    } else
    HIP_TRY(ctx, hipEventSynchronize(S.done));
    release_pipe(ctx, S);                                       // the results are in the slot's pinned buffers
    const uint32_t n = S.submittedQueries;
    int status = MC_OK;
    for (uint32_t i = 0; i < n; ++i) {
        S.hhitcounts[i] = S.hqstat[i].hits;
        if (S.hqstat[i].hits > kMaxHitsPerQuery) status = MC_ERR_UNSUPPORTED;
    }
    out->num_queries = n;
    out->max_candidates = ctx->cfg.max_candidates;
    out->cands = S.hcands;
    out->hit_counts = S.hhitcounts;
    out->hit_offsets = ctx->cfg.copy_allhits ? S.hhitoff : nullptr;
    out->hits = ctx->cfg.copy_allhits ? S.hhits : nullptr;
    if (status) return fail(ctx, status, "a query produced more than 2^20-1 location hits (unsupported)");
    return MC_OK;
}

const char* mc_runtime_warning(void)
{
    static thread_local std::string copy;
    { std::lock_guard<std::mutex> l(g_warnMu); copy = g_warning; }
    return copy.c_str();
}

int mc_slot_stats(mc_ctx* ctx, uint64_t stats[4])
{
    if (!ctx || !stats) return MC_ERR_INVALID;
    std::lock_guard<std::mutex> l(ctx->coMu);
    stats[0] = ctx->coalesce ? 1 : 0; stats[1] = ctx->coBatches; stats[2] = ctx->coSlots; stats[3] = ctx->coDisp.size();
    return MC_OK;
}

int mc_batch_clear(mc_ctx* ctx, uint32_t slot)
{
    if (!ctx || slot >= ctx->slots.size()) return MC_ERR_INVALID;
    Slot& S = ctx->slots[slot];
    if (S.submitted && ctx->coalesce) {
        { std::unique_lock<std::mutex> l(ctx->coMu); ctx->coDoneCv.wait(l, [&] { return S.coState == 3; }); }
        if (S.coEvent) (void)hipEventSynchronize(S.coDoneEv);
        S.coState = 0; S.coEvent = false;
    } else if (S.submitted) (void)hipEventSynchronize(S.done);
    release_pipe(ctx, S);
    S.submitted = false; S.nq = 0; S.nchars = 0; S.maxSingle = 0;
    S.raw = false; S.rawBytes = 0; S.rawBytes2 = 0; S.rawDev = nullptr;
    return MC_OK;
}

}  // extern "C"

// every slot pipe sized for a full slot of reads of the usual length (see size_pipe): called by mc_open_database from a thread of its own
// once the table is announced; `locs` / `keys`: the part headers' counts
int mcamd::reserve_slot_pipes(mc_ctx* ctx, uint64_t locs, uint64_t keys, bool waitForStores)
{
    if (!ctx || ctx->pipes.empty() || ctx->parts.empty()) return MC_OK;
    if (hipSetDevice(ctx->device) != hipSuccess) return MC_ERR_HIP;
    t_quietErrors = true;                                        // (the loader thread owns ctx->err)
    // The table comes first: a single-part table's location store is allocated when the index pass is through (announce_store /
    // allocate_values), and on a device the table nearly fills the pipes must not have taken its memory by then.
    for (; waitForStores;) {
        if (ctx->loadSettled.load(std::memory_order_acquire)) break;
        if (ctx->storesPlaced.load(std::memory_order_acquire) >= ctx->parts.size()) break;
        std::this_thread::sleep_for(std::chrono::microseconds(500));
    }
    const SketchParams sp = ctx->querySketch;
    const uint32_t K = ctx->cfg.max_candidates, n = ctx->coalesce ? ctx->coMaxQueries : ctx->cfg.slot_max_queries;   // (coalescer: a dispatcher's pipe takes a united batch)
    const bool lanePath = lane_path_takes(lane_path_supported(sp), lane_candidates_supported(K), ctx->useLanePath, query_wants(ctx->cfg.copy_allhits ? MC_WANT_ALLHITS : 0));
    // (a slot of short reads: 152 characters each -- a slot filled with longer reads has fewer of them and grows its buffers as before)
    const uint64_t chars = std::min<uint64_t>(ctx->coalesce ? ctx->coMaxChars : ctx->cfg.slot_max_chars, (uint64_t)n * 152);
    int rc = MC_OK;
    for (Pipe* P : ctx->pipes) {
        PipeSizes sz{};
        if ((rc = size_pipe(ctx, *P, n, chars, false, lanePath, locs, keys, sz))) break;
    }
    t_quietErrors = false;
    return rc;
}
// the same for the context's own two pipes (mc_query_device with and without MC_SECOND_PIPE): the part set driver sizes them for its batches
// right after a part has loaded -- on the group loader's thread, beside the other parts' loads -- instead of inside the first batches
int mcamd::reserve_query_pipes(mc_ctx* ctx, uint32_t n, uint64_t chars)
{
    if (!ctx || ctx->parts.empty() || !ctx->tableReady) return MC_OK;
    const SketchParams sp = ctx->querySketch;
    const bool lanePath = lane_path_takes(lane_path_supported(sp), lane_candidates_supported(ctx->cfg.max_candidates), ctx->useLanePath, QueryWants{});   // (whatever the calls will want)
    uint64_t locs = 0;
    for (auto& p : ctx->parts) locs += p.locations;
    for (Pipe* P : {&ctx->pipe0, &ctx->pipe1}) {
        PipeSizes sz{};
        hipStream_t st = nullptr;
        if (const int rc = enter_pipe(ctx, *P, nullptr, st)) return rc;
        if (const int rc = size_pipe(ctx, *P, n, chars, false, lanePath, locs, ctx->parts[0].keysStored, sz)) return rc;
    }
    return MC_OK;
}
