// tests/cpp/kernel_harness.hip -- TEST INFRASTRUCTURE, not product: drives the sorted path's device stages (launch_scan_u32,
// launch_gw_order, launch_gw_segsort, gw_sorted_cands_kernel through launch_big_cands) with inputs a test chooses, through the internal
// launcher interface of csrc/kernels.h.  Built into metacache_amd/lib/libmckharness.so beside libmetacache_amd.so, which it links; it
// holds no kernels of its own and the product library gets no entry point for it (tests/kernel_harness.py is the ctypes side).
//
// Every entry point takes HOST arrays: it validates them on the host FIRST and returns a KH_ERR_* code without any device call if a
// check fails (a mistake in a test must never become a device fault), then allocates device buffers, uploads, runs on a stream of its
// own, synchronises, downloads and frees.
#include "kernels.h"
#include "device_common.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <vector>

using namespace mcamd;

extern "C" {

enum KhError : int {
    KH_OK = 0,
    KH_ERR_HIP = 1,        // a device call failed (no device: every entry point that passed validation ends here)
    KH_ERR_ARG = 2,        // null pointer, nothing wanted, stride 0, sizes out of the harness's limits
    KH_ERR_COUNT = 3,      // nlists == 0 or nlists > n
    KH_ERR_LENGTH = 4,     // a list of 0 or more than kGwMaxKept numbers
    KH_ERR_RANGE = 5,      // offset + length beyond the pool
    KH_ERR_OVERLAP = 6,    // two lists share pool words
    KH_ERR_PADDING = 7,    // a number equals 0xFFFFFFFF (the sort's padding)
    KH_ERR_WINDOW = 8,     // a number outside every target's windows (in a gap, or beyond gwBase[targets])
    KH_ERR_ORDER = 9,      // a list that is not ascending
    KH_ERR_MAXWIN = 10,    // maxWin == 0 or maxWin > gap
    KH_ERR_K = 11,         // K == 0 or K > 4
    KH_ERR_QUERY = 12,     // q >= n, or two lists with the same q
    KH_ERR_TABLE = 13      // no targets, gap below 8, or the window numbers do not fit 32 bits
};

}  // extern "C"

namespace {

constexpr uint64_t kMaxBatch = 1u << 22, kMaxPool = 1u << 28, kMaxScan = 1u << 26;   // the harness's own limits (far above what the tests use)

// device buffers and the streams / events of one call: freed on every way out
struct Scope {
    std::vector<void*> dev, pinned;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> events;
    bool failed = false;
    template <class T> T* alloc(size_t count)
    {
        void* p = nullptr;
        if (hipMalloc(&p, std::max<size_t>(count, 1) * sizeof(T) + 256) != hipSuccess) { failed = true; return nullptr; }
        dev.push_back(p);
        return static_cast<T*>(p);
    }
    template <class T> T* upload(const T* host, size_t count)
    {
        T* p = alloc<T>(count);
        if (p && count && hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) failed = true;
        return p;
    }
    template <class T> T* filled(size_t count, int byte)
    {
        T* p = alloc<T>(count);
        if (p && hipMemset(p, byte, std::max<size_t>(count, 1) * sizeof(T)) != hipSuccess) failed = true;
        return p;
    }
    template <class T> void download(T* host, const T* devp, size_t count)
    {
        if (host && count && hipMemcpy(host, devp, count * sizeof(T), hipMemcpyDeviceToHost) != hipSuccess) failed = true;
    }
    // uploads and fills go through the null stream, the launches through a stream that does not wait for it: everything that was
    // uploaded or filled is in place before the first launch
    bool ready() { if (hipDeviceSynchronize() != hipSuccess) failed = true; return !failed; }
    hipStream_t stream()
    {
        hipStream_t s = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess) { failed = true; return nullptr; }
        streams.push_back(s);
        return s;
    }
    hipEvent_t event()
    {
        hipEvent_t e = nullptr;
        if (hipEventCreateWithFlags(&e, hipEventDisableTiming) != hipSuccess) { failed = true; return nullptr; }
        events.push_back(e);
        return e;
    }
    ~Scope()
    {
        for (hipStream_t s : streams) (void)hipStreamDestroy(s);
        for (hipEvent_t e : events) (void)hipEventDestroy(e);
        for (void* p : dev) (void)hipFree(p);
        for (void* p : pinned) (void)hipHostFree(p);
    }
};

// the checks every list call shares: counts, lengths, pool range, overlap, padding
int check_lists(uint32_t n, uint32_t nlists, const uint32_t* lengths, const uint32_t* offsets, const uint32_t* pool, uint64_t poolWords)
{
    if (n == 0 || n > kMaxBatch || poolWords == 0 || poolWords > kMaxPool) return KH_ERR_ARG;
    if (nlists == 0 || nlists > n) return KH_ERR_COUNT;
    if (!lengths || !offsets || !pool) return KH_ERR_ARG;
    for (uint32_t i = 0; i < nlists; ++i) {
        if (lengths[i] == 0 || lengths[i] > kGwMaxKept) return KH_ERR_LENGTH;
        if ((uint64_t)offsets[i] + lengths[i] > poolWords) return KH_ERR_RANGE;
    }
    std::vector<uint32_t> byOff(nlists);
    std::iota(byOff.begin(), byOff.end(), 0u);
    std::sort(byOff.begin(), byOff.end(), [&](uint32_t a, uint32_t b) { return offsets[a] < offsets[b]; });
    for (uint32_t i = 0; i + 1 < nlists; ++i)
        if ((uint64_t)offsets[byOff[i]] + lengths[byOff[i]] > offsets[byOff[i + 1]]) return KH_ERR_OVERLAP;
    for (uint32_t i = 0; i < nlists; ++i)
        for (uint32_t j = 0; j < lengths[i]; ++j)
            if (pool[(size_t)offsets[i] + j] == 0xFFFFFFFFu) return KH_ERR_PADDING;
    return KH_OK;
}

// The compact store's numbering, as the context lays it out when a database is opened: gwBase[0] = gap, gwBase[t + 1] = gwBase[t] +
// windows(t) + gap, and the directory dir[blk] = the target whose numbers (gap included) hold max(blk << shift, gap).
int gw_layout(uint32_t targets, const uint32_t* windows, uint32_t gap, std::vector<uint32_t>& base, uint32_t& shift, std::vector<uint32_t>& dir)
{
    if (!windows || targets == 0 || gap < 8) return KH_ERR_TABLE;
    uint64_t total = gap;
    for (uint32_t t = 0; t < targets; ++t) total += (uint64_t)windows[t] + gap;
    if (total >= 0xFFFFFFFFull) return KH_ERR_TABLE;
    base.assign((size_t)targets + 1, 0u);
    base[0] = gap;
    for (uint32_t t = 0; t < targets; ++t) base[t + 1] = base[t] + windows[t] + gap;
    shift = 6;
    while (((total >> shift) + 2) > (1ull << 22)) ++shift;
    const size_t nd = (size_t)(total >> shift) + 2;
    dir.assign(nd, 0u);
    size_t t = 0;
    for (size_t blk = 0; blk < nd; ++blk) {
        const uint64_t g = std::max<uint64_t>((uint64_t)blk << shift, gap);
        while (t + 1 < targets && g >= base[t + 1]) ++t;
        dir[blk] = (uint32_t)t;
    }
    return KH_OK;
}

// a Workspace that holds only what the order, the sort and the scan of the sorted lists read: the counters, the kListFiltered records
// {q, pool offset, length, maxWin} and the kSideSorted row
struct SortedWork {
    Workspace ws{};
    int build(Scope& S, uint32_t n, uint32_t nlists, const uint32_t* lengths, const uint32_t* offsets, const uint32_t* q, const uint32_t* maxWin)
    {
        std::vector<uint32_t> counters(kCounterWords, 0u);
        counters[kCntSorted] = nlists;
        std::vector<uint4> lists((size_t)kWorkLists * n, make_uint4(0u, 0u, 0u, 0u));
        std::vector<uint32_t> side((size_t)kSideRows * n, 0u);
        for (uint32_t i = 0; i < nlists; ++i) {
            lists[list_at(kListFiltered, n) + i] = make_uint4(q ? q[i] : i, offsets[i], lengths[i], maxWin ? maxWin[i] : 1u);
            side[list_at(kSideSorted, n) + i] = i;
        }
        // counters + lists in one buffer, as work_lists_bytes lays them out
        char* buf = S.alloc<char>(work_lists_bytes(n));
        if (!buf) return KH_ERR_HIP;
        if (hipMemcpy(buf, counters.data(), kCounterBytes, hipMemcpyHostToDevice) != hipSuccess ||
            hipMemcpy(buf + kCounterBytes, lists.data(), lists.size() * sizeof(uint4), hipMemcpyHostToDevice) != hipSuccess) return KH_ERR_HIP;
        ws.midCount = reinterpret_cast<uint32_t*>(buf);
        ws.midList = reinterpret_cast<uint4*>(buf + kCounterBytes);
        ws.sideList = S.upload(side.data(), side.size());
        return S.failed ? KH_ERR_HIP : KH_OK;
    }
    // the side list longest first (query_pipe.cpp run_sorted_tail: size query, then 3 n words + the order's own bytes)
    int order(Scope& S, uint32_t n, uint32_t nseg, hipStream_t st)
    {
        size_t ordBytes = 0;
        if (launch_gw_order(kSideSorted, ws, n, nseg, nullptr, ordBytes, st) != 0) return KH_ERR_HIP;
        uint32_t* scratch = S.alloc<uint32_t>((size_t)3 * n + ordBytes / 4 + 64);
        if (!scratch) return KH_ERR_HIP;
        return launch_gw_order(kSideSorted, ws, n, nseg, scratch, ordBytes, st) != 0 ? KH_ERR_HIP : KH_OK;
    }
};

}  // namespace

extern "C" {

// {kGwMaxKept, kGwGap, kFlagDone, kFlagCands, kCntSorted, kCntSortedBig, kCounterWords, kSideSorted}
void kh_constants(uint32_t out[8])
{
    const uint32_t c[8] = {kGwMaxKept, kGwGap, kFlagDone, kFlagCands, kCntSorted, kCntSortedBig, kCounterWords, (uint32_t)kSideSorted};
    std::memcpy(out, c, sizeof c);
}

// ---- the launchers' host-only size queries (no device call) -----------------------------------------------------------------------
uint64_t kh_scan_tmp_bytes(uint32_t n) { return scan_tmp_bytes(n); }
uint64_t kh_order_temp_bytes(uint32_t n, uint32_t count)
{
    size_t bytes = 0;
    Workspace ws{};
    return launch_gw_order(kSideSorted, ws, n, count, nullptr, bytes, nullptr) == 0 ? bytes : 0;
}
uint64_t kh_segsort_temp_bytes(uint32_t n, uint32_t nseg, uint64_t poolCap)
{
    size_t bytes = 0;
    Workspace ws{};
    return launch_gw_segsort(nullptr, bytes, nullptr, nullptr, poolCap, ws, n, nseg, 32u, nullptr) == 0 ? bytes : 0;
}

// gwBase[targets + 1], the directory and its shift for `targets` targets of windows[t] windows; dir == nullptr or dirCap too small: only
// the directory's length comes back (0: the layout is refused)
uint64_t kh_gw_layout(uint32_t targets, const uint32_t* windows, uint32_t gap, uint32_t* baseOut, uint32_t* shiftOut, uint32_t* dirOut, uint64_t dirCap)
{
    std::vector<uint32_t> base, dir;
    uint32_t shift = 0;
    if (gw_layout(targets, windows, gap, base, shift, dir) != KH_OK) return 0;
    if (baseOut) std::memcpy(baseOut, base.data(), base.size() * 4);
    if (shiftOut) *shiftOut = shift;
    if (dirOut && dirCap >= dir.size()) std::memcpy(dirOut, dir.data(), dir.size() * 4);
    return dir.size();
}

// ---- launch_scan_u32: exclusive scan of in[i * stride], i < n -> out32[n + 1], out64[n + 1], the grand total in pinned host memory ------
int kh_scan(const uint32_t* in, uint32_t stride, uint32_t n, int want32, int want64, int wantHost, uint32_t* out32, uint64_t* out64, uint64_t* hostTotal)
{
    if (stride == 0 || (!want32 && !want64) || (n && !in) || (want32 && !out32) || (want64 && !out64) || (wantHost && !hostTotal)) return KH_ERR_ARG;
    if ((uint64_t)n * stride > kMaxScan) return KH_ERR_ARG;
    Scope S;
    const size_t words = (size_t)n * stride;
    uint32_t* dIn = S.upload(in, words);
    uint32_t* d32 = want32 ? S.filled<uint32_t>((size_t)n + 1, 0xA5) : nullptr;
    uint64_t* d64 = want64 ? S.filled<uint64_t>((size_t)n + 1, 0xA5) : nullptr;
    char* tmp = S.alloc<char>(scan_tmp_bytes(n));
    uint64_t* pinned = nullptr;
    if (wantHost) {
        if (hipHostMalloc((void**)&pinned, 128) != hipSuccess) return KH_ERR_HIP;
        S.pinned.push_back(pinned);
        *pinned = 0xA5A5A5A5A5A5A5A5ull;
    }
    hipStream_t st = S.stream();
    if (!S.ready()) return KH_ERR_HIP;
    launch_scan_u32(dIn, stride, n, d32, d64, tmp, st, pinned);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return KH_ERR_HIP;
    S.download(out32, d32, want32 ? (size_t)n + 1 : 0);
    S.download(out64, d64, want64 ? (size_t)n + 1 : 0);
    if (wantHost) *hostTotal = *pinned;
    return S.failed ? KH_ERR_HIP : KH_OK;
}

// ---- launch_gw_order + launch_gw_segsort: nlists lists (lengths[i] numbers at pool[offsets[i]]) of a batch of n reads ----------------
// sideOut[nlists]: the kSideSorted row after ordering (list numbers); sortedOut[poolWords]: the sort's output buffer, which starts as a
// copy of the pool (so the words outside every list must come back as they went in); poolAfter[poolWords] (may be null): the input pool
// after the run.
int kh_order_sort(uint32_t n, uint32_t nlists, const uint32_t* lengths, const uint32_t* offsets, const uint32_t* pool, uint64_t poolWords,
                  int secondStream, uint32_t* sideOut, uint32_t* sortedOut, uint32_t* poolAfter)
{
    if (!sideOut || !sortedOut) return KH_ERR_ARG;
    if (const int rc = check_lists(n, nlists, lengths, offsets, pool, poolWords)) return rc;
    Scope S;
    SortedWork W;
    if (const int rc = W.build(S, n, nlists, lengths, offsets, nullptr, nullptr)) return rc;
    uint32_t* dIn = S.upload(pool, poolWords);
    uint32_t* dOut = S.upload(pool, poolWords);
    hipStream_t st = S.stream();
    GwSortSide side2;
    if (secondStream) { side2.stream = S.stream(); side2.fork = S.event(); side2.join = S.event(); }
    if (!S.ready()) return KH_ERR_HIP;
    const uint32_t nseg = std::min(nlists, n);
    if (const int rc = W.order(S, n, nseg, st)) return rc;
    size_t tmpBytes = 0;
    if (launch_gw_segsort(nullptr, tmpBytes, dIn, dOut, poolWords, W.ws, n, nseg, 32u, st) != 0) return KH_ERR_HIP;
    char* tmp = S.alloc<char>(tmpBytes + 256);
    if (!tmp) return KH_ERR_HIP;
    if (launch_gw_segsort(tmp, tmpBytes, dIn, dOut, poolWords, W.ws, n, nseg, 32u, st, secondStream ? &side2 : nullptr) != 0) return KH_ERR_HIP;
    if (hipStreamSynchronize(st) != hipSuccess || (side2.stream && hipStreamSynchronize(side2.stream) != hipSuccess)) return KH_ERR_HIP;
    S.download(sideOut, W.ws.sideList + list_at(kSideSorted, n), nlists);
    S.download(sortedOut, dOut, poolWords);
    S.download(poolAfter, dIn, poolWords);
    return S.failed ? KH_ERR_HIP : KH_OK;
}

// ---- gw_sorted_cands_kernel (both instances) through launch_big_cands(FilterStep::SortedCands) ----------------------------------------
// The lists are SORTED global window numbers of the layout (targets, windows[], gap); list i belongs to read q[i] (distinct, < n) with
// window range maxWin[i] and qstat.hits qhits[i].  taxkey: [targets] or null.  Out: cands[n][K][4] {tgt, hits, beg, end} (0xFF bytes
// where the kernels wrote nothing), qflag[n] and hitScan[n] (0xA5 bytes likewise), *sortedBig = midCount[kCntSortedBig].
int kh_sorted_cands(uint32_t n, uint32_t nlists, const uint32_t* lengths, const uint32_t* offsets, const uint32_t* pool, uint64_t poolWords,
                    const uint32_t* maxWin, const uint32_t* q, const uint32_t* qhits, uint32_t targets, const uint32_t* windows, uint32_t gap,
                    uint32_t K, const uint32_t* taxkey, uint32_t* candsOut, uint32_t* qflagOut, uint32_t* hitScanOut, uint32_t* sortedBig)
{
    if (!maxWin || !q || !qhits || !candsOut || !qflagOut || !hitScanOut || !sortedBig) return KH_ERR_ARG;
    if (const int rc = check_lists(n, nlists, lengths, offsets, pool, poolWords)) return rc;
    if (K == 0 || K > kLaneK) return KH_ERR_K;
    std::vector<uint32_t> base, dir;
    uint32_t shift = 0;
    if (const int rc = gw_layout(targets, windows, gap, base, shift, dir)) return rc;
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t i = 0; i < nlists; ++i) {
        if (q[i] >= n || seen[q[i]]) return KH_ERR_QUERY;
        seen[q[i]] = 1;
        if (maxWin[i] == 0 || maxWin[i] > gap) return KH_ERR_MAXWIN;
        const uint32_t* g = pool + offsets[i];
        for (uint32_t j = 0; j < lengths[i]; ++j) {
            if (j && g[j] < g[j - 1]) return KH_ERR_ORDER;
            // the target whose numbers (gap behind it included) hold g[j]: the last t with base[t] <= g[j]
            const size_t t = (size_t)(std::upper_bound(base.begin(), base.end(), g[j]) - base.begin());
            if (t == 0 || t > targets || g[j] - base[t - 1] >= windows[t - 1]) return KH_ERR_WINDOW;
        }
    }
    Scope S;
    SortedWork W;
    if (const int rc = W.build(S, n, nlists, lengths, offsets, q, maxWin)) return rc;
    Workspace& ws = W.ws;
    ws.bigPool2 = S.upload(pool, poolWords);
    std::vector<QueryStat> qs(n, QueryStat{0u, 0u, 0u, 0u});
    for (uint32_t i = 0; i < nlists; ++i) qs[q[i]].hits = qhits[i];
    ws.qstat = S.upload(qs.data(), qs.size());
    ws.qflag = S.filled<uint32_t>(n, 0xA5);
    ws.hitScan = S.filled<uint32_t>(n, 0xA5);
    mc_candidate_dev* dCands = S.filled<mc_candidate_dev>((size_t)n * K, 0xFF);
    DeviceTable tab{};
    tab.tgtMask = 0xFFFFFFFFu;
    tab.values32 = ws.bigPool2;                                    // (any valid pointer: it selects the gw kernels in launch_big_cands)
    tab.gwBase = S.upload(base.data(), base.size());
    tab.gwDir = S.upload(dir.data(), dir.size());
    tab.gwDirShift = shift; tab.gwGap = gap; tab.gwTargets = targets;
    uint32_t* dTax = taxkey ? S.upload(taxkey, targets) : nullptr;
    hipStream_t st = S.stream();
    if (!S.ready()) return KH_ERR_HIP;
    if (const int rc = W.order(S, n, std::min(nlists, n), st)) return rc;
    BatchView b{};
    b.n = n;
    const SketchParams sp{16u, 16u, 127u, 112u};
    launch_big_cands(FilterStep::SortedCands, b, sp, tab, ws, K, dTax, dCands, st);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return KH_ERR_HIP;
    S.download(candsOut, reinterpret_cast<const uint32_t*>(dCands), (size_t)n * K * 4);
    S.download(qflagOut, ws.qflag, n);
    S.download(hitScanOut, ws.hitScan, n);
    S.download(sortedBig, ws.midCount + kCntSortedBig, 1);
    return S.failed ? KH_ERR_HIP : KH_OK;
}

}  // extern "C"
