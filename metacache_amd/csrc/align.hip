// metacache_amd/csrc/align.hip -- mc_align_semiglobal: the reference's semi-global alignment (alignment.hpp:177-276, the scheme of
// :88-171, the orientation choice of classification.cpp:76-100) for a batch of problems.  A problem is (read 1, optional mate, subject);
// the device returns read 1's score forward and reverse-complemented, the mate's two scores, which orientation won, and the winner's
// two aligned strings.
//
// ONE WAVE PER PROBLEM.  The subject's columns are dealt over the 64 lanes in strips of W columns (lane l: columns l*W .. l*W+W-1), the
// rows are skewed over the lanes: at step r lane l is on row r - l.  What a lane needs from its left neighbour -- the score of that row's
// cell left of its strip, and the row's query character -- comes down the wave by a DPP shift of one lane (wave_shr:1), never through
// memory; the cell above is the lane's own previous row, W registers.  A cell's predecessor is 2 bits (none / diag / above / left as in
// relaxation_result); a lane's strip of one row is 2 W bits, stored as one byte (W <= 4) or two.
//   short tier  len_q <= 256, len_s <= 512: W = ceil(len_s / 64), the predecessor bits live in an LDS slab of the wave's own
//               (len_q x 64 or 128 bytes; 150 x 350 cells: 19 200 bytes), the trace walks the slab.
//   long tier   everything else: W = 8, the subject goes through in panels of 512 columns; a panel's last column travels to the next panel
//               through a row of len_q + 1 numbers in device scratch, the predecessor bits go to device scratch as well (2 bits per cell,
//               a panel's last strip padded).  The host cuts sub-batches so that scratch and output stay under "align_scratch_mb".
// The forward alignment is traced while it is computed; reverse and the mate's two are score-only passes; where reverse wins, it is
// computed once more with its trace (the slab then holds the winner's bits).  Plain HIP C++; no inline assembly.
#include "context.h"

#include <algorithm>
#include <climits>
#include <cstring>

namespace mcamd {

struct AlignWork {                       // what one caller needs on the device; kept by the context between calls
    hipStream_t stream = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    DevBuf dChars, dRes, dScratch;                // input (characters | problems | lists), output (results | aligned strings), the long tier's scratch
    void* hIn = nullptr; size_t hInCap = 0;      // pinned staging: characters + problems + index lists
    void* hOut = nullptr; size_t hOutCap = 0;    // pinned: results + aligned strings
};

}  // namespace mcamd

using namespace mcamd;

namespace {

constexpr uint32_t kShortMaxQ = 256, kShortMaxS = 512, kLongW = 8, kLanes = 64;

struct AlignProblem {
    uint64_t q, m, s;                    // first characters in the sub-batch's character buffer
    uint32_t lenQ, lenM, lenS, hasMate;
    uint64_t out;                        // its 2 x max(1, lenQ + lenS) bytes in the output buffer: aligned query, aligned target, each written from the back
    uint64_t scratch;                    // long tier: its boundary row + predecessor bits in the scratch buffer (byte offset, 128-byte aligned)
};
struct AlignResult { int32_t fwd, rev, mfwd, mrev; uint32_t reversed, length; };

// the value of the lane below (lane 0: fill).  Every lane of the wave must be active.
__device__ __forceinline__ int wave_shr1(int v, int fill) { return __builtin_amdgcn_update_dpp(fill, v, 0x138 /* wave_shr:1 */, 0xF, 0xF, false); }

__device__ __forceinline__ uint8_t complement(uint8_t c)      // dna_encoding.hpp:46-65: case kept, U -> A, everything else as it is
{
    switch (c) {
        case 'A': return 'T'; case 'a': return 't'; case 'C': return 'G'; case 'c': return 'g';
        case 'G': return 'C'; case 'g': return 'c'; case 'T': return 'A'; case 't': return 'a';
        case 'U': return 'A'; case 'u': return 'a'; default: return c;
    }
}
__device__ __forceinline__ uint8_t query_char(const uint8_t* q, uint32_t len, uint32_t i, bool rc) { return rc ? complement(q[len - 1 - i]) : q[i]; }

// where the predecessor bits of a pass go and come from
template <bool LONG> struct PredStore;
template <> struct PredStore<false> {            // LDS: [row][lane], cb bytes each
    uint8_t* slab; uint32_t cb;
    __device__ void put(uint32_t, uint32_t row0, uint32_t lane, uint32_t bits) const
    {
        if (cb == 1) slab[row0 * kLanes + lane] = (uint8_t)bits; else reinterpret_cast<uint16_t*>(slab)[row0 * kLanes + lane] = (uint16_t)bits;
    }
    __device__ uint32_t get(uint32_t, uint32_t row0, uint32_t lane) const
    {
        return cb == 1 ? slab[row0 * kLanes + lane] : reinterpret_cast<const uint16_t*>(slab)[row0 * kLanes + lane];
    }
};
template <> struct PredStore<true> {             // device scratch: [panel][row][lane], 2 bytes each
    uint16_t* bits16; uint32_t lenQ;
    __device__ void put(uint32_t panel, uint32_t row0, uint32_t lane, uint32_t bits) const { bits16[((uint64_t)panel * lenQ + row0) * kLanes + lane] = (uint16_t)bits; }
    __device__ uint32_t get(uint32_t panel, uint32_t row0, uint32_t lane) const
    {
        const uint64_t i = ((uint64_t)panel * lenQ + row0) * kLanes + lane;       // (read past the L1: other lanes of this wave wrote it)
        const uint32_t w = __hip_atomic_load(reinterpret_cast<const uint32_t*>(bits16) + (i >> 1), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        return (w >> ((i & 1) * 16)) & 0xFFFFu;
    }
};

// One alignment's matrix: score and end cell as align_semi_global finds them (alignment.hpp:228-249); with 'trace' the predecessor of
// every cell goes to the store.  W columns per lane and panel; bnd (long tier): len_q + 1 numbers, a panel's last column for the next one.
template <bool LONG>
__device__ void semiglobal_pass(const uint8_t* __restrict__ q, uint32_t lenQ, bool rc, const uint8_t* __restrict__ s, uint32_t lenS, bool trace,
                                const PredStore<LONG>& store, int32_t* bnd, uint32_t W, int& score, uint32_t& endQ, uint32_t& endS)
{
    const uint32_t lane = threadIdx.x;
    const uint32_t panelCols = kLanes * W;
    const uint32_t npanels = (lenS + panelCols - 1) / panelCols;
    int rowBest = INT_MIN, colBest = INT_MIN, endVal = 0;
    uint32_t rowBestS = 0, colBestQ = 0;
    for (uint32_t p = 0; p < npanels; ++p) {
        const uint32_t c0 = p * panelCols;
        const uint32_t cols = min(panelCols, lenS - c0);
        const uint32_t myc0 = lane * W;
        const uint32_t nk = myc0 < cols ? min(W, cols - myc0) : 0u;              // this lane's columns in the panel
        const bool lastPanel = p + 1 == npanels;
        const uint32_t lastLane = (cols - 1) / W;
        uint8_t sub[8]; int prev[8];
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) { sub[k] = k < nk ? s[c0 + myc0 + k] : (uint8_t)0; prev[k] = 0; }
        int mylast = 0, diagIn = 0, qc = 0, qchunk = 0, bchunk = 0;
        const uint32_t steps = lenQ + lastLane;                                  // lane lastLane is on row lenQ then
        for (uint32_t r = 1; r <= steps; ++r) {
            const uint32_t inChunk = (r - 1) & 63u;
            if (inChunk == 0) {                                                  // rows r .. r + 63: lane 0's next 64 query characters (and left neighbours)
                const uint32_t row = r + lane;
                qchunk = row <= lenQ ? (int)query_char(q, lenQ, row - 1, rc) : 0;
                if (LONG && p > 0) bchunk = row <= lenQ ? __hip_atomic_load(bnd + row, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0;
            }
            int leftIn = wave_shr1(mylast, 0);
            int qin = wave_shr1(qc, 0);
            const int q0 = __shfl(qchunk, (int)inChunk);
            const int b0 = (LONG && p > 0) ? __shfl(bchunk, (int)inChunk) : 0;
            if (lane == 0) { qin = q0; leftIn = b0; }
            const int row = (int)r - (int)lane;
            if (nk > 0 && row >= 1 && row <= (int)lenQ) {
                int diag = diagIn, left = leftIn;
                uint32_t bits = 0;
#pragma unroll
                for (uint32_t k = 0; k < 8; ++k) {
                    if (k < nk) {                                                // relax, alignment.hpp:98-122: diag, then above / left only if strictly greater
                        const int up = prev[k];
                        int sc = diag + (qin == (int)sub[k] ? 2 : -1);
                        uint32_t pd = 1;
                        if (up - 1 > sc) { sc = up - 1; pd = 2; }
                        if (left - 1 > sc) { sc = left - 1; pd = 3; }
                        diag = up; prev[k] = sc; left = sc;
                        bits |= pd << (2 * k);
                    }
                }
                mylast = left;
                if (trace) store.put(p, (uint32_t)row - 1, lane, bits);
                if (lastPanel && lane == lastLane) {                             // the matrix's last column: rows 1 .. lenQ - 1 ascending, then the corner
                    if ((uint32_t)row < lenQ) { if (left > colBest) { colBest = left; colBestQ = (uint32_t)row; } }
                    else endVal = left;
                }
                if (LONG && !lastPanel && lane == kLanes - 1) __hip_atomic_store(bnd + row, left, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            diagIn = leftIn; qc = qin;
        }
        // the matrix's last row: columns 1 .. lenS - 1 ascending, the first of the greatest
        int bv = INT_MIN; uint32_t bs = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; ++k) {
            const uint32_t si = c0 + myc0 + k + 1;
            if (k < nk && si < lenS && prev[k] > bv) { bv = prev[k]; bs = si; }
        }
        for (int off = 32; off > 0; off >>= 1) {
            const int ov = __shfl_xor(bv, off); const uint32_t os = (uint32_t)__shfl_xor((int)bs, off);
            if (ov > bv || (ov == bv && os < bs)) { bv = ov; bs = os; }
        }
        if (bv > rowBest) { rowBest = bv; rowBestS = bs; }
        if (lastPanel) { endVal = __shfl(endVal, (int)lastLane); colBest = __shfl(colBest, (int)lastLane); colBestQ = (uint32_t)__shfl((int)colBestQ, (int)lastLane); }
        if (LONG) { __threadfence(); __syncthreads(); }                          // the boundary row is read by this wave's other lanes in the next panel
    }
    score = endVal; endQ = lenQ; endS = lenS;
    if (colBest > score) { score = colBest; endQ = colBestQ; endS = lenS; }
    if (rowBest > score) { score = rowBest; endQ = lenQ; endS = rowBestS; }
}

template <bool LONG>
__global__ void __launch_bounds__(64) align_kernel(const AlignProblem* __restrict__ probs, const uint32_t* __restrict__ list, uint32_t n,
                                                  const uint8_t* __restrict__ chars, uint8_t* __restrict__ out, AlignResult* __restrict__ res,
                                                  uint8_t* __restrict__ scratch)
{
    extern __shared__ __attribute__((aligned(16))) uint8_t slabS[];
    if (blockIdx.x >= n) return;
    const uint32_t pi = list[blockIdx.x];
    const AlignProblem P = probs[pi];
    const uint32_t lane = threadIdx.x;
    const uint8_t* q = chars + P.q; const uint8_t* m = chars + P.m; const uint8_t* s = chars + P.s;
    const uint64_t cap = max((uint64_t)1, (uint64_t)P.lenQ + P.lenS);
    uint8_t* outQ = out + P.out; uint8_t* outT = outQ + cap;
    const uint32_t W = LONG ? kLongW : max(1u, (P.lenS + kLanes - 1) / kLanes);
    PredStore<LONG> store;
    int32_t* bnd = nullptr;
    if constexpr (LONG) {
        bnd = reinterpret_cast<int32_t*>(scratch + P.scratch);
        store.bits16 = reinterpret_cast<uint16_t*>(scratch + P.scratch + (((uint64_t)max(P.lenQ, P.lenM) + 1) * 4 + 127) / 128 * 128);   // (behind the boundary row: host long_scratch)
        store.lenQ = P.lenQ;
    } else { store.slab = slabS; store.cb = W <= 4 ? 1u : 2u; }

    AlignResult R{0, 0, 0, 0, 1, 1};
    if (P.lenQ == 0 || P.lenS == 0) {            // an empty matrix: score 0 both ways (reverse is shown), the trace's do-while gives one column of gaps
        if (P.hasMate && P.lenM > 0 && P.lenS > 0) {
            int sc; uint32_t eq, es;
            semiglobal_pass<LONG>(m, P.lenM, false, s, P.lenS, false, store, bnd, W, sc, eq, es); R.mfwd = sc;
            semiglobal_pass<LONG>(m, P.lenM, true, s, P.lenS, false, store, bnd, W, sc, eq, es); R.mrev = sc;
            R.reversed = !((uint64_t)(int64_t)R.mfwd > (uint64_t)(int64_t)R.mrev);
        }
        if (lane == 0) { outQ[cap - 1] = '_'; outT[cap - 1] = '_'; res[pi] = R; }
        return;
    }
    int sc; uint32_t endQ, endS, eq, es;
    semiglobal_pass<LONG>(q, P.lenQ, false, s, P.lenS, true, store, bnd, W, sc, endQ, endS); R.fwd = sc;
    semiglobal_pass<LONG>(q, P.lenQ, true, s, P.lenS, false, store, bnd, W, sc, eq, es); R.rev = sc;
    if (P.hasMate && P.lenM > 0) {
        semiglobal_pass<LONG>(m, P.lenM, false, s, P.lenS, false, store, bnd, W, sc, eq, es); R.mfwd = sc;
        semiglobal_pass<LONG>(m, P.lenM, true, s, P.lenS, false, store, bnd, W, sc, eq, es); R.mrev = sc;
    }
    // make_semi_global_alignment sums in std::size_t: a negative score wraps (classification.cpp:79-99)
    const uint64_t sumF = (uint64_t)(int64_t)R.fwd + (uint64_t)(int64_t)R.mfwd, sumR = (uint64_t)(int64_t)R.rev + (uint64_t)(int64_t)R.mrev;
    const bool rev = !(sumF > sumR);
    R.reversed = rev;
    if (rev) semiglobal_pass<LONG>(q, P.lenQ, true, s, P.lenS, true, store, bnd, W, sc, endQ, endS);
    __threadfence_block();
    __syncthreads();                             // the predecessor bits are in place for the lane that walks them
    if (lane == 0) {
        uint32_t qi = endQ, si = endS, len = 0;
        const uint32_t panelCols = kLanes * W;
        uint32_t panel = (si - 1) / panelCols, c = (si - 1) % panelCols, l = c / W, k = c % W;
        do {                                     // alignment.hpp:256-268, encode :125-154
            const uint32_t pd = (store.get(panel, qi - 1, l) >> (2 * k)) & 3u;
            uint8_t a = '_', b = '_';
            if (pd != 3) { --qi; a = query_char(q, P.lenQ, qi, rev); }
            if (pd != 2) {
                --si; b = s[si];
                if (k > 0) --k; else { k = W - 1; if (l > 0) --l; else { l = kLanes - 1; --panel; } }
            }
            ++len;
            outQ[cap - len] = a; outT[cap - len] = b;
        } while (qi > 0 && si > 0);
        R.length = len;
        res[pi] = R;
    }
}

int grow_with_headroom(mc_ctx* ctx, DevBuf& b, size_t bytes)      // an eighth more than asked for; no room is MC_ERR_NOMEM
{
    if (bytes <= b.cap) return MC_OK;
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    if (hipMalloc(&b.p, want) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return fail(ctx, MC_ERR_NOMEM, "mc_align_semiglobal: cannot allocate " + std::to_string(want >> 20) + " MB of device memory"); }
    b.cap = want;
    return MC_OK;
}
int grow_host(mc_ctx* ctx, void*& p, size_t& cap, size_t bytes)
{
    if (bytes <= cap) return MC_OK;
    if (p) (void)hipHostFree(p);
    p = nullptr; cap = 0;
    const size_t want = bytes + bytes / 8 + 256;
    if (hipHostMalloc(&p, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return fail(ctx, MC_ERR_NOMEM, "mc_align_semiglobal: cannot allocate pinned host memory"); }
    cap = want;
    return MC_OK;
}

inline size_t up128(size_t x) { return (x + 127) / 128 * 128; }
// a long-tier problem's scratch: the boundary row (one number per row of the longer of read and mate, + 1), then read 1's predecessor bits
inline size_t long_scratch(uint64_t lq, uint64_t lm, uint64_t ls) { return up128((std::max(lq, lm) + 1) * 4) + (ls + kLanes * kLongW - 1) / (kLanes * kLongW) * lq * kLanes * 2 + 128; }

// the problems [a, b) on the device; results and strings into the caller's arrays (aligned_off[a] is set, [a+1 .. b] are filled)
int run_sub_batch(mc_ctx* ctx, AlignWork& w, const char* reads, const uint64_t* roff, const char* mates, const uint64_t* moff, const char* subjects,
                  const uint64_t* soff, uint64_t a, uint64_t b, int32_t* sf, int32_t* sr, int32_t* mf, int32_t* mr, uint8_t* reversed, char* aligned,
                  uint64_t* alignedOff)
{
    const size_t n = (size_t)(b - a);
    size_t nchars = 0, outBytes = 0, scratchBytes = 0, nshort = 0, ldsBytes = 0;
    for (uint64_t i = a; i < b; ++i) {
        const uint64_t lq = roff[i + 1] - roff[i], lm = mates ? moff[i + 1] - moff[i] : 0, ls = soff[i + 1] - soff[i];
        nchars += lq + lm + ls;
        outBytes += 2 * std::max<uint64_t>(1, lq + ls);
        if (lq <= kShortMaxQ && ls <= kShortMaxS) { ++nshort; ldsBytes = std::max<size_t>(ldsBytes, (size_t)lq * kLanes * (ls <= 4 * kLanes ? 1 : 2)); }
        else scratchBytes += long_scratch(lq, lm, ls);
    }
    const size_t probsAt = up128(nchars + 16), listAt = probsAt + up128(n * sizeof(AlignProblem)), inBytes = listAt + up128(n * 4);
    const size_t resBytes = up128(n * sizeof(AlignResult));
    if (int rc = grow_host(ctx, w.hIn, w.hInCap, inBytes)) return rc;
    if (int rc = grow_host(ctx, w.hOut, w.hOutCap, resBytes + outBytes)) return rc;
    if (int rc = grow_with_headroom(ctx, w.dChars, inBytes)) return rc;
    if (int rc = grow_with_headroom(ctx, w.dRes, resBytes + outBytes)) return rc;
    if (int rc = grow_with_headroom(ctx, w.dScratch, scratchBytes + 128)) return rc;
    uint8_t* hc = static_cast<uint8_t*>(w.hIn);
    AlignProblem* hp = reinterpret_cast<AlignProblem*>(hc + probsAt);
    uint32_t* hl = reinterpret_cast<uint32_t*>(hc + listAt);       // the short tier's problems from the front, the long tier's from the back
    size_t at = 0, oat = 0, sat = 0, ns = 0, nl = 0;
    for (uint64_t i = a; i < b; ++i) {
        AlignProblem& P = hp[i - a];
        const uint64_t lq = roff[i + 1] - roff[i], lm = mates ? moff[i + 1] - moff[i] : 0, ls = soff[i + 1] - soff[i];
        P.q = at; std::memcpy(hc + at, reads + roff[i], lq); at += lq;
        P.m = at; if (lm) std::memcpy(hc + at, mates + moff[i], lm); at += lm;
        P.s = at; std::memcpy(hc + at, subjects + soff[i], ls); at += ls;
        P.lenQ = (uint32_t)lq; P.lenM = (uint32_t)lm; P.lenS = (uint32_t)ls; P.hasMate = mates ? 1u : 0u;
        P.out = oat; oat += 2 * std::max<uint64_t>(1, lq + ls);
        P.scratch = 0;
        if (lq <= kShortMaxQ && ls <= kShortMaxS) hl[ns++] = (uint32_t)(i - a);
        else {
            P.scratch = sat;
            sat += long_scratch(lq, lm, ls);
            hl[n - 1 - nl++] = (uint32_t)(i - a);
        }
    }
    uint8_t* dc = static_cast<uint8_t*>(w.dChars.p);
    uint8_t* dr = static_cast<uint8_t*>(w.dRes.p);
    HIP_TRY(ctx, hipMemcpyAsync(dc, hc, inBytes, hipMemcpyHostToDevice, w.stream));
    HIP_TRY(ctx, hipEventRecord(w.e0, w.stream));
    const AlignProblem* dp = reinterpret_cast<const AlignProblem*>(dc + probsAt);
    const uint32_t* dl = reinterpret_cast<const uint32_t*>(dc + listAt);
    if (ns) hipLaunchKernelGGL(align_kernel<false>, dim3((uint32_t)ns), dim3(64), ldsBytes, w.stream, dp, dl, (uint32_t)ns, dc, dr + resBytes,
                               reinterpret_cast<AlignResult*>(dr), (uint8_t*)nullptr);
    if (nl) hipLaunchKernelGGL(align_kernel<true>, dim3((uint32_t)nl), dim3(64), 0, w.stream, dp, dl + (n - nl), (uint32_t)nl, dc, dr + resBytes,
                               reinterpret_cast<AlignResult*>(dr), static_cast<uint8_t*>(w.dScratch.p));
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(w.e1, w.stream));
    HIP_TRY(ctx, hipMemcpyAsync(w.hOut, dr, resBytes + outBytes, hipMemcpyDeviceToHost, w.stream));
    HIP_TRY(ctx, hipStreamSynchronize(w.stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, w.e0, w.e1) == hipSuccess) ctx->alignKernelNs += (uint64_t)((double)ms * 1e6);
    const AlignResult* hr = static_cast<const AlignResult*>(w.hOut);
    const char* ho = static_cast<const char*>(w.hOut) + resBytes;
    uint64_t to = alignedOff[a];
    for (uint64_t i = a; i < b; ++i) {
        const AlignResult& R = hr[i - a];
        const AlignProblem& P = hp[i - a];
        const uint64_t cap = std::max<uint64_t>(1, (uint64_t)P.lenQ + P.lenS);
        if (R.length < 1 || R.length > cap) return fail(ctx, MC_ERR_HIP, "mc_align_semiglobal: a trace left its bounds");
        sf[i] = R.fwd; sr[i] = R.rev; mf[i] = R.mfwd; mr[i] = R.mrev; reversed[i] = (uint8_t)R.reversed;
        std::memcpy(aligned + to, ho + P.out + cap - R.length, R.length);
        std::memcpy(aligned + to + R.length, ho + P.out + 2 * cap - R.length, R.length);
        to += 2ull * R.length;
        alignedOff[i + 1] = to;
    }
    ++ctx->alignSubBatches;
    return MC_OK;
}

}  // namespace

namespace mcamd {
void free_align_works(mc_ctx* ctx)
{
    for (AlignWork* w : ctx->alignWorks) {
        if (w->stream) { (void)hipStreamSynchronize(w->stream); (void)hipStreamDestroy(w->stream); }
        if (w->e0) (void)hipEventDestroy(w->e0);
        if (w->e1) (void)hipEventDestroy(w->e1);
        for (DevBuf* b : {&w->dChars, &w->dRes, &w->dScratch}) if (b->p) (void)hipFree(b->p);
        if (w->hIn) (void)hipHostFree(w->hIn);
        if (w->hOut) (void)hipHostFree(w->hOut);
        delete w;
    }
    ctx->alignWorks.clear();
}
}  // namespace mcamd

extern "C" int mc_align_semiglobal(mc_ctx* ctx, const char* reads, const uint64_t* read_off, const char* mates, const uint64_t* mate_off,
                                   const char* subjects, const uint64_t* subj_off, uint64_t n, int32_t* score_fwd, int32_t* score_rev,
                                   int32_t* mate_fwd, int32_t* mate_rev, uint8_t* reversed, char* aligned, uint64_t aligned_cap, uint64_t* aligned_off)
{
    if (!ctx) return MC_ERR_INVALID;
    if (!aligned_off) return fail(ctx, MC_ERR_INVALID, "mc_align_semiglobal: null argument");
    aligned_off[0] = 0;
    if (n == 0) return MC_OK;
    if (!reads || !read_off || !subjects || !subj_off || !score_fwd || !score_rev || !mate_fwd || !mate_rev || !reversed || !aligned || (mates && !mate_off))
        return fail(ctx, MC_ERR_INVALID, "mc_align_semiglobal: null argument");
    uint64_t need = 0;
    for (uint64_t i = 0; i < n; ++i) {
        if (read_off[i + 1] < read_off[i] || subj_off[i + 1] < subj_off[i] || (mates && mate_off[i + 1] < mate_off[i]))
            return fail(ctx, MC_ERR_INVALID, "mc_align_semiglobal: offsets must not decrease");
        const uint64_t lq = read_off[i + 1] - read_off[i], ls = subj_off[i + 1] - subj_off[i], lm = mates ? mate_off[i + 1] - mate_off[i] : 0;
        if (lq >= (1ull << 28) || ls >= (1ull << 28) || lm >= (1ull << 28)) return fail(ctx, MC_ERR_UNSUPPORTED, "mc_align_semiglobal: sequence of 2^28 characters or more");
        need += 2 * std::max<uint64_t>(1, lq + ls);
    }
    if (aligned_cap < need) return fail(ctx, MC_ERR_INVALID, "mc_align_semiglobal: the buffer for the aligned strings must hold 2 x max(1, len_q + len_s) characters per problem");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { (void)hipGetLastError(); return fail(ctx, MC_ERR_HIP, "no usable HIP device (this library has no CPU fallback)"); }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    AlignWork* w = nullptr;
    { std::lock_guard<std::mutex> l(ctx->alignMtx); if (!ctx->alignWorks.empty()) { w = ctx->alignWorks.back(); ctx->alignWorks.pop_back(); } }
    if (!w) w = new AlignWork();
    struct Return { mc_ctx* c; AlignWork* w; ~Return() { std::lock_guard<std::mutex> l(c->alignMtx); c->alignWorks.push_back(w); } } giveBack{ctx, w};
    if (!w->stream) HIP_TRY(ctx, hipStreamCreateWithFlags(&w->stream, hipStreamNonBlocking));
    if (!w->e0) HIP_TRY(ctx, hipEventCreate(&w->e0));
    if (!w->e1) HIP_TRY(ctx, hipEventCreate(&w->e1));
    // sub-batches: device output + the long tier's scratch + characters of one stay under the budget; one problem alone always goes
    const uint64_t budget = (uint64_t)std::max<int64_t>(1, ctx->alignScratchMb) << 20;
    for (uint64_t a = 0; a < n;) {
        uint64_t b = a, cost = 0;
        while (b < n && b - a < (1u << 22)) {
            const uint64_t lq = read_off[b + 1] - read_off[b], ls = subj_off[b + 1] - subj_off[b], lm = mates ? mate_off[b + 1] - mate_off[b] : 0;
            uint64_t c = 2 * std::max<uint64_t>(1, lq + ls) + lq + ls + lm + sizeof(AlignProblem) + sizeof(AlignResult) + 4;
            if (!(lq <= kShortMaxQ && ls <= kShortMaxS)) c += long_scratch(lq, lm, ls);
            if (b > a && cost + c > budget) break;
            cost += c; ++b;
        }
        if (int rc = run_sub_batch(ctx, *w, reads, read_off, mates, mate_off, subjects, subj_off, a, b, score_fwd, score_rev, mate_fwd, mate_rev, reversed, aligned, aligned_off)) return rc;
        for (uint64_t i = a; i < b; ++i) {
            const uint64_t lq = read_off[i + 1] - read_off[i], ls = subj_off[i + 1] - subj_off[i];
            ctx->alignCells += lq * ls;
        }
        ctx->alignProblems += b - a;
        a = b;
    }
    return MC_OK;
}

extern "C" int mc_align_stats(const mc_ctx* ctx, uint64_t stats[4])
{
    if (!ctx || !stats) return MC_ERR_INVALID;
    stats[0] = ctx->alignProblems; stats[1] = ctx->alignCells; stats[2] = ctx->alignKernelNs; stats[3] = ctx->alignSubBatches;
    return MC_OK;
}
