// metacache_amd/csrc/input_device.hip -- mc_input_*: a query file RESIDENT on the device, for callers above the C ABI that own no device
// memory themselves (`mcq query`, MCQ_INPUT_DEVICE).  mc_input_open takes a file's bytes as they lie on the host -- plain
// text, or BGZF, which goes through mc_bgzf_index and the DEVICE form of mc_inflate_blocks so that the plain bytes never exist on the
// host --, cuts the resident bytes piece by piece with mc_parse_cut (every piece but the last with MC_CUT_OPEN, the next one starting at
// `consumed`) and keeps the batches as {offset, bytes, records}; a batch that exceeds what a slot takes is cut again with half the
// records, down to one query.  The batches then go to the slots through mc_batch_add_device_bytes.  No kernels of its own.
#include "rows_common.h"

#include <algorithm>
#include <memory>
#include <vector>

using namespace mcamd;

struct mc_input {
    mc_ctx* ctx = nullptr;
    uint8_t* dBytes = nullptr;               // the file's plain bytes
    uint64_t nbytes = 0;
    std::vector<mc_input_batch> batches;
};

namespace {

struct DeviceBlock {                         // freed with the scope
    void* p = nullptr;
    ~DeviceBlock() { if (p) (void)hipFree(p); }
    bool alloc(uint64_t bytes) { return hipMalloc(&p, bytes) == hipSuccess; }
};

struct Cutter {
    mc_ctx* ctx; mc_input* in; hipStream_t st;
    uint32_t per; int pairFlag; uint64_t slotBytes;
    DeviceBlock ws, cuts, status;
    uint64_t cutsCap = 0, wsBytes = 0;
    uint64_t* hStatus = nullptr;             // pinned [8]
    std::vector<uint64_t> hCuts;
    ~Cutter() { if (hStatus) (void)hipHostFree(hStatus); }

    // one mc_parse_cut of in->dBytes[at, at + n) on the device, then its status (and, with MC_PARSE_OK, its cuts) on the host
    int cut(uint64_t at, uint64_t n, uint32_t R, bool open)
    {
        const uint64_t need = mc_parse_cut_scratch_bytes(n);
        if (need > wsBytes) { if (ws.p) { (void)hipFree(ws.p); ws.p = nullptr; } if (!ws.alloc(need)) return fail(ctx, MC_ERR_HIP, "mc_input_open: no memory for the cut's workspace"); wsBytes = need; }
        for (int pass = 0; pass < 2; ++pass) {
            const int flags = pairFlag | (open ? MC_CUT_OPEN : 0);
            if (const int rc = mc_parse_cut(ctx, (const char*)in->dBytes + at, n, R, flags, (uint64_t*)cuts.p, cutsCap, (uint64_t*)status.p, ws.p, wsBytes, st)) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(hStatus, status.p, 64, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (hStatus[4] != MC_PARSE_OVERFLOW) break;
            if (cuts.p) { (void)hipFree(cuts.p); cuts.p = nullptr; }
            cutsCap = hStatus[1] + 1;
            if (!cuts.alloc(cutsCap * 8)) return fail(ctx, MC_ERR_HIP, "mc_input_open: no memory for the cuts");
        }
        if (hStatus[4] == MC_PARSE_OK) {
            hCuts.resize(hStatus[1] + 1);
            HIP_TRY(ctx, hipMemcpy(hCuts.data(), cuts.p, hCuts.size() * 8, hipMemcpyDeviceToHost));
        }
        return MC_OK;
    }

    // the batches of a cut that lies in hCuts / hStatus (records per batch R), at `at`; one that exceeds a slot is cut again
    int take(uint64_t at, uint32_t R, bool closedHalf, uint64_t& irregularAt, bool& irregular)
    {
        const std::vector<uint64_t> c = hCuts;
        const uint64_t whole = hStatus[0];
        for (size_t i = 0; i + 1 < c.size(); ++i) {
            const uint32_t recs = (uint32_t)std::min<uint64_t>(R, whole - (uint64_t)i * R);
            const bool half = closedHalf && i + 2 == c.size() && (recs & 1u);
            const uint64_t b = at + c[i], n = c[i + 1] - c[i];
            if (n <= slotBytes || R <= per) {
                in->batches.push_back(mc_input_batch{b, n, recs, (recs + per - 1) / per, half ? 1u : 0u, n > slotBytes ? 1u : 0u});
                continue;
            }
            uint32_t finer = std::max(per, R / 2);
            if (per == 2) finer &= ~1u;
            if (const int rc = cut(b, n, finer, false)) return rc;
            if (hStatus[4] != MC_PARSE_OK) { irregular = true; irregularAt = b + hStatus[5]; return MC_OK; }   // (cannot happen: the range was accepted as part of a larger one)
            if (const int rc = take(b, finer, half, irregularAt, irregular)) return rc;
            if (irregular) return MC_OK;
        }
        return MC_OK;
    }
};

void set_info(uint64_t info[8], uint64_t verdict, uint64_t detail, uint64_t detail2 = 0) { info[0] = verdict; info[1] = detail; info[7] = detail2; }

}  // namespace

extern "C" {

int mc_input_open(mc_ctx* ctx, const void* file_bytes, uint64_t nbytes, int flags, uint32_t records_per_batch, uint64_t piece_bytes, uint64_t slot_bytes,
                  uint64_t max_resident_bytes, mc_input** out, uint64_t info[8])
{
    if (!ctx) return MC_ERR_INVALID;
    if (!out || !info) return fail(ctx, MC_ERR_INVALID, "mc_input_open: no place for the handle or the info");
    *out = nullptr;
    for (int k = 0; k < 8; ++k) info[k] = 0;
    if (!file_bytes || nbytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_input_open: no bytes");
    if (flags & ~MC_PARSE_PAIRS) return fail(ctx, MC_ERR_INVALID, "mc_input_open: unknown flag");
    if (records_per_batch == 0 || ((flags & MC_PARSE_PAIRS) && (records_per_batch & 1u))) return fail(ctx, MC_ERR_INVALID, "mc_input_open: no records per batch, or an odd number with MC_PARSE_PAIRS");
    if (piece_bytes == 0 || piece_bytes > (1ull << 31) || slot_bytes == 0) return fail(ctx, MC_ERR_INVALID, "mc_input_open: a piece of 0 or more than 2^31 bytes, or a slot of 0 bytes");
    if (!ctx->stream) return fail(ctx, MC_ERR_STATE, "mc_input_open: the context has no device (mc_open_metadata)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    const uint8_t* B = (const uint8_t*)file_bytes;
    std::unique_ptr<mc_input> in(new mc_input);
    in->ctx = ctx;
    struct Drop { mc_input* h; ~Drop() { if (h && h->dBytes) (void)hipFree(h->dBytes); } } drop{in.get()};   // (released below where the handle is kept)
    const bool gz = nbytes >= 2 && B[0] == 0x1f && B[1] == 0x8b;
    if (gz) {
        uint64_t bi[4] = {0, 0, 0, 0};
        if (const int rc = mc_bgzf_index(B, nbytes, nullptr, 0, bi)) return rc;
        if (bi[2] != MC_BGZF_OK) { set_info(info, MC_INPUT_NOT_BGZF, bi[3]); drop.h = in.get(); return MC_OK; }
        std::vector<mc_bgzf_block> rows(bi[0]);
        if (const int rc = mc_bgzf_index(B, nbytes, rows.data(), rows.size(), bi)) return rc;
        in->nbytes = bi[1];
        info[2] = in->nbytes;
        if (in->nbytes == 0) { set_info(info, MC_INPUT_EMPTY, 0); return MC_OK; }
        if (in->nbytes > max_resident_bytes) { set_info(info, MC_INPUT_TOO_LARGE, in->nbytes); return MC_OK; }
        DeviceBlock dIn, dRows, dStatus;
        if (hipMalloc((void**)&in->dBytes, in->nbytes + 32) != hipSuccess || !dIn.alloc((nbytes + 15) / 16 * 16 + 16) || !dRows.alloc(rows.size() * sizeof(mc_bgzf_block)) || !dStatus.alloc(32)) {
            (void)hipGetLastError();
            set_info(info, MC_INPUT_NO_MEMORY, in->nbytes);
            return MC_OK;
        }
        HIP_TRY(ctx, hipMemcpyAsync(dIn.p, B, nbytes, hipMemcpyHostToDevice, st));
        HIP_TRY(ctx, hipMemcpyAsync(dRows.p, rows.data(), rows.size() * sizeof(mc_bgzf_block), hipMemcpyHostToDevice, st));
        // the rows in groups of at most 2^20 members: a group's status is read before the next one is enqueued
        uint64_t hst[4] = {0, 0, 0, 0};
        constexpr size_t kGroup = (size_t)1 << 20;
        for (size_t r0 = 0; r0 < rows.size(); r0 += kGroup) {
            const size_t m = std::min(kGroup, rows.size() - r0);
            if (const int rc = mc_inflate_blocks(ctx, (const uint8_t*)dIn.p, nbytes, (const mc_bgzf_block*)dRows.p + r0, m, 0, in->dBytes, in->nbytes, (uint64_t*)dStatus.p, st)) return rc;
            HIP_TRY(ctx, hipMemcpyAsync(hst, dStatus.p, 32, hipMemcpyDeviceToHost, st));
            HIP_TRY(ctx, hipStreamSynchronize(st));
            if (hst[0] != MC_INFLATE_OK) { set_info(info, MC_INPUT_REFUSED, r0 + hst[1], hst[2]); info[6] = hst[0]; return MC_OK; }
        }
        info[6] = 1;
    } else {
        in->nbytes = nbytes;
        info[2] = nbytes;
        if (nbytes > max_resident_bytes) { set_info(info, MC_INPUT_TOO_LARGE, nbytes); return MC_OK; }
        if (hipMalloc((void**)&in->dBytes, nbytes + 32) != hipSuccess) { (void)hipGetLastError(); set_info(info, MC_INPUT_NO_MEMORY, nbytes); return MC_OK; }
        HIP_TRY(ctx, hipMemcpyAsync(in->dBytes, B, nbytes, hipMemcpyHostToDevice, st));
    }
    // the pieces
    Cutter C{ctx, in.get(), st, (flags & MC_PARSE_PAIRS) ? 2u : 1u, flags & MC_PARSE_PAIRS, slot_bytes};
    C.cutsCap = 1024;
    if (!C.cuts.alloc(C.cutsCap * 8) || !C.status.alloc(64) || hipHostMalloc((void**)&C.hStatus, 64) != hipSuccess) { (void)hipGetLastError(); set_info(info, MC_INPUT_NO_MEMORY, in->nbytes); return MC_OK; }
    uint64_t pos = 0, pieces = 0, records = 0;
    // (a refused file that was inflated keeps its handle: the caller copies the bytes back once and reads them the old way)
    auto refused = [&](uint64_t verdict, uint64_t detail) { set_info(info, verdict, detail); in->batches.clear(); if (gz) { *out = in.release(); drop.h = nullptr; } return MC_OK; };
    while (pos < in->nbytes) {
        uint64_t size = piece_bytes;
        for (;;) {
            const uint64_t n = std::min(size, in->nbytes - pos);
            const bool last = pos + n == in->nbytes;
            if (const int rc = C.cut(pos, n, records_per_batch, !last)) return rc;
            if (C.hStatus[4] != MC_PARSE_OK) return refused(MC_INPUT_IRREGULAR, pos + C.hStatus[5]);
            if (last || C.hStatus[2] > 0) break;
            if (size >= (1ull << 31)) return refused(MC_INPUT_RECORD_TOO_LARGE, pos);   // a record that does not fit the largest piece
            size = std::min<uint64_t>(size * 2, 1ull << 31);
        }
        const uint64_t consumed = C.hStatus[2], whole = C.hStatus[0];
        const bool half = C.hStatus[7] != 0;
        uint64_t at = 0; bool irregular = false;
        if (const int rc = C.take(pos, records_per_batch, half, at, irregular)) return rc;
        if (irregular) return refused(MC_INPUT_IRREGULAR, at);
        records += whole; ++pieces;
        pos += consumed;
    }
    info[3] = pieces; info[4] = in->batches.size(); info[5] = records;
    set_info(info, MC_INPUT_OK, 0);
    *out = in.release(); drop.h = nullptr;
    return MC_OK;
}

int mc_input_batches(const mc_input* in, mc_input_batch* batches, uint64_t capacity, const void** device_bytes, uint64_t* nbytes)
{
    if (!in) return MC_ERR_INVALID;
    if (device_bytes) *device_bytes = in->dBytes;
    if (nbytes) *nbytes = in->nbytes;
    if (batches) std::copy_n(in->batches.begin(), std::min<uint64_t>(capacity, in->batches.size()), batches);
    return MC_OK;
}

int mc_input_download(const mc_input* in, void* host_bytes, uint64_t capacity)
{
    if (!in || !host_bytes) return MC_ERR_INVALID;
    if (capacity < in->nbytes) return fail(in->ctx, MC_ERR_INVALID, "mc_input_download: the buffer is smaller than the file");
    HIP_TRY(in->ctx, hipSetDevice(in->ctx->device));
    HIP_TRY(in->ctx, hipMemcpy(host_bytes, in->dBytes, in->nbytes, hipMemcpyDeviceToHost));
    return MC_OK;
}

void mc_input_close(mc_input* in)
{
    if (!in) return;
    if (in->dBytes) { (void)hipSetDevice(in->ctx->device); (void)hipFree(in->dBytes); }
    delete in;
}

}  // extern "C"
