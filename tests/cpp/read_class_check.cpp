// tests/cpp/read_class_check.cpp -- host check of csrc/read_class.h: the rule that sorts a read into its class against a decision table
// written here on its own (plain numbers, the order of the work-list table in csrc/kernels.h, no call into the header), the limits
// every class promises its consumer, the work-list record's fields, and the classes' counter slots and lists.
// Built and run by tests/test_read_class_cpu.py under the address and undefined-behaviour sanitizers.
#include "read_class.h"

#include <cstdio>
#include <set>
#include <vector>

using namespace mcamd;

namespace {

int g_bad = 0;
void mismatch(const char* what, uint32_t H, uint32_t ent, uint32_t mw, uint32_t bigMin, bool compact, long got, long want)
{
    if (++g_bad <= 20) std::printf("MISMATCH %s: H %u entries %u maxWin %u bigMin %u %s: %ld, expected %ld\n", what, H, ent, mw, bigMin,
                                   compact ? "compact" : "8-byte", got, want);
}

constexpr uint32_t kGap = 1024;   // DeviceTable::gwGap as the loader sets it

// ---- the decision table: class numbers and limits as the table in kernels.h and the kernels' heads give them ----
uint32_t model_class(uint32_t H, uint32_t ent, uint32_t mw, uint32_t bigMin, uint32_t gap, bool compact)
{
    // 7, the filtered path: more than bigMin locations, and more than the 64 that are sorted in registers ...
    if (H > bigMin && H > 64) {
        if (compact) {                                   // ... compact store: what the record can name, inside the gap between two targets
            if (ent <= 4095 && mw <= gap && H <= 1048575) return 7;
        } else {                                         // ... 8-byte store: up to 3 entries for each of 64 lanes, the counting kernel's window range
            if (ent <= 192 && mw <= 8) return 7;
        }
    }
    const bool counted = ent <= 256 && mw <= 8;          // hash_cands_kernel can take the read
    if (H <= 64) return 0;                               // kListMid64
    if (H <= 128) return counted ? 5 : 1;                // kListHash256, else kListMid128
    if (H <= 256) return counted ? 5 : 2;                // kListHash256, else kListMid256
    if (H <= 512 && counted) return 3;                   // kListHash512
    if (H <= 1024 && counted) return 4;                  // kListHash1024
    return 6;                                            // the wave kernels
}
bool model_second(uint32_t H, uint32_t ent, bool compact)
{
    if (compact) return H > 2048;
    return ent > 64;
}
uint32_t model_segment(uint32_t H, uint32_t cls)
{
    uint32_t seg = 0;
    if (H <= 1048575 && H > 256) seg = H;                // beyond what is sorted in LDS, and a list at all
    if (cls == 3 || cls == 4 || cls == 5 || cls == 7) seg = 0;   // the counting kernels and the filtered path read the table's lists
    return seg;
}

std::vector<uint32_t> hit_counts(uint32_t bigMin)
{
    std::set<uint32_t> hs;
    for (const uint32_t border : {0u, 64u, 128u, 256u, 512u, 1024u, kGwSmallH, bigMin, kMaxHitsPerQuery}) {
        hs.insert(border);
        if (border > 0) hs.insert(border - 1);
        if (border < 0xFFFFFFFFu) hs.insert(border + 1);
    }
    return std::vector<uint32_t>(hs.begin(), hs.end());
}

}  // namespace

int main()
{
    const uint32_t bigMins[] = {0u, 64u, 200u, 5000u, 0xFFFFFFFFu};
    const uint32_t maxWins[] = {1u, kHashWin, kHashWin + 1, kGap, kGap + 1};
    const uint32_t entries[] = {1u, 64u, 65u, 192u, 193u, 256u, 257u, 0xFFFu, 0x1000u};
    unsigned long rule = 0, limits = 0;
    for (const bool compact : {false, true})
        for (const uint32_t bigMin : bigMins)
            for (const uint32_t mw : maxWins)
                for (const uint32_t ent : entries)
                    for (const uint32_t H : hit_counts(bigMin)) {
                        const ClassLimits lim{bigMin, kGap, compact};
                        const uint32_t cls = read_class(H, ent, mw, lim), want = model_class(H, ent, mw, bigMin, kGap, compact);
                        // a. the rule
                        if (cls != want) mismatch("read_class", H, ent, mw, bigMin, compact, cls, want);
                        if (filter_takes(H, ent, mw, lim) != (want == 7)) mismatch("filter_takes", H, ent, mw, bigMin, compact, filter_takes(H, ent, mw, lim), want == 7);
                        if (filter_second(H, ent, compact) != model_second(H, ent, compact))
                            mismatch("filter_second", H, ent, mw, bigMin, compact, filter_second(H, ent, compact), model_second(H, ent, compact));
                        if (segment_hits(H, cls) != model_segment(H, want)) mismatch("segment_hits", H, ent, mw, bigMin, compact, segment_hits(H, cls), model_segment(H, want));
                        ++rule;
                        // b. what the class promises its consumer
                        bool ok = true;
                        switch (cls) {
                        case kListMid64: ok = H <= 64; break;
                        case kListMid128: ok = H <= 128; break;
                        case kListMid256: ok = H <= 256 && H <= kMidMax; break;
                        case kListHash256: ok = ent <= kHashEnt && mw <= kHashWin && H > 64 && H <= 256; break;
                        case kListHash512: ok = ent <= kHashEnt && mw <= kHashWin && H > 256 && H <= 512; break;
                        case kListHash1024: ok = ent <= kHashEnt && mw <= kHashWin && H > 512 && H <= kHashMax; break;
                        case kClassFilter:
                            ok = compact ? (ent <= kRecEntMax && rec_entries(work_record(0, 0, ent, H, mw).packed) == ent &&
                                            rec_hits(work_record(0, 0, ent, H, mw).packed) == H && H <= kMaxHitsPerQuery)
                                         : (ent <= kBigEnt * kBigEPL && mw <= kHashWin);
                            break;
                        case kClassWave: break;
                        default: ok = false;
                        }
                        if (!ok) mismatch("consumer limits", H, ent, mw, bigMin, compact, cls, -1);
                        ++limits;
                    }
    std::printf("rule ok: %lu cases\nlimits ok: %lu cases\n", rule, limits);

    // c. the record's fields, up to the largest legal values
    unsigned long recs = 0;
    for (const uint32_t ent : {0u, 1u, 64u, kRecEntMax - 1, kRecEntMax})
        for (const uint32_t H : {0u, 1u, 65u, kGwSmallH, kMaxHitsPerQuery - 1, kMaxHitsPerQuery}) {
            const WorkRecord r = work_record(0xFFFFFFFFu, 0xFFFFFFFEu, ent, H, 0xFFFFFFFDu);
            if (r.query != 0xFFFFFFFFu || r.first != 0xFFFFFFFEu || r.maxWin != 0xFFFFFFFDu || rec_entries(r.packed) != ent || rec_hits(r.packed) != H)
                mismatch("work_record", H, ent, r.maxWin, 0, true, r.packed, -1);
            ++recs;
        }
    std::printf("record ok: %lu cases\n", recs);

    // d. the classes' counter slots and lists, as the table in kernels.h names them: {class, slot of ws.midCount, list of ws.midList}
    const uint32_t slots[][3] = {{0, 0, 0}, {1, 1, 1}, {2, 2, 2}, {3, 3, 3}, {4, 4, 4}, {5, 8, 5}, {7, 9, 6}};
    unsigned long maps = 0;
    for (const auto& s : slots) {
        if (class_counter(s[0]) != s[1] || class_list(s[0]) != s[2]) mismatch("class_counter / class_list", 0, 0, 0, 0, true, class_counter(s[0]), s[1]);
        ++maps;
    }
    static_assert(kListMid64 == 0 && kListMid128 == 1 && kListMid256 == 2 && kListHash512 == 3 && kListHash1024 == 4 && kListHash256 == 5 &&
                  kListFilter == 6 && kListFiltered == 7 && kWorkLists == 8 && kClassWave == 6 && kClassFilter == 7, "classes 0 .. 5 are the lists of the same number");
    static_assert(kCntMid64 == 0 && kCntMid128 == 1 && kCntMid256 == 2 && kCntHash512 == 3 && kCntHash1024 == 4 && kCntHash256 == 8 &&
                  kCntFilter == 9 && kCntSecond == 10, "the slots of the table in kernels.h");
    std::printf("slots ok: %lu cases\n", maps);
    return g_bad ? 1 : 0;
}
