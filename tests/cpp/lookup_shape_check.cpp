// tests/cpp/lookup_shape_check.cpp -- host check of lookup_shape (csrc/query_rules.h): which instance of gw_filter_count_kernel<LOOKUP> a batch
// gets.  The model is the list of shipped instances itself: (window range, candidates) in {2, 3} x {1, 2}, for batches WITHOUT a window
// range per read; every other batch keeps the instance for any shape {0, 0}.  Stand-alone: a plain host compiler builds it.
#include "query_rules.h"

#include <cstdio>
#include <cstring>

using namespace mcamd;

int main()
{
    static_assert(lookup_shape(false, 3, 2) == LookupShape{3, 2}, "the flagship batch: 150 bp single reads, two candidates");
    static_assert(lookup_shape(true, 3, 2) == LookupShape{0, 0}, "a range per read: never fixed");
    const uint32_t shipped[4][2] = {{3, 2}, {2, 2}, {3, 1}, {2, 1}};
    uint64_t cases = 0, fixed = 0, bad = 0;
    for (int perRead = 0; perRead < 2; ++perRead)
        for (uint32_t win = 0; win <= 70; ++win)
            for (uint32_t k = 0; k <= 9; ++k) {
                const uint32_t wins[2] = {win, win > 64 ? 0xFFFFFFFFu - (70 - win) : win};   // (and the largest values)
                for (uint32_t w : wins) {
                    bool want = false;
                    for (const auto& s : shipped) want = want || (!perRead && w == s[0] && k == s[1]);
                    const LookupShape got = lookup_shape(perRead != 0, w, k);
                    const bool ok = want ? (got.maxWin == w && got.k == k) : (got.maxWin == 0 && got.k == 0);
                    // the name the launch counters use: one per shipped instance, one for the rest
                    char name[64];
                    if (want) std::snprintf(name, sizeof name, "gw_filter_lookup_w%u_k%u", w, k);
                    else std::snprintf(name, sizeof name, "gw_filter_lookup_any");
                    const bool nameOk = std::strcmp(name, lookup_shape_name(got)) == 0;
                    if (!ok || !nameOk) { ++bad; std::printf("MISMATCH perRead %d windows %u maxcand %u -> {%u, %u} %s\n", perRead, w, k, got.maxWin, got.k, lookup_shape_name(got)); }
                    ++cases; fixed += want;
                }
            }
    std::printf("lookup shape %s: %llu cases, %llu fixed\n", bad ? "FAILED" : "ok", (unsigned long long)cases, (unsigned long long)fixed);
    return bad ? 1 : 0;
}
