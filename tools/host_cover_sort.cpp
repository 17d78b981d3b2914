// tools/host_cover_sort.cpp -> libmccoversort.so: what `mcq query -hits-per-ref` did with its per-target records before the library
// sorted them (mcq_main.cpp, show_hits_per_ref): one std::sort of 32-byte Cover records on one thread, by target, window range and
// query id.  Measurement tool (tools/target_hits_bench.py); nothing of it is in the product.
#include "metacache_amd.h"

#include <algorithm>
#include <chrono>
#include <vector>

struct Cover { uint32_t tgt; uint64_t qid; uint32_t beg, end, hits; };
static_assert(sizeof(Cover) == 32, "the record mcq kept per qualifying candidate");

// the records as Covers (not timed), then the sort (timed): milliseconds; *sorted_ok = the result is in order
extern "C" double mc_tool_cover_sort_ms(const mc_target_hit* rec, uint64_t n, int* sorted_ok)
{
    std::vector<Cover> covers(n);
    for (uint64_t i = 0; i < n; ++i) covers[i] = Cover{rec[i].tgt, rec[i].query, rec[i].beg, rec[i].end, rec[i].hits};
    auto less = [](const Cover& a, const Cover& b) {
        if (a.tgt != b.tgt) return a.tgt < b.tgt;
        if (a.beg != b.beg) return a.beg < b.beg;
        if (a.end != b.end) return a.end < b.end;
        return a.qid < b.qid;
    };
    const auto t0 = std::chrono::steady_clock::now();
    std::sort(covers.begin(), covers.end(), less);
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (sorted_ok) *sorted_ok = std::is_sorted(covers.begin(), covers.end(), less) ? 1 : 0;
    return ms;
}

// 1 if rec[0 .. n) ascends by (tgt, beg, end, query, hits): the order mc_target_hits_collect promises
extern "C" int mc_tool_records_in_order(const mc_target_hit* rec, uint64_t n)
{
    for (uint64_t i = 1; i < n; ++i) {
        const mc_target_hit &a = rec[i - 1], &b = rec[i];
        if (a.tgt != b.tgt) { if (a.tgt > b.tgt) return 0; continue; }
        if (a.beg != b.beg) { if (a.beg > b.beg) return 0; continue; }
        if (a.end != b.end) { if (a.end > b.end) return 0; continue; }
        if (a.query != b.query) { if (a.query > b.query) return 0; continue; }
        if (a.hits > b.hits) return 0;
    }
    return 1;
}
