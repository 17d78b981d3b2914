// tests/cpp/table_rules_check.cpp -- host check of csrc/table_rules.h: the load-time size rule and the host load steps (the multi-part
// merge, Mode T's cut) against a naive model written here: a std::map from key to the concatenated location list, the rules applied
// per part in the reference's order (host_hashmap.hpp:454-495: remove-overpopulated empties a bucket, max-locations keeps the first n).
// Stand-alone: tests/test_table_rules_cpu.py builds it with -fsanitize=address,undefined and runs it.
#include "table_rules.h"

#include <algorithm>
#include <cstdio>
#include <map>

using namespace mcamd;

static int g_bad = 0;
#define CHECK(cond, ...) do { if (!(cond)) { if (++g_bad <= 20) { std::printf("MISMATCH %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

// ---- the model ------------------------------------------------------------------------------------------------------------------------
static uint32_t model_size(uint32_t fileSize, uint32_t rmOver, uint32_t maxLocs)
{
    if (rmOver != 0 && fileSize > rmOver) return 0;
    return maxLocs != 0 && fileSize > maxLocs ? maxLocs : fileSize;
}
static uint32_t model_alloc(uint32_t size, uint32_t align)
{
    if (size <= 1) return 0;                                   // nothing, or the bucket's inline payload
    uint32_t a = 0;
    while (a < size) a += align;
    return a;
}
static uint32_t model_fmix(uint32_t h) { h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16; return h; }
static uint32_t model_owner(uint32_t key, uint32_t shards) { return shards <= 1 ? 0u : (uint32_t)(((uint64_t)model_fmix(key ^ 0x9E3779B9u) * shards) >> 32); }
using Model = std::map<uint32_t, std::vector<uint64_t>>;

// ---- batches --------------------------------------------------------------------------------------------------------------------------
struct Batch {
    std::vector<uint32_t> keys; std::vector<uint8_t> sizes, values;   // exactly as long as their content: a read past an end is the sanitizer's
    uint32_t tb;
    explicit Batch(uint32_t targetBytes) : tb(targetBytes) {}
    void key(uint32_t k, uint32_t size) { keys.push_back(k); sizes.push_back((uint8_t)size); }
    void value(uint32_t win, uint32_t tgt)
    {
        for (int b = 0; b < 4; ++b) values.push_back((uint8_t)(win >> (8 * b)));
        for (uint32_t b = 0; b < tb; ++b) values.push_back((uint8_t)(tgt >> (8 * b)));
    }
};
static uint32_t le(const uint8_t* p, uint32_t bytes) { uint32_t v = 0; for (uint32_t b = 0; b < bytes; ++b) v |= (uint32_t)p[b] << (8 * b); return v; }

// the first `count` keys (from 1 upwards) whose home bucket in a table of n buckets is `home`
static std::vector<uint32_t> keys_at_home(uint32_t n, uint32_t home, size_t count)
{
    std::vector<uint32_t> out;
    for (uint32_t k = 1; out.size() < count; ++k)
        if ((uint32_t)(((uint64_t)model_fmix(k) * n) >> 32) == home) out.push_back(k);
    return out;
}

// a key's list as the table holds it (through mix32 / next_bucket, as a lookup walks); false: not in the table.  probes: buckets visited
static bool lookup(const std::vector<TableBucket>& buckets, const std::vector<uint64_t>& store, uint32_t key, std::vector<uint64_t>& out, uint32_t& probes)
{
    const uint32_t n = (uint32_t)buckets.size(), home = (uint32_t)(((uint64_t)mix32(key) * n) >> 32);
    uint32_t cur = home;
    out.clear();
    for (probes = 1; probes <= n + 1; ++probes) {
        const TableBucket& b = buckets.at(cur);
        bool hasFree = false;
        for (uint32_t j = 0; j < kSlotsPerBucket; ++j) {
            if (!b.size[j]) { hasFree = true; continue; }
            if (b.key[j] != key) continue;
            if (b.size[j] == 1) out.push_back(b.payload[j]);
            else for (uint32_t t = 0; t < b.size[j]; ++t) out.push_back(store.at(b.payload[j] + t));
            return true;
        }
        if (hasFree) return false;
        cur = next_bucket(home, cur, probes, n);
    }
    return false;
}

// the model's update for one batch, then: every key of the model is in the table with exactly its list, and the counters agree
struct MergeRun {
    std::vector<TableBucket> buckets; std::vector<uint64_t> store; Model model; MergeCounters c;
    uint32_t rmOver, maxLocs;
    uint64_t modelLocs = 0;
    std::vector<uint32_t> seen;                                 // every key a batch brought, kept or not
    MergeRun(uint32_t nbuckets, uint32_t rm, uint32_t mx) : buckets(nbuckets), rmOver(rm), maxLocs(mx) {}
    MergeStatus add(uint32_t part, const Batch& B, bool inModel = true)
    {
        const MergeStatus st = merge_part_batch(buckets, store, part, B.keys.data(), B.sizes.data(), B.values.data(), B.keys.size(), B.tb, rmOver, maxLocs, c);
        const uint8_t* v = B.values.data();
        seen.insert(seen.end(), B.keys.begin(), B.keys.end());
        for (size_t i = 0; i < B.keys.size() && inModel; v += (size_t)B.sizes[i] * (4 + B.tb), ++i)
            for (uint32_t t = 0, n = model_size(B.sizes[i], rmOver, maxLocs); t < n; ++t, ++modelLocs)
                model[B.keys[i]].push_back(((uint64_t)(le(v + t * (4 + B.tb) + 4, B.tb) | part << 24) << 32) | le(v + t * (4 + B.tb), 4));
        return st;
    }
    void verify(const char* what) const
    {
        std::vector<uint64_t> got;
        uint32_t probes = 0, longest = 1;
        for (const auto& kv : model) {
            const bool there = lookup(buckets, store, kv.first, got, probes);
            CHECK(there && got == kv.second, "%s: key %u: %s, %zu locations for the model's %zu", what, kv.first, there ? "found" : "missing", got.size(), kv.second.size());
            if (there && probes > longest) longest = probes;
        }
        for (uint32_t k : seen) CHECK(model.count(k) || !lookup(buckets, store, k, got, probes), "%s: key %u is in the table, and in no part of the model", what, k);
        CHECK(c.keysStored == model.size() && c.locations == modelLocs && c.maxProbe == longest, "%s: counters %llu keys / %llu locations / probe %u, model %zu / %llu / %u",
              what, (unsigned long long)c.keysStored, (unsigned long long)c.locations, c.maxProbe, model.size(), (unsigned long long)modelLocs, longest);
    }
};

static int check_merge()
{
    static const uint32_t kSizes[] = {1, 0, 2, 254, 255, 3};
    static const uint32_t kRules[][2] = {{0, 0}, {254, 0}, {1, 0}, {0, 2}, {0, 1}, {254, 2}};   // {rmOver, maxLocs}: none, each alone, together
    int cases = 0;
    char what[96];
    for (uint32_t nb : {2u, 4u, 6u})
        for (uint32_t nparts : {2u, 4u})
            for (uint32_t tb : {2u, 4u})
                for (const auto& r : kRules) {
                    // 4 * nb keys with ONE home bucket: the probe sequence runs home, sibling, on linearly and (nb = 6: from bucket 5) wraps to 0;
                    // key 0 of the pool has one location in every part (inline, then re-homed into the store by part 1, a run from part 2 on),
                    // the others take their sizes in turn, absent (file size 0, or emptied by the rules) in some parts
                    const std::vector<uint32_t> pool = keys_at_home(nb, nb == 2 ? 0 : 2, 4 * nb);
                    MergeRun run(nb, r[0], r[1]);
                    uint32_t win = 0;
                    for (uint32_t part = 0; part < nparts; ++part)
                        for (uint32_t half = 0; half < 2; ++half) {
                            Batch B(tb);
                            for (size_t i = half; i < pool.size(); i += 2) {
                                const uint32_t size = i == 0 ? 1 : kSizes[(i + part) % 6];
                                B.key(pool[i], size);
                                for (uint32_t t = 0; t < size; ++t) B.value(win++, (uint32_t)(i * 1000 + t) & (tb == 2 ? 0xFFFFu : 0xFFFFFFu));
                            }
                            std::snprintf(what, sizeof what, "merge nb=%u parts=%u tb=%u rmOver=%u maxLocs=%u part %u batch %u", nb, nparts, tb, r[0], r[1], part, half);
                            CHECK(run.add(part, B) == MergeStatus::Ok, "%s: status", what);
                            run.verify(what);
                        }
                    CHECK(run.model.count(pool[0]) && run.model[pool[0]].size() == nparts, "%s: the key of every part", what);
                    ++cases;
                }
    // the three failures; the vectors keep their sizes' worth of content (a write past an end is the sanitizer's)
    for (uint32_t nb : {2u, 4u, 6u}) {
        const std::vector<uint32_t> pool = keys_at_home(nb, nb - 1, 4 * nb + 1);
        MergeRun run(nb, 0, 0);
        Batch all(4), more(4);
        for (size_t i = 0; i < 4 * nb; ++i) { all.key(pool[i], 1); all.value((uint32_t)i, 7); }
        more.key(pool[4 * nb], 2); more.value(1, 1); more.value(2, 2);
        CHECK(run.add(0, all) == MergeStatus::Ok, "full table nb=%u: filling it", nb);
        run.verify("full table: filled");
        CHECK(run.add(1, all) == MergeStatus::Ok, "full table nb=%u: merging into it", nb);
        CHECK(run.add(1, more, false) == MergeStatus::TableFull && run.buckets.size() == nb, "full table nb=%u: one more key", nb);
        run.verify("full table: after the refusal");
        ++cases;
    }
    {
        MergeRun run(2, 0, 0);
        Batch B(2);
        B.key(12345, 255);
        for (uint32_t t = 0; t < 255; ++t) B.value(t, t);
        for (uint32_t k = 0; k < 257; ++k) {                    // 257 x 255 = 65 535: the largest bucket there is
            CHECK(run.add(k & 255, B) == MergeStatus::Ok, "large bucket: merge %u", k);
            // (the runs that merges leave behind are dropped here, or the store of this case alone takes 67 MB)
            std::vector<uint64_t> live;
            uint32_t probes;
            lookup(run.buckets, run.store, 12345, live, probes);
            run.store = live;
            for (auto& b : run.buckets) for (uint32_t j = 0; j < kSlotsPerBucket; ++j) if (b.size[j]) b.payload[j] = 0;
        }
        run.verify("large bucket: 65535 locations");
        CHECK(run.add(3, B, false) == MergeStatus::BucketTooLarge, "large bucket: 65536 and more");
        Batch one(2);
        one.key(12345, 1); one.value(9, 9);
        CHECK(run.add(3, one, false) == MergeStatus::BucketTooLarge, "large bucket: 65536");
        run.verify("large bucket: after the refusals");
        ++cases;
    }
    {
        MergeRun run(2, 0, 0);
        Batch ok(4), bad(4);
        ok.key(5, 1); ok.value(1, (1u << 24) - 1); ok.key(6, 2); ok.value(2, 0); ok.value(3, (1u << 24) - 1);
        bad.key(7, 2); bad.value(1, 3); bad.value(2, 1u << 24);
        CHECK(run.add(1, ok) == MergeStatus::Ok, "target ids: 2^24 - 1");
        run.verify("target ids: 2^24 - 1");
        CHECK(run.add(1, bad, false) == MergeStatus::TargetTooLarge, "target ids: 2^24");
        ++cases;
    }
    return cases;
}

static int check_rules()
{
    int cases = 0;
    for (uint32_t rmOver : {0u, 1u, 3u, 254u})
        for (uint32_t maxLocs : {0u, 1u, 2u, 254u})
            for (uint32_t shards : {1u, 3u})
                for (uint32_t align : {1u, kListAlign}) {
                    for (uint32_t fs = 0; fs < 256; ++fs) {
                        const uint32_t want = model_size(fs, rmOver, maxLocs);
                        CHECK(size_after_rules(fs, rmOver, maxLocs) == want, "size_after_rules(%u, %u, %u) = %u, model %u", fs, rmOver, maxLocs, size_after_rules(fs, rmOver, maxLocs), want);
                        for (uint32_t key : {0u, 1u, 2u, 77u, 4096u, 0x9E3779B9u, 0xFFFFFFFEu, 0xFFFFFFFFu}) {
                            uint32_t owners = 0;
                            for (uint32_t idx = 0; idx < shards; ++idx) {
                                const LoadFilter lf{maxLocs, rmOver, idx, shards, align};
                                const uint32_t mine = model_owner(key, shards) == idx ? want : 0, got = effective_size(key, fs, lf);
                                CHECK(got == mine && list_alloc(got, lf.align) == model_alloc(mine, align), "effective_size(key %u, %u; rmOver %u, maxLocs %u, shard %u of %u) = %u, model %u; store %u, model %u",
                                      key, fs, rmOver, maxLocs, idx, shards, got, mine, list_alloc(got, lf.align), model_alloc(mine, align));
                                owners += key_owner(key, shards) == idx;
                            }
                            CHECK(owners == 1, "key %u: %u owners among %u shards", key, owners, shards);
                        }
                    }
                    ++cases;
                }
    return cases;
}

static int check_cut()
{
    static const uint32_t kSizes[] = {2, 0, 1, 254, 255, 3};
    static const uint32_t kRules[][2] = {{0, 0}, {254, 0}, {3, 0}, {0, 2}, {0, 1}, {254, 2}};
    const uint32_t T = 5;                                      // targets 0 .. 4
    static const uint32_t kRanges[][2] = {{0, 1}, {T - 1, T}, {3, 3}, {1, 4}, {0, 0xFFFFFFFFu}};   // first target, last target, empty, inner, everything
    int cases = 0;
    for (uint32_t tb : {2u, 4u})
        for (const auto& r : kRules)
            for (const auto& range : kRanges) {
                Batch B(tb);
                std::vector<uint8_t> wantSizes, wantValues;
                uint64_t wantKept = 0;
                for (uint32_t i = 0; i < 40; ++i) {
                    const uint32_t size = kSizes[i % 6], eff = model_size(size, r[0], r[1]);
                    B.key(i, size);
                    uint32_t n = 0;
                    for (uint32_t t = 0; t < size; ++t) {
                        const uint32_t win = i * 256 + t, tgt = (t * 7 + i) % T;
                        B.value(win, tgt);
                        if (t < eff && tgt >= range[0] && tgt < range[1]) { wantValues.insert(wantValues.end(), B.values.end() - (4 + tb), B.values.end()); ++n; }
                    }
                    wantSizes.push_back((uint8_t)n);
                    wantKept += n;
                }
                const uint64_t kept = cut_batch_values(B.sizes.data(), B.values.data(), (uint32_t)B.keys.size(), tb, range[0], range[1], r[0], r[1]);
                B.values.resize((size_t)std::min<uint64_t>(kept, wantKept) * (4 + tb));
                wantValues.resize(B.values.size());
                CHECK(kept == wantKept && B.sizes == wantSizes && B.values == wantValues, "cut tb=%u rmOver=%u maxLocs=%u targets [%u, %u): %llu values kept, model %llu",
                      tb, r[0], r[1], range[0], range[1], (unsigned long long)kept, (unsigned long long)wantKept);
                ++cases;
            }
    return cases;
}

int main()
{
    const int rules = check_rules(), merge = check_merge(), cut = check_cut();
    if (g_bad) { std::printf("%d MISMATCHES\n", g_bad); return 1; }
    std::printf("rules ok: %d settings\nmerge ok: %d cases\ncut ok: %d cases\n", rules, merge, cut);
    return 0;
}
