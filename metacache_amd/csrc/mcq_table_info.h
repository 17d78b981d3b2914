// metacache_amd/csrc/mcq_table_info.h -- `mcq info <db> statistics | locations | featurecounts` (aliases stat, loc, featuremap, features)
// behind MCQ_INFO_DEVICE=1: what the reference prints from its hash table (print_content_properties, printing.cpp:662-696;
// location_list_size_statistics, print_feature_map and print_feature_counts, host_hashmap.hpp:376-445) from the table in HBM, through
// mc_table_histogram / mc_table_features / mc_table_lookup.  Every part of the database is opened on its own, one after the other
// (mc_config.single_part); the lines of a part come in ascending feature order (the reference walks its own hash slots), the feature map
// in pieces of kInfoLookupKeys features, so the location store is never held on the host.  Part of mcq_main.cpp.
#pragma once

inline bool info_table_topic(const std::string& what)
{
    return what == "statistics" || what == "stat" || what == "locations" || what == "loc" || what == "featuremap" || what == "features" || what == "featurecounts";
}

constexpr uint64_t kInfoLookupKeys = 1ull << 20;

struct SizeStatistics {                                                    // statistics_accumulator over a histogram of list sizes: exact integer sums,
    uint64_t n = 0, s1 = 0, s2 = 0, s3 = 0, max = 0;                        // then the reference's arithmetic on doubles (stat_moments.hpp:685-707, :836-854)
    void add(const uint64_t hist[256])
    {
        for (uint64_t s = 1; s < 256; ++s) {
            if (!hist[s]) continue;
            n += hist[s]; s1 += s * hist[s]; s2 += s * s * hist[s]; s3 += s * s * s * hist[s];
            max = std::max(max, s);
        }
    }
    double mean() const { return n ? double(s1) / double(n) : 0.0; }
    double variance() const { return n < 2 ? 0.0 : (double(s2) - double(s1) * double(s1) / double(n)) / (double(n) - 1.0); }
    double stddev() const { return std::sqrt(variance()); }
    double skewness() const
    {
        const double cm2 = variance();
        if (n < 2 || !(cm2 > 0.0)) return 0.0;
        const double dn = double(n), n2 = dn * dn, d1 = double(s1);
        return ((n2 * double(s3) - 3.0 * dn * (d1 * double(s2)) + 2.0 * (d1 * d1 * d1)) / (dn * n2)) / std::pow(cm2, 1.5);
    }
};

// the table of keys + dead keys as the reference sizes it: reserve_keys at the database's default load factor, in single precision
// (hash_multimap.hpp:552-554)
inline uint64_t reference_buckets(uint64_t keys) { return uint64_t(1.0f + float(keys) / 0.8f); }

inline void print_size_block(uint64_t buckets, const SizeStatistics& st, uint64_t dead)
{
    std::cout << "buckets            " << buckets << '\n'
              << "bucket size        max: " << double(st.max) << " mean: " << st.mean() << " +/- " << st.stddev() << " <> " << st.skewness() << '\n'
              << "features           " << st.n << '\n'
              << "dead features      " << dead << '\n'
              << "locations          " << st.s1 << '\n';
}

// after print_static_properties: the content block, then -- for the map and the counts -- the lines between the two rules
inline int info_table_content(const std::string& name, const std::string& what, uint64_t parts, uint64_t targets, uint64_t rankedTargets, uint64_t taxaInTree)
{
    using clock = std::chrono::steady_clock;
    struct Timed { uint64_t calls = 0; double ms = 0; } tHist, tFeat, tLook;
    auto timed = [](Timed& t, auto&& call) {
        const auto t0 = clock::now();
        const int rc = call();
        t.ms += std::chrono::duration<double, std::milli>(clock::now() - t0).count();
        ++t.calls;
        return rc;
    };
    struct Ctx {
        mc_ctx* c = nullptr;
        ~Ctx() { close(); }
        void close() { if (c) mc_destroy(c); c = nullptr; }
        void open(const std::string& db, int part)
        {
            close();
            mc_config cfg; mc_config_default(&cfg);
            cfg.kmerlen = cfg.sketchlen = cfg.winlen = cfg.winstride = 0;
            cfg.num_slots = 1;
            cfg.single_part = part;
            if (mc_open_database(db.c_str(), &cfg, &c) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
        }
    } db;
    auto check = [&](int rc) { if (rc != MC_OK) throw std::runtime_error(mc_last_error(db.c)); };
    const bool several = parts > 1;
    const bool counts = what == "featurecounts", map = !counts && what != "statistics" && what != "stat";

    struct PartInfo { uint64_t hist[256]; uint64_t dead = 0; };
    std::vector<PartInfo> info(parts);
    for (uint64_t p = 0; p < parts; ++p) {
        db.open(name, several ? int(p) : -1);
        check(timed(tHist, [&] { return mc_table_histogram(db.c, info[p].hist, &info[p].dead); }));
    }
    std::cout << "------------------------------------------------\n"
              << "database parts     " << parts << '\n';
    if (targets > 0)
        std::cout << "targets            " << targets << '\n'
                  << "ranked targets     " << rankedTargets << '\n'
                  << "taxa in tree       " << taxaInTree << '\n';
    SizeStatistics all;
    uint64_t allBuckets = 0, allDead = 0;
    for (const PartInfo& pi : info) all.add(pi.hist);
    if (all.n > 0) {
        for (uint64_t p = 0; p < parts; ++p) {
            SizeStatistics st;
            st.add(info[p].hist);
            const uint64_t buckets = reference_buckets(st.n + info[p].dead);
            allBuckets += buckets; allDead += info[p].dead;
            if (!several) continue;
            std::cout << "------------------------------------------------\n"
                      << "database part " << (p + 1) << " / " << parts << ":\n";
            print_size_block(buckets, st, info[p].dead);
        }
        if (several) std::cout << "------------------------------------------------\n" << "complete database (all parts):\n";
        print_size_block(allBuckets, all, allDead);
    }
    std::cout << "------------------------------------------------\n";
    if (counts || map) {
        std::cout << "===================================================\n";
        std::string text;
        std::vector<uint32_t> keys, sizes;
        std::vector<uint64_t> offsets;
        std::vector<mc_location> locs;
        for (uint64_t p = 0; p < parts; ++p) {
            if (several) { db.open(name, int(p)); std::cout << "database part " << (p + 1) << ":\n"; }
            uint64_t num = 0;
            check(timed(tFeat, [&] { return mc_table_features(db.c, nullptr, nullptr, 0, &num, 0); }));
            keys.resize(num); sizes.resize(num);
            if (num) check(timed(tFeat, [&] { return mc_table_features(db.c, keys.data(), sizes.data(), num, &num, 0); }));
            for (uint64_t done = 0; done < num; done += kInfoLookupKeys) {
                const uint64_t m = std::min(kInfoLookupKeys, num - done);
                text.clear();
                if (counts) {
                    for (uint64_t i = done; i < done + m; ++i) { text += std::to_string(keys[i]); text += " -> "; text += std::to_string(sizes[i]); text += '\n'; }
                } else {
                    uint64_t total = 0;
                    for (uint64_t i = done; i < done + m; ++i) total += sizes[i];
                    offsets.resize(m + 1); locs.resize(total);
                    check(timed(tLook, [&] { return mc_table_lookup(db.c, keys.data() + done, m, offsets.data(), locs.data(), total, 0); }));
                    for (uint64_t i = 0; i < m; ++i) {
                        text += std::to_string(keys[done + i]); text += " -> ";
                        for (uint64_t k = offsets[i]; k < offsets[i + 1]; ++k) {
                            text += '('; text += std::to_string(locs[k].tgt); text += ','; text += std::to_string(locs[k].win); text += ')';
                        }
                        text += '\n';
                    }
                }
                std::cout.write(text.data(), (std::streamsize)text.size());
            }
        }
        std::cout << "===================================================\n";
    }
    if (std::getenv("MCQ_PROFILE"))
        std::cerr << "mcq profile: table info: mc_table_histogram " << tHist.calls << " calls " << tHist.ms << " ms, mc_table_features " << tFeat.calls
                  << " calls " << tFeat.ms << " ms, mc_table_lookup " << tLook.calls << " calls " << tLook.ms << " ms\n";
    return 0;
}
