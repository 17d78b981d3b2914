// examples/table_info_example.cpp -- what a loaded table holds (print_content_properties, printing.cpp:662-696; print_feature_counts and
// print_feature_map, host_hashmap.hpp:413-445) on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/table_info_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o table_info_example
//   ./table_info_example <database> [part] [features to list, default 10]
// Reads one part of the database (part 0 by default), prints the statistics of its location lists from the histogram the device made
// (database::table_histogram -> mc_amd::table_statistics), then the first features in ascending order with their lists
// (database::table_features, database::table_lookup) as the reference's `info <db> featuremap` prints them.
#include "metacache_amd.hpp"

#include <iostream>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 2) { std::cerr << "usage: table_info_example <database> [part] [features]\n"; return 2; }
    try {
        const int part = argc > 2 ? std::stoi(argv[2]) : 0;
        const std::size_t show = argc > 3 ? std::size_t(std::stoul(argv[3])) : 10;
        mc_amd::database db;
        db.read(argv[1], part);
        const auto h = db.table_histogram();
        const mc_amd::table_statistics lss(h.hist, h.dead);
        std::cout << "buckets            " << lss.buckets() << '\n'
                  << "bucket size        max: " << double(lss.max) << " mean: " << lss.mean() << " +/- " << lss.stddev() << " <> " << lss.skewness() << '\n'
                  << "features           " << lss.features << '\n'
                  << "dead features      " << lss.dead << '\n'
                  << "locations          " << lss.locations << '\n';
        const auto f = db.table_features();
        const std::size_t n = std::min(show, f.features.size());
        mc_amd::span<const std::uint32_t> first;
        first.first = f.features.data(); first.last = f.features.data() + n;
        const auto lists = db.table_lookup(first);
        for (std::size_t i = 0; i < n; ++i) {
            std::cout << f.features[i] << " -> ";
            for (std::uint64_t k = lists.offsets[i]; k < lists.offsets[i + 1]; ++k)
                std::cout << '(' << lists.locations[k].tgt << ',' << lists.locations[k].win << ')';
            std::cout << '\n';
        }
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;                  // main.cpp:65-68
        return 1;
    }
    return 0;
}
