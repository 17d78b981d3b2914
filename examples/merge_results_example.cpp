// examples/merge_results_example.cpp -- per-part result files merged on the device, on metacache_amd.hpp (mc_amd::result_merger).
//   g++ -std=c++14 -Iinclude examples/merge_results_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o merge_results_example
//   ./merge_results_example <taxa.txt> <max candidates> <part file> <part file> ...
//   e.g. the part files tests/golden/merge_in/part0.txt and part1.txt
// taxa.txt holds the taxonomy as arrays, one taxon per line: <taxid> <rank 0..21> <21 lineage entries: taxon index + 1, 0 = none>.
// The files are folded in the order given (merge below species, as `merge` does by default); per query it prints
//   <id> TAB <header> TAB <taxid:hits,...> TAB <taxid of the assignment or 0> TAB <its rank, 21 = unclassified>
// with the vote of `merge`'s defaults (hitmin 5, hitdiff 1, highest domain).  A file the device refuses says so on stderr and returns 3.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <sstream>
#include <string>

// the column of top_hits behind query_id in the file's TABLE_LAYOUT line (0: none)
static std::uint32_t tophits_column(const std::string& bytes)
{
    const std::size_t at = bytes.find("# TABLE_LAYOUT:");
    if (at == std::string::npos) return 0;
    const std::string line = bytes.substr(at + 15, bytes.find('\n', at) - at - 15);
    std::uint32_t col = 0;
    for (std::size_t p = 0;;) {
        const std::size_t bar = line.find('|', p);
        if (line.substr(p, bar == std::string::npos ? bar : bar - p).find("top_hits") != std::string::npos) return col;
        if (bar == std::string::npos) return 0;
        p = bar + 1;
        ++col;
    }
}

int main(int argc, char** argv)
{
    if (argc < 5) { std::cerr << "usage: merge_results_example <taxa.txt> <max candidates> <part file> <part file> ...\n"; return 2; }
    try {
        std::vector<std::int64_t> ids;
        std::vector<std::uint8_t> rank;
        std::vector<std::uint32_t> lin;
        std::ifstream ts(argv[1]);
        for (std::string l; std::getline(ts, l);) {
            std::istringstream is(l);
            std::int64_t id; unsigned r;
            if (!(is >> id >> r)) continue;
            ids.push_back(id); rank.push_back(std::uint8_t(r));
            for (int k = 0; k < MC_NUM_RANKS; ++k) { std::uint32_t x = 0; is >> x; lin.push_back(x); }
        }
        const std::uint32_t maxCand = std::uint32_t(std::stoul(argv[2]));

        mc_amd::result_merger merger;
        merger.set_taxa(lin.data(), rank.data(), ids.data(), ids.size());
        merger.begin(1024, maxCand, 4);
        std::vector<std::string> files;                        // by call number, for the header places
        for (int a = 3; a < argc; ++a) {
            std::ifstream is(argv[a], std::ios::binary);
            const std::string bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
            const std::uint32_t col = tophits_column(bytes);
            if (bytes.empty() || !col) { std::cerr << "refused: " << argv[a] << " is no result file\n"; return 3; }
            const auto st = merger.add(bytes.data(), bytes.size(), col);
            while (files.size() < merger.calls()) files.push_back(bytes);   // (a retry after a reserve is a call of its own)
            if (st.verdict != MC_MERGE_OK) { std::cerr << "refused: " << argv[a] << ": verdict " << st.verdict << " at byte " << st.offence << "\n"; return 3; }
        }
        const auto m = merger.lists();
        mc_classify_options opt;
        mc_classify_options_default(&opt);
        opt.hits_min = 5; opt.lowest_rank = 4; opt.highest_rank = 19;
        const auto assigned = merger.classify(opt);
        for (std::uint64_t q = 0; q < m.queries; ++q) {
            const std::uint32_t* h = &m.header_place[3 * q];
            std::cout << q + 1 << '\t' << (h[2] ? files[h[0]].substr(h[1], h[2]) : std::string()) << '\t';
            for (std::uint32_t j = 0; j < maxCand && m.lists[q * maxCand + j].hits; ++j)
                std::cout << (j ? "," : "") << ids[m.lists[q * maxCand + j].taxon - 1] << ':' << m.lists[q * maxCand + j].hits;
            std::cout << '\t' << (assigned[q].taxon ? ids[assigned[q].taxon - 1] : 0) << '\t' << (assigned[q].info & 0xFFu) << '\n';
        }
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
