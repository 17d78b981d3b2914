// examples/parse_mates_example.cpp -- paired reads out of two mate files (R1, R2) without a cutting loop or an interleave of one's own.
//   g++ -std=c++14 -Iinclude examples/parse_mates_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o parse_mates_example
//   ./parse_mates_example <database> <mates1.fa | .fq> <mates2.fa | .fq>
// Both files' bytes go to the device as they are: database::parse_mates cuts them there (mc_parse_mates) and prints, per query,
//   <name> TAB <len1> TAB <len2> TAB <header of the first mate> TAB <header of the second mate>
// and query_batch::add_file_mates hands the same bytes to a batch whose pairs the device cuts at submission; per query it prints
//   <target of the best candidate or -> TAB <its hits>
// Files the device refuses (irregular, unequal record counts, or more than one batch takes) say so on stderr and return 3.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

static std::string slurp(const char* path)
{
    std::ifstream is(path, std::ios::binary);
    return std::string((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
}

int main(int argc, char** argv)
{
    if (argc < 4) { std::cerr << "usage: parse_mates_example <database> <mates1> <mates2>\n"; return 2; }
    try {
        mc_amd::database db;
        db.read(argv[1]);
        const std::string b1 = slurp(argv[2]), b2 = slurp(argv[3]);

        const auto p = db.parse_mates(b1.data(), b1.size(), b2.data(), b2.size());
        if (p.verdict == MC_PARSE_UNEQUAL) { std::cerr << "refused: " << p.records1 << " records beside " << p.records2 << "\n"; return 3; }
        if (p.verdict != MC_PARSE_OK) { std::cerr << "refused: verdict " << p.verdict << " at byte " << p.offence << " of range " << p.offenceRange << "\n"; return 3; }
        for (std::uint32_t q = 0; q < p.queries; ++q)
            std::cout << p.names.substr(p.nameOff[q], p.nameOff[q + 1] - p.nameOff[q]) << '\t' << p.qinfo[4 * q + 1] << '\t' << p.qinfo[4 * q + 3] << '\t'
                      << b1.substr(p.hdr[4 * q], p.hdr[4 * q + 1]) << '\t' << b2.substr(p.hdr[4 * q + 2], p.hdr[4 * q + 3]) << '\n';

        mc_amd::query_batch batch(db, 1);
        if (!batch.add_file_mates(0, b1.data(), b1.size(), b2.data(), b2.size())) { std::cerr << "refused: the files exceed one batch\n"; return 3; }
        db.query_gpu_async(batch, 0, mc_amd::taxon_rank(0));
        auto& host = batch.host_data(0);
        host.wait_for_results();
        const mc_batch_record_info info = host.records();
        if (info.verdict != MC_PARSE_OK) { std::cerr << "refused: verdict " << info.verdict << " at byte " << info.offence << "\n"; return 3; }
        for (std::size_t q = 0; q < host.num_queries(); ++q) {
            const auto top = host.top_candidates(q);
            if (top.first->hits) std::cout << top.first->tgt << '\t' << top.first->hits << '\n';
            else std::cout << "-\t0\n";
        }
        host.clear();
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
