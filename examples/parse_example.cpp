// examples/parse_example.cpp -- reads out of a FASTA / FASTQ file without a cutting loop of one's own, on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/parse_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o parse_example
//   ./parse_example <database> <reads.fa | reads.fq> [pairs: 0 | 1]
// The file's bytes go to the device as they are: database::parse_records cuts them there (mc_parse_records) and prints, per query,
//   <name> TAB <len1> TAB <len2> TAB <header of the first record>
// and query_batch::add_file_bytes hands the same bytes to a batch whose reads the device cuts at submission; per query it prints
//   <target of the best candidate or -> TAB <its hits>
// A file the device refuses (irregular, or more than one batch takes) says so on stderr and returns 3.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: parse_example <database> <reads> [pairs]\n"; return 2; }
    try {
        const bool pairs = argc > 3 && std::stoi(argv[3]) != 0;
        mc_amd::database db;
        db.read(argv[1]);
        std::ifstream is(argv[2], std::ios::binary);
        const std::string bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());

        const auto p = db.parse_records(bytes.data(), bytes.size(), pairs);
        if (p.verdict != MC_PARSE_OK) { std::cerr << "refused: verdict " << p.verdict << " at byte " << p.offence << "\n"; return 3; }
        for (std::uint32_t q = 0; q < p.queries; ++q) {
            const std::uint32_t r = pairs ? 2 * q : q;
            std::cout << p.names.substr(p.nameOff[q], p.nameOff[q + 1] - p.nameOff[q]) << '\t' << p.qinfo[4 * q + 1] << '\t' << p.qinfo[4 * q + 3] << '\t'
                      << bytes.substr(p.hdr[2 * r], p.hdr[2 * r + 1]) << '\n';
        }

        mc_amd::query_batch batch(db, 1);
        if (!batch.add_file_bytes(0, bytes.data(), bytes.size(), pairs)) { std::cerr << "refused: the file exceeds one batch\n"; return 3; }
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
