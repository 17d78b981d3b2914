// examples/parse_cut_example.cpp -- the batches of a FASTA / FASTQ file without an index loop of one's own, on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/parse_cut_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o parse_cut_example
//   ./parse_cut_example <database> <reads.fa | reads.fq> <records per batch> [pairs: 0 | 1] [open: 0 | 1]
// The file's bytes go to the device as they are: database::parse_cut finds the batch borders there (mc_parse_cut) and prints
//   status TAB <whole> TAB <batches> TAB <consumed> TAB <record starts seen> TAB <largest batch in bytes> TAB <half pair>
//   <cuts[0]> ... <cuts[batches]>, one a line
// A file the device refuses (irregular) says so on stderr and returns 3.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 4) { std::cerr << "usage: parse_cut_example <database> <reads> <records per batch> [pairs] [open]\n"; return 2; }
    try {
        const std::uint32_t perBatch = std::uint32_t(std::stoul(argv[3]));
        const bool pairs = argc > 4 && std::stoi(argv[4]) != 0, open = argc > 5 && std::stoi(argv[5]) != 0;
        mc_amd::database db;
        db.read(argv[1]);
        std::ifstream is(argv[2], std::ios::binary);
        const std::string bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());

        const auto c = db.parse_cut(bytes.data(), bytes.size(), perBatch, pairs, open);
        if (c.verdict != MC_PARSE_OK) { std::cerr << "refused: verdict " << c.verdict << " at byte " << c.offence << "\n"; return 3; }
        std::cout << "status\t" << c.whole << '\t' << c.cuts.size() - 1 << '\t' << c.consumed << '\t' << c.seen << '\t' << c.longest << '\t' << (c.halfPair ? 1 : 0) << '\n';
        for (const std::uint64_t at : c.cuts) std::cout << at << '\n';
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
