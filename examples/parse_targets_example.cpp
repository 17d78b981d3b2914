// examples/parse_targets_example.cpp -- reference genomes cut into build targets without a reader loop of one's own, on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/parse_targets_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o parse_targets_example
//   ./parse_targets_example <database to write> <genomes.fa> [more.fa ...]
// The files' bytes go to the device back to back, as they are: database::parse_targets cuts them there (mc_parse_targets) and the program prints
//   status TAB <records> TAB <records with a sequence> TAB <longest sequence>
//   <file> TAB <number inside the file> TAB <header> TAB <length> TAB <FNV-1a of the sequence, hex>     one line per record, empty ones included
// then adds every record with a sequence to a builder under its header's first word and writes the database.
// A range the device refuses (a file that does not begin with '>', a '+' line, ...) says so on stderr and returns 3.
#include "metacache_amd.hpp"

#include <fstream>
#include <iomanip>
#include <iostream>
#include <iterator>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: parse_targets_example <database to write> <genomes.fa> [more.fa ...]\n"; return 2; }
    try {
        std::string bytes;
        std::vector<std::uint64_t> fileOff(1, 0);
        for (int i = 2; i < argc; ++i) {
            std::ifstream is(argv[i], std::ios::binary);
            if (!is) throw std::runtime_error(std::string("cannot read ") + argv[i]);
            bytes.append((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
            fileOff.push_back(bytes.size());
        }
        mc_amd::database db;
        db.create();
        const mc_amd::parsed_targets p = db.parse_targets(bytes.data(), bytes.size(), fileOff);
        if (p.verdict != MC_PARSE_OK) { std::cerr << "refused: verdict " << p.verdict << " at byte " << p.offence << " in file " << p.file << "\n"; return 3; }
        std::cout << "status\t" << p.records << '\t' << p.withSequence << '\t' << p.longest << '\n';
        for (std::size_t r = 0; r < p.records; ++r) {
            const mc_parse_target& t = p.targets[r];
            std::uint64_t h = 14695981039346656037ull;
            for (std::uint32_t k = 0; k < t.len; ++k) h = (h ^ p.seq[t.seq_off + k]) * 1099511628211ull;
            std::cout << t.file << '\t' << t.index << '\t' << p.header(bytes.data(), r) << '\t' << t.len << '\t' << std::hex << h << std::dec << '\n';
        }

        mc_config c;
        mc_config_default(&c);
        mc_builder* b = nullptr;
        if (mc_build_begin(&c, &b) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
        struct Free { mc_builder* b; ~Free() { mc_build_free(b); } } guard{b};
        for (std::size_t r = 0; r < p.records; ++r) {
            const mc_parse_target& t = p.targets[r];
            if (t.len == 0) continue;
            const std::string header = p.header(bytes.data(), r), name = header.substr(0, header.find(' '));
            if (mc_build_add_target_src(b, reinterpret_cast<const char*>(p.seq.data() + t.seq_off), t.len, name.c_str(), 0, argv[2 + t.file], t.index) != MC_OK)
                throw std::runtime_error(mc_build_last_error(b));
        }
        if (mc_build_finish(b, nullptr) != MC_OK || mc_build_write(b, argv[1], nullptr, 0) != MC_OK) throw std::runtime_error(mc_build_last_error(b));
        std::cout << "written\t" << argv[1] << '\t' << p.withSequence << " targets\n";
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
