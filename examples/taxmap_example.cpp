// examples/taxmap_example.cpp -- targets ranked from accession2taxid tables on the device, on metacache_amd.hpp (mc_amd::accession_mapper).
//   g++ -std=c++14 -Iinclude examples/taxmap_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o taxmap_example
//   ./taxmap_example <names.txt> <table> <table> ...
//   e.g. the table tests/golden/build_in/taxonomy/toy.accession2taxid
// names.txt holds one target name per line, followed by a blank and 0 where the name takes no taxid (a target that has a parent already).
// The tables are read in the order given, each without its first line, until no name is wanted; per name, in ascending order, it prints
//   <name> TAB <taxid> TAB <number of the table, from 0> TAB <offset of the row behind the table's first line>
// or <name> TAB - where no row named it.  A table the device refuses says so on stderr and returns 3.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <map>
#include <sstream>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: taxmap_example <names.txt> <table> <table> ...\n"; return 2; }
    try {
        std::map<std::string, std::uint8_t> byName;
        std::ifstream ns(argv[1]);
        for (std::string l; std::getline(ns, l);) {
            std::istringstream is(l);
            std::string name; int wanted = 1;
            if (!(is >> name)) continue;
            is >> wanted;
            byName[name] = wanted ? 1 : 0;
        }
        std::vector<std::string> names;
        std::vector<std::uint8_t> wanted;
        for (const auto& kv : byName) { names.push_back(kv.first); wanted.push_back(kv.second); }

        mc_amd::accession_mapper mapper;
        mapper.begin(names, wanted);
        std::vector<int> tableOfCall;
        std::uint64_t remaining = 1;
        for (int a = 2; a < argc && remaining; ++a) {
            std::ifstream is(argv[a], std::ios::binary);
            if (!is.good()) continue;
            const std::string bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
            const std::size_t nl = bytes.find('\n');
            if (nl == std::string::npos || nl + 1 == bytes.size()) continue;       // nothing behind the first line
            const auto st = mapper.add(bytes.data() + nl + 1, bytes.size() - nl - 1);
            tableOfCall.push_back(a - 2);
            if (st.verdict != MC_TAXMAP_OK) { std::cerr << "refused: " << argv[a] << ": verdict " << st.verdict << " at byte " << st.offence << "\n"; return 3; }
            remaining = st.remaining;
        }
        const auto r = mapper.result();
        for (std::size_t i = 0; i < names.size(); ++i) {
            const std::uint64_t pos = r.position[i];
            if (pos == ~std::uint64_t(0)) std::cout << names[i] << "\t-\n";
            else std::cout << names[i] << '\t' << r.taxid[i] << '\t' << tableOfCall[pos >> 32] << '\t' << (pos & 0xFFFFFFFFull) << '\n';
        }
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
