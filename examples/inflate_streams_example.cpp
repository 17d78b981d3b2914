// examples/inflate_streams_example.cpp -- gzip-compressed genome files inflated on the device, a wave per file, on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/inflate_streams_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o inflate_streams_example
//   ./inflate_streams_example <database> <file.gz>...  > plain
// mc_amd::gzip_hint reads each file's first header and its trailing ISIZE on the host (no device, no zlib); database::inflate_streams
// hands the files it takes to the device in one call (mc_inflate_streams).  Every file has its own verdict, one line on stderr:
// "<file>: ok M members B bytes", "<file>: foreign reason R" (the hint refused it) or "<file>: refused reason R" (the device did).  The
// accepted files' bytes go to stdout in the order of the arguments.  3 is returned if any file was left out: such a file is read through
// zlib instead.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <string>
#include <vector>

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: inflate_streams_example <database> <file.gz>...\n"; return 2; }
    try {
        std::vector<std::string> names, files;
        std::vector<std::uint64_t> room;
        int left = 0;
        for (int a = 2; a < argc; ++a) {
            std::ifstream is(argv[a], std::ios::binary);
            std::string bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
            const mc_amd::gzip_file_hint h = mc_amd::gzip_hint(bytes.data(), bytes.size());
            if (h.verdict != MC_GZIP_OK) { std::cerr << argv[a] << ": foreign reason " << h.offence << "\n"; ++left; continue; }
            names.push_back(argv[a]); files.push_back(std::move(bytes)); room.push_back(h.isize);
        }
        mc_amd::database db;
        db.read(argv[1]);
        const auto r = db.inflate_streams(files, room);
        for (std::size_t i = 0; i < files.size(); ++i) {
            if (r.results[i].reason) { std::cerr << names[i] << ": refused reason " << r.results[i].reason << "\n"; ++left; continue; }
            std::cerr << names[i] << ": ok " << r.results[i].members << " members " << r.plain[i].size() << " bytes\n";
            std::cout.write(r.plain[i].data(), std::streamsize(r.plain[i].size()));
        }
        if (left) return 3;
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
