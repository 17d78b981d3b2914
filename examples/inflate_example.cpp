// examples/inflate_example.cpp -- a bgzip-compressed file inflated on the device, on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/inflate_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o inflate_example
//   ./inflate_example <database> <file.gz>  > plain
// mc_amd::bgzf_index walks the file's members on the host (no device, no zlib); database::inflate hands them to the device, a wave per
// member (mc_inflate_blocks).  The verdict goes to stderr, the inflated bytes to stdout.  A file that is not BGZF ("foreign") or that the
// device refuses ("corrupt block B reason R") returns 3: such a file is read through zlib instead.
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <iterator>
#include <string>

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: inflate_example <database> <file.gz>\n"; return 2; }
    try {
        std::ifstream is(argv[2], std::ios::binary);
        const std::string bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
        const mc_amd::bgzf_members members = mc_amd::bgzf_index(bytes.data(), bytes.size());
        if (members.verdict != MC_BGZF_OK) { std::cerr << "foreign at byte " << members.offence << "\n"; return 3; }
        mc_amd::database db;
        db.read(argv[1]);
        const auto r = db.inflate(bytes.data(), bytes.size(), members);
        if (r.verdict == MC_INFLATE_CORRUPT) { std::cerr << "corrupt block " << r.block << " reason " << r.reason << "\n"; return 3; }
        if (r.verdict != MC_INFLATE_OK) { std::cerr << "refused: verdict " << r.verdict << " block " << r.block << "\n"; return 3; }
        std::cerr << "ok: " << members.blocks.size() << " blocks, " << bytes.size() << " bytes in, " << r.bytes.size() << " bytes out\n";
        std::cout.write(r.bytes.data(), std::streamsize(r.bytes.size()));
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;
        return 1;
    }
    return 0;
}
