// tools/bgzf_rules_check.cpp -- the host code that reads untrusted bytes for the device inflate (csrc/bgzf_rules.h: the walk behind
// mc_bgzf_index and the row checks of MC_INFLATE_HOST) as a stand-alone program, so that it can run under a sanitizer without a GPU:
//   g++ -std=c++14 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/bgzf_rules_check.cpp -o bgzf_rules_check
//   ./bgzf_rules_check file...        (tools/bgzf_rules_cases.py writes the index cases of the tests as files)
// Every file is copied into a heap block of exactly its size, so that one byte read past the end is an error.  Per file it walks the
// bytes with every capacity from 0 to the member count, checks the rows it gets, then every prefix of the file and -- seeded -- copies
// with single damaged bytes; it prints "<file> members out_bytes verdict offence".  No library, no device: the header alone.
#include "../metacache_amd/csrc/bgzf_rules.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <vector>

static int check(const unsigned char* src, size_t n, bool print, const char* name)
{
    unsigned char* exact = (unsigned char*)std::malloc(n ? n : 1);
    if (n) std::memcpy(exact, src, n);
    uint64_t info[4] = {0, 0, 0, 0};
    mcamd::bgzf_index(exact, n, nullptr, 0, info);
    const uint64_t members = info[0];
    int bad = 0;
    for (uint64_t cap = 0; cap <= members; cap += (members > 64 && cap + 1 < members - 1) ? members / 7 + 1 : 1) {
        mc_bgzf_block* rows = (mc_bgzf_block*)std::malloc(cap ? cap * sizeof(mc_bgzf_block) : 1);
        uint64_t again[4] = {0, 0, 0, 0};
        mcamd::bgzf_index(exact, n, rows, cap, again);
        if (std::memcmp(info, again, sizeof info) != 0) bad = 1;
        if (!mcamd::bgzf_rows_ok(rows, cap, n)) bad = 1;                    // what the walk gives passes the row checks
        if (cap > 1) {                                                      // and rows that are damaged do not get through them unread
            mc_bgzf_block keep = rows[cap - 1];
            rows[cap - 1].in_off = ~0ull; if (mcamd::bgzf_rows_ok(rows, cap, n)) bad = 1;
            rows[cap - 1] = keep; rows[cap - 1].in_len = 0xFFFFFFFFu; if (mcamd::bgzf_rows_ok(rows, cap, n)) bad = 1;
            rows[cap - 1] = keep; rows[cap - 1].out_off = ~0ull; rows[cap - 1].out_len = 65536; if (mcamd::bgzf_rows_ok(rows, cap, n)) bad = 1;
            rows[cap - 1] = keep; rows[cap - 1].out_len = 65537; if (mcamd::bgzf_rows_ok(rows, cap, n)) bad = 1;
            rows[cap - 1] = rows[0]; if (rows[0].in_len && mcamd::bgzf_rows_ok(rows, cap, n)) bad = 1;
        }
        std::free(rows);
    }
    if (print) std::printf("%s %llu %llu %llu %llu\n", name, (unsigned long long)info[0], (unsigned long long)info[1], (unsigned long long)info[2], (unsigned long long)info[3]);
    std::free(exact);
    return bad;
}

int main(int argc, char** argv)
{
    int bad = 0;
    for (int a = 1; a < argc; ++a) {
        std::ifstream is(argv[a], std::ios::binary);
        if (!is) { std::fprintf(stderr, "cannot read %s\n", argv[a]); return 2; }
        std::vector<unsigned char> bytes((std::istreambuf_iterator<char>(is)), std::istreambuf_iterator<char>());
        bad |= check(bytes.data(), bytes.size(), true, argv[a]);
        // every prefix of a small file, the prefixes around the member borders of a large one
        for (size_t n = 0; n < bytes.size(); n += (bytes.size() > 4096 && n > 64 && n + 64 < bytes.size()) ? 997 : 1) bad |= check(bytes.data(), n, false, argv[a]);
        // single damaged bytes, mostly in the first member's header
        uint64_t seed = 88172645463325252ull + (uint64_t)a;
        for (int k = 0; k < 2000 && !bytes.empty(); ++k) {
            seed ^= seed << 13; seed ^= seed >> 7; seed ^= seed << 17;
            std::vector<unsigned char> hurt(bytes);
            const size_t at = (size_t)((seed >> 8) % ((k & 1) ? std::min<size_t>(hurt.size(), 40) : hurt.size()));
            hurt[at] = (unsigned char)(seed >> 40);
            bad |= check(hurt.data(), hurt.size(), false, argv[a]);
        }
    }
    if (bad) { std::fprintf(stderr, "bgzf_rules_check: an inconsistency\n"); return 1; }
    return 0;
}
