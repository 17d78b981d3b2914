// tools/gzip_rules_check.cpp -- the host code that reads untrusted bytes for the device inflate of whole gzip files (csrc/gzip_rules.h:
// the header walk behind mc_gzip_hint and the row checks of mc_inflate_streams(MC_INFLATE_HOST)) as a stand-alone program, so that it
// can run under a sanitizer without a GPU:
//   g++ -std=c++14 -g -fsanitize=address,undefined -fno-sanitize-recover=all -Iinclude tools/gzip_rules_check.cpp -o gzip_rules_check
//   ./gzip_rules_check file...        (tools/gzip_rules_cases.py writes the rows of the tests as files)
// Every range is copied into a heap block of exactly its size, so that one byte read past the end is an error.  Per file it takes the
// hint of the whole file, of every prefix and -- seeded -- of 2 000 copies with single damaged bytes, walks the header of a member at
// every offset of the first 600 bytes as a first and as a later member, and puts rows made from the file through the row checks; it
// prints "<file> verdict payload isize offence".  No library, no device: the header alone.
#include "../metacache_amd/csrc/gzip_rules.h"

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
    uint64_t info[4] = {9, 9, 9, 9};
    mcamd::gzip_hint(exact, n, info);
    int bad = 0;
    // what the hint says is consistent with itself and stays inside the range
    if (info[0] == MC_GZIP_OK) { if (info[3] != 0 || info[1] < 10 || info[1] + 8 > n) bad = 1; }
    else if (info[0] != MC_GZIP_FOREIGN || info[3] == 0 || info[1] != 0) bad = 1;
    if (n >= 4 && info[2] != mcamd::gzip_u32(exact + n - 4)) bad = 1;
    // a member's header at every offset of the front, as a first and as a later member: the verdicts differ only in the reason for bytes
    // that are no magic
    for (uint64_t p = 0; p < n && p < 600; ++p) {
        uint64_t a = 0, b = 0;
        const uint32_t ra = mcamd::gzip_header(exact, n, p, true, a), rb = mcamd::gzip_header(exact, n, p, false, b);
        if ((ra == 0) != (rb == 0) || (ra == 0 && (a != b || a < p + 10 || a > n))) bad = 1;
        if (ra && ra != rb && !(ra == MC_INFLATE_R_HEADER && rb == MC_INFLATE_R_TRAILING)) bad = 1;
    }
    // rows made from the range: what is good passes, what is damaged does not get through unread
    if (n >= mcamd::kGzipMinRow) {
        mc_gzip_stream* rows = (mc_gzip_stream*)std::malloc(3 * sizeof(mc_gzip_stream));
        const uint64_t half = n / 2;
        rows[0] = {0, n, 0, info[2] & 0x7FFFFFFFull};
        rows[1] = {0, half >= mcamd::kGzipMinRow ? half : n, 1ull << 31, 5};
        rows[2] = {n - mcamd::kGzipMinRow, mcamd::kGzipMinRow, (1ull << 31) + 5, 0};
        if (!mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;
        mc_gzip_stream keep = rows[2];
        rows[2].in_off = ~0ull; if (mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;
        rows[2] = keep; rows[2].in_len = n + 1; rows[2].in_off = 0; if (mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;
        rows[2] = keep; rows[2].in_len = 17; if (mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;
        rows[2] = keep; rows[2].out_cap = (1ull << 31) + 1; if (mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;
        rows[2] = keep; rows[2].out_off = ~0ull; rows[2].out_cap = 2; if (mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;
        rows[2] = keep; rows[2].out_off = (1ull << 31) + 4; rows[2].out_cap = 1; if (mcamd::gzip_rows_ok(rows, 3, n)) bad = 1;     // overlaps row 1
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
        // every prefix of a small file; of a large one every prefix of the front, which holds the header, and of the end
        for (size_t n = 0; n < bytes.size(); n += (bytes.size() > 4096 && n > 700 && n + 64 < bytes.size()) ? 997 : 1) bad |= check(bytes.data(), n, false, argv[a]);
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
    if (bad) { std::fprintf(stderr, "gzip_rules_check: an inconsistency\n"); return 1; }
    return 0;
}
