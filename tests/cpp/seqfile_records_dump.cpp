// prints what SeqFile's eager index delivers for every file: a line "file <records> fast|exact" (fast: byte_range covers all records, the
// file went through the fast scan), then per record the header and the sequence as hexadecimal digits, separated by a blank
#include "mcq_common.h"
using namespace mcq;
static void hex(const View& v) { for (size_t k = 0; k < v.n; ++k) printf("%02x", (unsigned char)v.p[k]); }
int main(int argc, char** argv) {
    for (int a = 1; a < argc; ++a) {
        SeqFile f(argv[a]); f.index(4);
        const char* base = nullptr; size_t b = 0, e = 0;
        const bool fast = f.records() > 0 && f.byte_range(0, f.records(), base, b, e);
        printf("file %zu %s %zu %zu\n", f.records(), fast ? "fast" : "exact", b, e);
        std::string scratch; View h, s;
        for (size_t i = 0; i < f.records(); ++i) { f.record(i, h, s, scratch); hex(h); printf(" "); hex(s); printf("\n"); }
    }
    return 0;
}
