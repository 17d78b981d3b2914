// tools/gzread_loop.cpp -> a small shared library for tools/inflate_bench.py: the loop `mcq` inflates a compressed query file with
// (SeqFile, csrc/mcq_common.h) -- gzread on one thread, through a 1 MiB zlib buffer, into a vector that starts at four times the file's
// size and grows by doubling -- timed on its own.  Returns the seconds; *out_bytes = the inflated size, 0 on failure.
#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <sys/stat.h>
#include <vector>

extern "C" double gzread_loop(const char* path, uint64_t* out_bytes)
{
    const auto t0 = std::chrono::steady_clock::now();
    *out_bytes = 0;
    struct stat st;
    if (stat(path, &st) != 0) return 0.0;
    gzFile g = gzopen(path, "rb");
    if (!g) return 0.0;
    gzbuffer(g, 1u << 20);
    std::vector<char> own(std::max<size_t>((size_t)st.st_size * 4, 1u << 20));
    size_t size = 0;
    for (;;) {
        if (size == own.size()) own.resize(own.size() * 2);
        const int got = gzread(g, own.data() + size, (unsigned)std::min<size_t>(own.size() - size, 1u << 30));
        if (got < 0) { gzclose(g); return 0.0; }
        if (got == 0) break;
        size += (size_t)got;
    }
    gzclose(g);
    *out_bytes = size;
    return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
