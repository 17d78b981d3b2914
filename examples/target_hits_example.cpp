// examples/target_hits_example.cpp -- the per-target hit lists of -hits-per-ref (matches_per_target.hpp:104-136) on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/target_hits_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o target_hits_example
//   ./target_hits_example <database> <file with one sequence per line> [hitmin]
// every batch's qualifying candidates go to the context's log (query_host_data::record_target_hits); database::hits_per_target sorts
// it on the device.  Prints per target with records:  <target> TAB <records> TAB <query>/<first window>+<more windows>:<hits>,...
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

struct sequence_query { std::string header, seq1, seq2; };                       // database_query.hpp:45-72
struct classification_options { int lowestRank = 0; std::size_t insertSizeMax = 0, maxNumCandidatesPerQuery = 2; };

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: target_hits_example <database> <sequences.txt> [hitmin]\n"; return 2; }
    try {
        classification_options opt;
        const std::uint32_t hitsMin = argc > 3 ? std::uint32_t(std::stoul(argv[3])) : 0u;
        mc_amd::database db;
        db.read(argv[1]);
        mc_amd::query_batch batch(db, 1);
        std::vector<sequence_query> all;
        { std::ifstream is(argv[2]); std::string line; while (std::getline(is, line)) all.push_back({"q", line, ""}); }

        std::size_t done = 0;
        auto flush = [&](std::size_t upto) {
            db.query_gpu_async(batch, 0, mc_amd::taxon_rank(opt.lowestRank));
            auto& host = batch.host_data(0);
            host.wait_for_results();
            host.record_target_hits(hitsMin, opt.lowestRank, done);                  // query ids = the reads' places in the file
            host.clear();
            done = upto;
        };
        for (std::size_t i = 0; i < all.size(); ++i) {
            auto rules = mc_amd::make_candidate_generation_rules(all[i], opt, db.target_sketching().winstride);
            if (!batch.add_paired_read(0, all[i].seq1, all[i].seq2, rules)) {
                flush(i);
                if (!batch.add_paired_read(0, all[i].seq1, all[i].seq2, rules))
                    std::cerr << "query batch is too small for a single read!\n";     // database_query.hpp:101-105
            }
        }
        flush(all.size());

        const mc_amd::database::target_hit_lists lists = db.hits_per_target();
        for (std::size_t t = 0; t + 1 < lists.offsets.size(); ++t) {
            if (lists.offsets[t] == lists.offsets[t + 1]) continue;
            std::cout << t << '\t' << (lists.offsets[t + 1] - lists.offsets[t]) << '\t';
            for (std::uint64_t i = lists.offsets[t]; i < lists.offsets[t + 1]; ++i) {
                const mc_target_hit& h = lists.records[i];
                std::cout << (i > lists.offsets[t] ? "," : "") << h.query << '/' << h.beg << '+' << (h.end - h.beg) << ':' << h.hits;
            }
            std::cout << '\n';
        }
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;                  // main.cpp:65-68
        return 1;
    }
    return 0;
}
