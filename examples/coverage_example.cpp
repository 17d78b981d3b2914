// examples/coverage_example.cpp -- the two passes of -cov-percentile (classification.cpp:747-838) on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/coverage_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o coverage_example
//   ./coverage_example <database> <file with one sequence per line> <percentile, 0 .. 1> [hitmin]
// first pass: every batch's candidates mark the windows they cover (query_host_data::cover); database::keep_by_coverage drops the
// targets at the low end; second pass: the same batches again, classified from the candidates that are left (classify_kept).
// prints  "kept <targets>"  and then per query:  <index> TAB <taxon index + 1, 0 = unclassified> TAB <rank>
#include "metacache_amd.hpp"

#include <fstream>
#include <functional>
#include <iostream>
#include <string>
#include <vector>

struct sequence_query { std::string header, seq1, seq2; };                       // database_query.hpp:45-72
struct classification_options { int lowestRank = 0; std::size_t insertSizeMax = 0, maxNumCandidatesPerQuery = 2; };

int main(int argc, char** argv)
{
    if (argc < 4) { std::cerr << "usage: coverage_example <database> <sequences.txt> <percentile> [hitmin]\n"; return 2; }
    try {
        classification_options opt;
        mc_classify_options vote;
        mc_classify_options_default(&vote);
        const float percentile = std::stof(argv[3]);
        if (argc > 4) vote.hits_min = std::uint32_t(std::stoul(argv[4]));
        mc_amd::database db;
        db.read(argv[1]);
        mc_amd::query_batch batch(db, 1);
        std::vector<sequence_query> all;
        { std::ifstream is(argv[2]); std::string line; while (std::getline(is, line)) all.push_back({"q", line, ""}); }

        // both passes walk the reads in the same batches; `each` sees a batch whose results have arrived
        auto pass = [&](const std::function<void(mc_amd::query_batch::query_host_data&, std::size_t)>& each) {
            std::size_t done = 0;
            auto flush = [&](std::size_t upto) {
                db.query_gpu_async(batch, 0, mc_amd::taxon_rank(opt.lowestRank));
                auto& host = batch.host_data(0);
                host.wait_for_results();
                each(host, done);
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
        };
        pass([&](mc_amd::query_batch::query_host_data& host, std::size_t) { host.cover(vote.hits_min, vote.lowest_rank); });
        std::cout << "kept " << db.keep_by_coverage(percentile) << '\n';
        pass([&](mc_amd::query_batch::query_host_data& host, std::size_t first) {
            std::size_t s = 0;
            for (const mc_assignment& a : host.classify_kept(vote)) std::cout << (first + s++) << '\t' << a.taxon << '\t' << (a.info & 0xFFu) << '\n';
        });
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;                  // main.cpp:65-68
        return 1;
    }
    return 0;
}
