// examples/evaluate_example.cpp -- -precision / -taxon-coverage (classification.cpp:237-295, printing.cpp:537-592) on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/evaluate_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o evaluate_example
//   ./evaluate_example <database> <file with one sequence per line> <file with one true taxon per line> [hitmin] [coverage: 0 / 1]
// a true taxon is a taxon index + 1 as in the lineage table (0 = unknown).  Every batch is classified (query_host_data::classify) and
// judged against the truth (query_host_data::evaluate); database::evaluation reads what the batches counted.
// prints per query:  <index> TAB <taxon index + 1> TAB <rank> TAB <known rank> TAB <correct rank> TAB <counted wrong>
// and then per rank: "rank" <r> <assigned> <known> <correct> <wrong> <precision> <sensitivity> <false positives>
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

struct sequence_query { std::string header, seq1, seq2; };                       // database_query.hpp:45-72
struct classification_options { int lowestRank = 0; std::size_t insertSizeMax = 0, maxNumCandidatesPerQuery = 2; };

int main(int argc, char** argv)
{
    if (argc < 4) { std::cerr << "usage: evaluate_example <database> <sequences.txt> <truth.txt> [hitmin] [coverage]\n"; return 2; }
    try {
        classification_options opt;
        mc_classify_options vote;
        mc_classify_options_default(&vote);
        if (argc > 4) vote.hits_min = std::uint32_t(std::stoul(argv[4]));
        const bool coverage = argc > 5 && std::stoi(argv[5]) != 0;
        mc_amd::database db;
        db.read(argv[1]);
        mc_amd::query_batch batch(db, 1);
        std::vector<sequence_query> all;
        std::vector<std::uint32_t> truth;
        { std::ifstream is(argv[2]); std::string line; while (std::getline(is, line)) all.push_back({"q", line, ""}); }
        { std::ifstream is(argv[3]); std::string line; while (std::getline(is, line)) truth.push_back(std::uint32_t(std::stoul(line))); }
        if (truth.size() != all.size()) throw std::runtime_error("one truth per sequence");

        std::size_t done = 0;
        auto flush = [&](std::size_t upto) {
            db.query_gpu_async(batch, 0, mc_amd::taxon_rank(opt.lowestRank));
            auto& host = batch.host_data(0);
            host.wait_for_results();
            const auto assigned = host.classify(vote);
            mc_amd::span<const std::uint32_t> t;
            t.first = truth.data() + done; t.last = truth.data() + upto;
            const auto verdicts = host.evaluate(t, coverage);
            for (std::size_t s = 0; s < assigned.size(); ++s)
                std::cout << (done + s) << '\t' << assigned[s].taxon << '\t' << (assigned[s].info & 0xFFu) << '\t' << int(verdicts[s].known) << '\t'
                          << int(verdicts[s].correct) << '\t' << int(verdicts[s].flags & 1) << '\n';
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
        const mc_amd::classification_statistics stats = db.evaluation();
        for (int r = 0; r < MC_NUM_RANKS; ++r) {
            const auto rk = mc_amd::taxon_rank(r);
            std::cout << "rank " << r << ' ' << stats.assigned(rk) << ' ' << stats.known(rk) << ' ' << stats.correct(rk) << ' ' << stats.wrong(rk) << ' '
                      << 100 * stats.precision(rk) << ' ' << 100 * stats.sensitivity(rk) << ' ' << stats.coverage(rk).false_pos() << '\n';
        }
        std::cout << "total " << stats.total() << " unknown " << stats.unknown() << '\n';
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;                  // main.cpp:65-68
        return 1;
    }
    return 0;
}
