// examples/matches_example.cpp -- the mapping lines with the -allhits column (show_matches, printing.cpp:315-365) on metacache_amd.hpp.
//   g++ -std=c++14 -Iinclude examples/matches_example.cpp -Lmetacache_amd/lib -lmetacache_amd -o matches_example
//   ./matches_example <database> <file with one sequence per line> [windows: 1 (default) = name/window:count, 0 = name:count]
// Every batch's location lists are run-length encoded on the device (query_host_data::format_matches, from the table of
// database::set_matches_text: a target prints as its name) and put into the lines as one more column
// (query_host_data::format_mappings' extra argument).  Query i is called "q<i>"; a taxon prints as "<rank number>:<name>".
#include "metacache_amd.hpp"

#include <fstream>
#include <iostream>
#include <string>
#include <vector>

struct sequence_query { std::string header, seq1, seq2; };                       // database_query.hpp:45-72
struct classification_options { int lowestRank = 0; std::size_t insertSizeMax = 0, maxNumCandidatesPerQuery = 2; };

int main(int argc, char** argv)
{
    if (argc < 3) { std::cerr << "usage: matches_example <database> <sequences.txt> [windows]\n"; return 2; }
    try {
        classification_options opt;
        mc_classify_options vote;
        mc_classify_options_default(&vote);
        const int matchFlags = argc > 3 && std::stoi(argv[3]) == 0 ? 0 : MC_MATCHES_WINDOWS;
        mc_config cfg;
        mc_config_default(&cfg);
        cfg.kmerlen = cfg.sketchlen = cfg.winlen = cfg.winstride = 0;
        cfg.copy_allhits = 1;                                                    // the batches keep their location lists
        mc_amd::database db;
        db.read(argv[1], -1, &cfg);
        {
            std::uint64_t numTaxa = 0, numTargets = 0;
            const std::uint32_t* lin = nullptr;
            mc_db_num_taxa(db.handle(), &numTaxa);
            mc_db_lineages(db.handle(), &lin, &numTargets);
            std::vector<std::string> result(1, "--"), names(1, ""), target, candidate;
            for (std::uint64_t x = 0; x < numTaxa; ++x) {
                std::int64_t id, parent; std::uint32_t rank; const char* name;
                mc_db_taxon(db.handle(), x, &id, &parent, &rank, &name);
                result.push_back(std::to_string(rank) + ":" + name);
                names.push_back(name);
            }
            for (std::uint64_t t = 0; t < numTargets; ++t) { target.push_back(result[lin[t * MC_NUM_RANKS]]); candidate.push_back(names[lin[t * MC_NUM_RANKS]]); }
            db.set_mapping_text(MC_TEXT_RESULT, result);
            db.set_mapping_text(MC_TEXT_TARGET_RESULT, target);
            db.set_mapping_text(MC_TEXT_CANDIDATE, candidate);
            db.set_matches_text(candidate);
        }
        mc_format_options fmt{};
        fmt.column[0] = '\t'; fmt.column_len = 1;
        mc_amd::query_batch batch(db, 1);
        std::vector<sequence_query> all;
        { std::ifstream is(argv[2]); std::string line; while (std::getline(is, line)) all.push_back({"q" + std::to_string(all.size()), line, ""}); }

        std::size_t done = 0;
        auto flush = [&](std::size_t upto) {
            db.query_gpu_async(batch, 0, mc_amd::taxon_rank(opt.lowestRank));
            auto& host = batch.host_data(0);
            host.wait_for_results();
            host.classify(vote);
            std::string names;
            std::vector<std::uint64_t> nameOff(1, 0);
            for (std::size_t i = done; i < upto; ++i) { names += all[i].header; nameOff.push_back(names.size()); }
            mc_amd::span<const std::uint64_t> off;
            off.first = nameOff.data(); off.last = nameOff.data() + nameOff.size();
            const auto pieces = host.format_matches(matchFlags);
            const auto lines = host.format_mappings(fmt, MC_FORMAT_QUERY_IDS | MC_FORMAT_TOPHITS, names.data(), off, done + 1, mc_amd::span<const std::uint32_t>(), &pieces);
            std::cout << lines.text;
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
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;                  // main.cpp:65-68
        return 1;
    }
    return 0;
}
