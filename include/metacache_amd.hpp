// metacache_amd.hpp -- header-only C++14 mirror of the reference's query-side interface on top of the C ABI
// (metacache_amd.h).  Same names and argument meaning as muellan/metacache so that the caller code of
// database_query.hpp:87-124 (query_gpu) carries over almost verbatim:
//
//   mc_amd::database db;  db.read("refseq");                                   // database::read        database.cpp:183-242
//   mc_amd::query_batch batch(db, numWorkers);                                  // query_batch ctor      database_query.hpp:192-202
//   auto rules = mc_amd::make_candidate_generation_rules(q, opt, db.target_sketching().winstride);
//   batch.add_paired_read(hostId, q.seq1, q.seq2, rules);                       // query_batch.cuh:383-391
//   db.query_gpu_async(batch, hostId, lowestRank);                              // database.hpp:386-397
//   batch.host_data(hostId).wait_for_results();                                 // query_batch.cu:147-152
//   batch.host_data(hostId).allhits(i) / top_candidates(i) / clear()            // query_batch.cuh:212-259
//
// Errors: the reference throws std::runtime_error (caught in main.cpp:65-77); so does this wrapper.
#ifndef METACACHE_AMD_HPP_
#define METACACHE_AMD_HPP_

#include "metacache_amd.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

namespace mc_amd {

using target_id = std::uint32_t;
using window_id = std::uint32_t;

enum class taxon_rank : int {                       // taxonomy.hpp:68-91
    Sequence = 0, Form, Variety, subSpecies, Species, subGenus, Genus, subTribe, Tribe, subFamily, Family, subOrder, Order,
    subClass, Class, subPhylum, Phylum, subKingdom, Kingdom, Domain, root, none
};

struct location { window_id win; target_id tgt; };                              // database.hpp:136-166 (widened)
struct window_range { window_id beg = 0, end = 0; };                             // candidate_structs.hpp:42-71
struct match_candidate {                                                          // candidate_structs.hpp:80-104 (tax resolved by the caller)
    target_id tgt; std::uint32_t hits; window_range pos;
};
struct candidate_generation_rules {                                               // candidate_structs.hpp:113-125
    window_id maxWindowsInRange = 3;
    std::size_t maxCandidates = 2;
    taxon_rank mergeBelow = taxon_rank::Sequence;
};
struct sketching_opt { std::uint32_t kmerlen = 16, sketchlen = 16, winlen = 127, winstride = 112; };

template <class T>
struct span {                                                                     // span.hpp
    const T* first = nullptr; const T* last = nullptr;
    const T* begin() const noexcept { return first; }
    const T* end() const noexcept { return last; }
    std::size_t size() const noexcept { return std::size_t(last - first); }
    const T& operator[](std::size_t i) const noexcept { return first[i]; }
};

// candidate_structs.hpp:134-151
template <class Query, class ClassificationOptions>
candidate_generation_rules make_candidate_generation_rules(const Query& query, const ClassificationOptions& opt, std::uint32_t targetWindowStride)
{
    candidate_generation_rules rules;
    rules.maxWindowsInRange = window_id(2 + (std::max<std::size_t>(query.seq1.size() + query.seq2.size(), opt.insertSizeMax) / targetWindowStride));
    rules.mergeBelow = taxon_rank(int(opt.lowestRank));
    rules.maxCandidates = opt.maxNumCandidatesPerQuery;
    return rules;
}

// classification_statistics (classification_statistics.hpp:135-227) over the per-rank bins of mc_evaluate_tally: the reference's accessor
// names and arithmetic.  assigned / known / correct (r) are sums from sequence up to r, wrong(r) from r up to root.
class classification_statistics {
public:
    using rank = taxon_rank;
    using count_t = std::uint64_t;
    struct confusion_statistics {                                                 // stat_confusion.hpp: one rank's four counters
        count_t tp = 0, fp = 0, tn = 0, fn = 0;
        count_t true_pos() const noexcept { return tp; }
        count_t false_pos() const noexcept { return fp; }
        count_t true_neg() const noexcept { return tn; }
        count_t false_neg() const noexcept { return fn; }
        count_t total() const noexcept { return tp + fp + tn + fn; }
    };
    classification_statistics() : e_{} {}
    explicit classification_statistics(const mc_evaluation& e) : e_(e) {}
    const mc_evaluation& bins() const noexcept { return e_; }

    count_t assigned() const noexcept { return upto(e_.assigned, rank::root); }
    count_t assigned(rank r) const noexcept { return upto(e_.assigned, r); }
    count_t unassigned() const noexcept { return e_.assigned[MC_NUM_RANKS]; }
    count_t total() const noexcept { return assigned() + unassigned(); }
    count_t known() const noexcept { return upto(e_.known, rank::root); }
    count_t known(rank r) const noexcept { return upto(e_.known, r); }
    count_t unknown() const noexcept { return e_.known[MC_NUM_RANKS]; }
    count_t correct() const noexcept { return upto(e_.correct, rank::root); }
    count_t correct(rank r) const noexcept { return upto(e_.correct, r); }
    count_t wrong() const noexcept { return wrong(rank::Sequence); }
    count_t wrong(rank rr) const noexcept { count_t s = 0; for (int r = int(rr); r < MC_NUM_RANKS; ++r) s += e_.wrong[r]; return s; }
    confusion_statistics coverage(rank r) const noexcept
    {
        const std::uint64_t* c = e_.coverage[int(r)];
        confusion_statistics s; s.tp = c[0]; s.fp = c[1]; s.tn = c[2]; s.fn = c[3];
        return s;
    }

    double known_rate(rank r) const noexcept { return total() > 0 ? known(r) / double(total()) : 0; }
    double known_rate() const noexcept { return total() > 0 ? known() / double(total()) : 0; }
    double unknown_rate() const noexcept { return total() > 0 ? unknown() / double(total()) : 0; }
    double classification_rate(rank r) const noexcept { return total() > 0 ? assigned(r) / double(total()) : 0; }
    double unclassified_rate() const noexcept { return total() > 0 ? unassigned() / double(total()) : 0; }
    double sensitivity(rank r) const noexcept { return known(r) > 0 ? correct(r) / double(known(r)) : 0; }
    double precision(rank r) const noexcept
    {
        const double tot = double(correct(r)) + double(wrong(r));                 // (in general neither assigned(r) nor known(r))
        return tot > 0 ? correct(r) / tot : 0;
    }

private:
    static count_t upto(const std::uint64_t* a, rank rr) noexcept { count_t s = 0; for (int r = 0; r <= int(rr) && r < MC_NUM_RANKS; ++r) s += a[r]; return s; }
    mc_evaluation e_;
};

// The statistics line of `info <db> statistics` (print_content_properties, printing.cpp:662-696) from the histogram of list sizes that
// database::table_histogram returns.  features, locations and the power sums are exact integers; the moments follow the reference's
// arithmetic on doubles made from them (stat_moments.hpp:685-707, :836-854); buckets is what the reference's hash table of
// features + dead keys reserves at the database's default load factor, in single precision (hash_multimap.hpp:552-554).  Several
// parts: add() each part's histogram, and sum the parts' buckets.  Above about 5 * 10^8 features the reference's own running double
// sums are no longer exact: its printed six digits are what this matches, not its last bit.
struct table_statistics {
    std::uint64_t features = 0, locations = 0, sum2 = 0, sum3 = 0, max = 0, dead = 0;
    table_statistics() = default;
    explicit table_statistics(const std::uint64_t hist[256], std::uint64_t deadFeatures = 0) { add(hist, deadFeatures); }
    void add(const std::uint64_t hist[256], std::uint64_t deadFeatures = 0)
    {
        for (std::uint64_t s = 1; s < 256; ++s) {
            if (!hist[s]) continue;
            features += hist[s]; locations += s * hist[s]; sum2 += s * s * hist[s]; sum3 += s * s * s * hist[s];
            max = std::max(max, s);
        }
        dead += deadFeatures;
    }
    double mean() const noexcept { return features ? double(locations) / double(features) : 0.0; }
    double variance() const noexcept
    {
        if (features < 2) return 0.0;
        const double n = double(features), s1 = double(locations);
        return (double(sum2) - s1 * s1 / n) / (n - 1.0);
    }
    double stddev() const noexcept { return std::sqrt(variance()); }
    double skewness() const noexcept
    {
        const double cm2 = variance();
        if (features < 2 || !(cm2 > 0.0)) return 0.0;
        const double n = double(features), n2 = n * n, s1 = double(locations), s2 = double(sum2);
        const double cm3 = (n2 * double(sum3) - 3.0 * n * (s1 * s2) + 2.0 * (s1 * s1 * s1)) / (n * n2);
        return cm3 / std::pow(cm2, 1.5);
    }
    std::uint64_t buckets(float loadFactor = 0.8f) const noexcept { return std::uint64_t(1.0f + float(features + dead) / loadFactor); }
};

// the members of a BGZF range (mc_bgzf_index; host code: no device, no zlib).  verdict MC_BGZF_OK: blocks[i] is member i and outBytes the
// sum of their ISIZE.  MC_BGZF_FOREIGN: the range is something else from byte `offence` on -- the caller reads it through zlib.
struct bgzf_members { int verdict = MC_BGZF_FOREIGN; std::uint64_t offence = 0, outBytes = 0; std::vector<mc_bgzf_block> blocks; };
inline bgzf_members bgzf_index(const void* bytes, std::size_t nbytes)
{
    bgzf_members m;
    std::uint64_t info[4] = {0, 0, 0, 0};
    if (mc_bgzf_index(static_cast<const std::uint8_t*>(bytes), nbytes, nullptr, 0, info) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
    m.blocks.resize(std::size_t(info[0]));
    if (mc_bgzf_index(static_cast<const std::uint8_t*>(bytes), nbytes, m.blocks.data(), m.blocks.size(), info) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
    m.verdict = int(info[2]); m.offence = info[3]; m.outBytes = info[1];
    return m;
}

// what a gzip file's first header and last four bytes say (mc_gzip_hint; host code: no device, no zlib).  verdict MC_GZIP_OK: the device
// takes the first member's header, whose deflate stream begins at `payload`; isize is the trailing ISIZE -- the plain size of a file of
// one member below 4 GiB, too small for a chain of members.  MC_GZIP_FOREIGN: offence says why (MC_INFLATE_R_*).
struct gzip_file_hint { int verdict = MC_GZIP_FOREIGN; std::uint64_t payload = 0, isize = 0; int offence = 0; };
inline gzip_file_hint gzip_hint(const void* bytes, std::size_t nbytes)
{
    gzip_file_hint h;
    std::uint64_t info[4] = {0, 0, 0, 0};
    if (mc_gzip_hint(static_cast<const std::uint8_t*>(bytes), nbytes, info) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
    h.verdict = int(info[0]); h.payload = info[1]; h.isize = info[2]; h.offence = int(info[3]);
    return h;
}

class query_batch;

// the targets of a range that holds many FASTA files back to back, cut on the device (mc_parse_targets on host arrays; the target rule:
// metacache_amd.h).  verdict MC_PARSE_OK: record r's header is bytes[hdr[2r] .. + hdr[2r + 1]), its sequence seq[targets[r].seq_off .. +
// targets[r].len), its file targets[r].file and its number inside that file targets[r].index; records counts ALL records, withSequence
// those with len > 0 (what a build adds).  Another verdict: the arrays are empty, offence says where the range broke the rule and file in
// which file (a file table that breaks its own rule: offence = the range's length, file = the first bad row).
struct parsed_targets {
    int verdict = MC_PARSE_IRREGULAR; std::uint64_t offence = 0, file = 0; std::uint32_t records = 0, withSequence = 0, longest = 0;
    std::vector<std::uint32_t> hdr; std::vector<mc_parse_target> targets; std::vector<std::uint8_t> seq;
    std::string header(const char* bytes, std::size_t r) const { return std::string(bytes + hdr[2 * r], hdr[2 * r + 1]); }
};

class database {
public:
    database() = default;
    database(const database&) = delete;
    database& operator=(const database&) = delete;
    ~database() { if (ctx_) mc_destroy(ctx_); }

    // database::read(filename, singlePartId, replication, scope, info); cfg carries the query-time options
    void read(const std::string& filename, int singlePartId = -1, const mc_config* cfg = nullptr)
    {
        mc_config c;
        if (cfg) c = *cfg; else { mc_config_default(&c); c.kmerlen = c.sketchlen = c.winlen = c.winstride = 0; }
        c.single_part = singlePartId;
        if (mc_open_database(filename.c_str(), &c, &ctx_) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
        std::uint64_t info[8];
        mc_db_info(ctx_, info);
        sk_.kmerlen = std::uint32_t(info[0]); sk_.sketchlen = std::uint32_t(info[1]);
        sk_.winlen = std::uint32_t(info[2]); sk_.winstride = std::uint32_t(info[3]);
        targets_ = info[5]; parts_ = unsigned(info[6]);
        maxCand_ = c.max_candidates; slots_ = c.num_slots; copyAllhits_ = c.copy_allhits != 0;
    }
    // a context on the device without a table: what the parse calls (parse_records, parse_cut, parse_targets, ...) need
    void create(int device = 0)
    {
        mc_config c;
        mc_config_default(&c);
        c.device = device;
        if (mc_create(&c, &ctx_) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
        maxCand_ = c.max_candidates; slots_ = c.num_slots; copyAllhits_ = c.copy_allhits != 0;
    }
    const sketching_opt& target_sketching() const noexcept { return sk_; }
    std::uint64_t target_count() const noexcept { return targets_; }
    unsigned part_count() const noexcept { return parts_; }
    mc_ctx* handle() const noexcept { return ctx_; }

    // -cov-percentile between its two passes (filter_targets_by_coverage, classification.cpp:591-634): the covered-window counts of what
    // the batches' cover() calls have marked (mc_coverage_counts, which is reset), the targets kept at `percentile` (a factor in
    // [0, 1]; mc_coverage_keep visiting the targets by ascending id) and the mask for classify_kept (mc_coverage_set_keep).
    // Returns the number of targets kept.
    std::size_t keep_by_coverage(float percentile) const
    {
        std::uint64_t n = 0;
        if (mc_coverage_counts(ctx_, nullptr, nullptr, 0, &n, nullptr, 0) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        std::vector<std::uint32_t> covered(n), windows(n);
        std::vector<std::uint8_t> keep(n);
        if (mc_coverage_counts(ctx_, covered.data(), windows.data(), n, nullptr, nullptr, 1) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        if (mc_coverage_keep(covered.data(), windows.data(), n, nullptr, 0, percentile, keep.data()) != MC_OK)
            throw std::runtime_error("mc_coverage_keep: percentile outside [0, 1]");
        if (mc_coverage_set_keep(ctx_, keep.data(), n) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        return std::size_t(std::count(keep.begin(), keep.end(), std::uint8_t(1)));
    }

    // -hits-per-ref after the last batch (matches_per_target::sort, matches_per_target.hpp:128-136): what the batches'
    // record_target_hits() calls have logged, sorted on the device by (tgt, beg, end, query, hits) -- records[offsets[t] ..
    // offsets[t + 1]) is target t's list (mc_target_hits_collect, which is reset: the call CONSUMES the log, hence not const)
    struct target_hit_lists { std::vector<std::uint64_t> offsets; std::vector<mc_target_hit> records; };
    target_hit_lists hits_per_target()
    {
        std::uint64_t nt = 0, nr = 0;
        if (mc_target_hits_collect(ctx_, nullptr, 0, &nt, nullptr, 0, &nr, nullptr, 0) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        target_hit_lists l;
        l.offsets.resize(nt + 1); l.records.resize(nr);
        if (mc_target_hits_collect(ctx_, l.offsets.data(), nt, nullptr, l.records.data(), nr, nullptr, nullptr, 1) != MC_OK)
            throw std::runtime_error(mc_last_error(ctx_));
        return l;
    }

    // one of the three string tables of the mapping lines (mc_format_set_text): MC_TEXT_RESULT (per taxon index + 1, entry 0 = the
    // unclassified text), MC_TEXT_TARGET_RESULT and MC_TEXT_CANDIDATE (per target); no format_mappings() may be in flight
    void set_mapping_text(int which, const std::vector<std::string>& strings) const
    {
        std::string bytes;
        std::vector<std::uint64_t> off(1, 0);
        for (const std::string& t : strings) { bytes += t; off.push_back(bytes.size()); }
        if (mc_format_set_text(ctx_, which, bytes.data(), off.data(), strings.size()) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
    }

    // the table of the all-hits column (mc_format_matches_set_text), per target: the text in front of "/window:length," (MC_MATCHES_WINDOWS)
    // or ":length,"; no format_matches() may be in flight
    void set_matches_text(const std::vector<std::string>& strings) const
    {
        std::string bytes;
        std::vector<std::uint64_t> off(1, 0);
        for (const std::string& t : strings) { bytes += t; off.push_back(bytes.size()); }
        if (mc_format_matches_set_text(ctx_, bytes.data(), off.data(), strings.size()) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
    }

    // the reads of a FASTA / FASTQ byte range, cut on the device (mc_parse_records on host arrays; the record rule: metacache_amd.h).
    // verdict MC_PARSE_OK: record r's header is bytes[hdr[2r] .. + hdr[2r + 1]), query q's reads are seq[qinfo[4q] .. + qinfo[4q + 1])
    // and seq[qinfo[4q + 2] .. + qinfo[4q + 3]), its name is names[nameOff[q] .. nameOff[q + 1]).  Another verdict: the arrays are empty
    // and offence says where the range broke the rule -- the caller cuts that range itself.
    struct parsed_records {
        int verdict = MC_PARSE_IRREGULAR; std::uint64_t offence = 0; std::uint32_t records = 0, queries = 0; bool halfPair = false;
        std::vector<std::uint32_t> hdr, qinfo, maxWin; std::vector<std::uint8_t> seq; std::string names; std::vector<std::uint64_t> nameOff;
    };
    parsed_records parse_records(const char* bytes, std::size_t nbytes, bool pairs = false, std::uint64_t insertSizeMax = 0) const
    {
        parsed_records p;
        std::uint64_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int pass = 0; pass < 2; ++pass) {                                   // (the first call reports what the second needs)
            mc_parse_output o{};
            const std::uint32_t mr = std::uint32_t(status[0]);
            p.hdr.assign(std::size_t(mr) * 2 + 1, 0); p.qinfo.assign(std::size_t(mr) * 4 + 1, 0); p.maxWin.assign(std::size_t(mr) + 1, 0);
            p.seq.assign(std::size_t(status[2]) + 1, 0); p.names.assign(std::size_t(status[3]) + 1, char(0)); p.nameOff.assign(std::size_t(mr) + 1, 0);
            o.hdr = p.hdr.data(); o.qinfo = p.qinfo.data(); o.seq = p.seq.data(); o.seq_capacity = status[2]; o.names = &p.names[0];
            o.names_capacity = status[3]; o.name_off = p.nameOff.data(); o.max_win = p.maxWin.data(); o.status = status; o.max_records = mr;
            if (mc_parse_records(ctx_, bytes, nbytes, MC_PARSE_HOST | (pairs ? MC_PARSE_PAIRS : 0), insertSizeMax, &o, nullptr, 0, nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            if (status[4] != MC_PARSE_OVERFLOW) break;
        }
        p.verdict = int(status[4]); p.offence = status[5];
        const bool ok = status[4] == MC_PARSE_OK;
        p.records = ok ? std::uint32_t(status[0]) : 0; p.queries = ok ? std::uint32_t(status[1]) : 0; p.halfPair = ok && status[7] != 0;
        p.hdr.resize(std::size_t(p.records) * 2); p.qinfo.resize(std::size_t(p.queries) * 4); p.maxWin.resize(p.queries);
        p.seq.resize(ok ? std::size_t(status[2]) : 0); p.names.resize(ok ? std::size_t(status[3]) : 0); p.nameOff.resize(ok ? std::size_t(p.queries) + 1 : 0);
        return p;
    }

    // files back to back in bytes[0, nbytes), file f = bytes[fileOff[f], fileOff[f + 1]) -> their targets (see parsed_targets)
    parsed_targets parse_targets(const char* bytes, std::size_t nbytes, const std::vector<std::uint64_t>& fileOff) const
    {
        parsed_targets p;
        if (fileOff.size() < 2) throw std::invalid_argument("database::parse_targets: a file table has two rows at least");
        std::uint64_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int pass = 0; pass < 2; ++pass) {                                   // (the first call reports what the second needs)
            mc_parse_targets_output o{};
            const std::uint32_t mr = std::uint32_t(status[0]);
            p.hdr.assign(std::size_t(mr) * 2 + 1, 0); p.targets.assign(std::size_t(mr) + 1, mc_parse_target{}); p.seq.assign(std::size_t(status[2]) + 1, 0);
            o.hdr = p.hdr.data(); o.targets = p.targets.data(); o.seq = p.seq.data(); o.seq_capacity = status[2]; o.status = status; o.max_records = mr;
            if (mc_parse_targets(ctx_, bytes, nbytes, fileOff.data(), std::uint32_t(fileOff.size() - 1), MC_PARSE_HOST, &o, nullptr, 0, nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            if (status[4] != MC_PARSE_OVERFLOW) break;
        }
        p.verdict = int(status[4]); p.offence = status[5]; p.file = status[7];
        const bool ok = status[4] == MC_PARSE_OK;
        p.records = ok ? std::uint32_t(status[0]) : 0; p.withSequence = ok ? std::uint32_t(status[1]) : 0; p.longest = ok ? std::uint32_t(status[6]) : 0;
        p.hdr.resize(std::size_t(p.records) * 2); p.targets.resize(p.records); p.seq.resize(ok ? std::size_t(status[2]) : 0);
        return p;
    }

    // the batch borders of a FASTA / FASTQ byte range, found on the device (mc_parse_cut on host arrays; the cut rule: metacache_amd.h).
    // verdict MC_PARSE_OK: batch i is bytes[cuts[i] .. cuts[i + 1]), recordsPerBatch whole records (the last batch: the rest); open: the
    // last record may be cut short and the next range starts at consumed.  Another verdict: cuts is empty and offence says where the
    // range broke the rule.
    struct cut_batches {
        int verdict = MC_PARSE_IRREGULAR; std::uint64_t offence = 0, whole = 0, consumed = 0, seen = 0, longest = 0; bool halfPair = false;
        std::vector<std::uint64_t> cuts;
    };
    cut_batches parse_cut(const char* bytes, std::size_t nbytes, std::uint32_t recordsPerBatch, bool pairs = false, bool open = false) const
    {
        cut_batches c;
        std::uint64_t status[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int pass = 0; pass < 2; ++pass) {                                   // (the first call reports what the second needs)
            c.cuts.assign(std::size_t(status[1]) + 1, 0);
            if (mc_parse_cut(ctx_, bytes, nbytes, recordsPerBatch, MC_PARSE_HOST | (pairs ? MC_PARSE_PAIRS : 0) | (open ? MC_CUT_OPEN : 0), c.cuts.data(),
                             c.cuts.size(), status, nullptr, 0, nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            if (status[4] != MC_PARSE_OVERFLOW) break;
        }
        c.verdict = int(status[4]); c.offence = status[5]; c.whole = status[0]; c.consumed = status[2]; c.seen = status[3]; c.longest = status[6];
        c.halfPair = status[7] != 0;
        if (status[4] != MC_PARSE_OK) c.cuts.clear();
        return c;
    }

    // the members of a BGZF range inflated on the device (mc_inflate_blocks on host arrays; the block rule: metacache_amd.h).  verdict
    // MC_INFLATE_OK: bytes is what zlib gives for the range.  Another verdict: bytes is empty, block is the lowest member the device
    // refused and reason says why (MC_INFLATE_R_*) -- the caller reads the range through zlib.
    struct inflated { int verdict = MC_INFLATE_CORRUPT; std::uint64_t block = 0; int reason = 0; std::string bytes; };
    inflated inflate(const void* bytes, std::size_t nbytes, const bgzf_members& members) const
    {
        inflated r;
        std::uint64_t status[4] = {0, 0, 0, 0};
        r.bytes.assign(std::size_t(members.outBytes) + 1, char(0));
        if (mc_inflate_blocks(ctx_, static_cast<const std::uint8_t*>(bytes), nbytes, members.blocks.data(), members.blocks.size(), MC_INFLATE_HOST,
                              reinterpret_cast<std::uint8_t*>(&r.bytes[0]), members.outBytes, status, nullptr) != MC_OK)
            throw std::runtime_error(mc_last_error(ctx_));
        r.verdict = int(status[0]); r.block = status[1]; r.reason = int(status[2]);
        r.bytes.resize(r.verdict == MC_INFLATE_OK ? std::size_t(members.outBytes) : 0);
        return r;
    }

    // whole gzip files inflated on the device, a wave per file (mc_inflate_streams on host arrays; the stream rule: metacache_amd.h).
    // files[i] is one file's bytes, room[i] the bytes its output may take (gzip_hint's isize for a file of one member).  Every file has
    // its own verdict: results[i].reason == 0 and plain[i] what zlib gives for it, or the reason (MC_INFLATE_R_*) and an empty plain[i] --
    // the caller reads that file through zlib.  verdict, row and reason are the call's: those of the lowest refused file.
    struct inflated_files { int verdict = MC_INFLATE_CORRUPT; std::uint64_t row = 0, accepted = 0; int reason = 0; std::vector<mc_gzip_result> results; std::vector<std::string> plain; };
    inflated_files inflate_streams(const std::vector<std::string>& files, const std::vector<std::uint64_t>& room) const
    {
        if (files.size() != room.size()) throw std::invalid_argument("inflate_streams: one room per file");
        inflated_files r;
        std::vector<mc_gzip_stream> rows(files.size());
        std::string in;
        std::uint64_t outAt = 0;
        for (std::size_t i = 0; i < files.size(); ++i) {
            in.resize((in.size() + 15) / 16 * 16, char(0));
            rows[i] = mc_gzip_stream{in.size(), files[i].size(), outAt, room[i]};
            in += files[i];
            outAt += room[i];
        }
        std::string out(std::size_t(outAt) + 1, char(0));
        std::uint64_t status[4] = {0, 0, 0, 0};
        r.results.resize(files.size());
        if (mc_inflate_streams(ctx_, reinterpret_cast<const std::uint8_t*>(in.data()), in.size(), rows.data(), rows.size(), MC_INFLATE_HOST,
                               reinterpret_cast<std::uint8_t*>(&out[0]), outAt, r.results.data(), status, nullptr) != MC_OK)
            throw std::runtime_error(mc_last_error(ctx_));
        r.verdict = int(status[0]); r.row = status[1]; r.reason = int(status[2]); r.accepted = status[3];
        r.plain.resize(files.size());
        for (std::size_t i = 0; i < files.size(); ++i)
            if (!r.results[i].reason) r.plain[i].assign(out, std::size_t(rows[i].out_off), std::size_t(r.results[i].produced));
        return r;
    }

    // the pairs of two mate files' byte ranges, cut on the device (mc_parse_mates on host arrays; the mates rule: metacache_amd.h):
    // query q is record q of bytes1 and record q of bytes2.  As parse_records(pairs = true), except that hdr row 2q is a place in bytes1
    // and row 2q + 1 a place in bytes2; records1 / records2 are set with MC_PARSE_OK and MC_PARSE_UNEQUAL, offenceRange with MC_PARSE_IRREGULAR.
    struct parsed_mates : parsed_records { std::uint32_t records1 = 0, records2 = 0; int offenceRange = 0; };
    parsed_mates parse_mates(const char* bytes1, std::size_t n1, const char* bytes2, std::size_t n2, std::uint64_t insertSizeMax = 0) const
    {
        parsed_mates p;
        std::uint64_t status[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int pass = 0; pass < 2; ++pass) {                                   // (the first call reports what the second needs)
            mc_parse_output o{};
            const std::uint32_t mr = std::uint32_t(status[0]);
            p.hdr.assign(std::size_t(mr) * 2 + 1, 0); p.qinfo.assign(std::size_t(mr) * 4 + 1, 0); p.maxWin.assign(std::size_t(mr) + 1, 0);
            p.seq.assign(std::size_t(status[2]) + 1, 0); p.names.assign(std::size_t(status[3]) + 1, char(0)); p.nameOff.assign(std::size_t(mr) + 1, 0);
            o.hdr = p.hdr.data(); o.qinfo = p.qinfo.data(); o.seq = p.seq.data(); o.seq_capacity = status[2]; o.names = &p.names[0];
            o.names_capacity = status[3]; o.name_off = p.nameOff.data(); o.max_win = p.maxWin.data(); o.status = status; o.max_records = mr;
            if (mc_parse_mates(ctx_, bytes1, n1, bytes2, n2, MC_PARSE_HOST, insertSizeMax, &o, nullptr, 0, nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            if (status[4] != MC_PARSE_OVERFLOW) break;
        }
        p.verdict = int(status[4]); p.offence = status[5]; p.offenceRange = int(status[7]);
        const bool ok = status[4] == MC_PARSE_OK;
        p.records = ok ? std::uint32_t(status[0]) : 0; p.queries = ok ? std::uint32_t(status[1]) : 0;
        p.records1 = std::uint32_t(status[8]); p.records2 = std::uint32_t(status[9]);
        p.hdr.resize(std::size_t(p.records) * 2); p.qinfo.resize(std::size_t(p.queries) * 4); p.maxWin.resize(p.queries);
        p.seq.resize(ok ? std::size_t(status[2]) : 0); p.names.resize(ok ? std::size_t(status[3]) : 0); p.nameOff.resize(ok ? std::size_t(p.queries) + 1 : 0);
        return p;
    }

    // -precision / -taxon-coverage after the last batch: what the batches' evaluate() calls have counted (mc_evaluate_tally; reset: the
    // counters start from zero again)
    classification_statistics evaluation(bool reset = false) const
    {
        mc_evaluation e;
        if (mc_evaluate_tally(ctx_, &e, reset ? 1 : 0) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        return classification_statistics(e);
    }

    // what the table in HBM holds (mc_table_*; one part per context -- read(name, part) -- and no query in flight meanwhile):
    // the histogram of list sizes with the number of features the load-time rules emptied (table_statistics makes the statistics line),
    struct size_histogram { std::uint64_t hist[256]; std::uint64_t dead; };
    size_histogram table_histogram() const
    {
        size_histogram h{};
        if (mc_table_histogram(ctx_, h.hist, &h.dead) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        return h;
    }
    // every stored feature in ascending order with the length of its location list (print_feature_counts, host_hashmap.hpp:433-445),
    struct feature_sizes { std::vector<std::uint32_t> features, sizes; };
    feature_sizes table_features() const
    {
        std::uint64_t n = 0;
        if (mc_table_features(ctx_, nullptr, nullptr, 0, &n, 0) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        feature_sizes f;
        f.features.resize(n); f.sizes.resize(n);
        if (n && mc_table_features(ctx_, f.features.data(), f.sizes.data(), n, &n, 0) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
        return f;
    }
    // and the location lists of some features, in the order of the database file (print_feature_map, host_hashmap.hpp:413-429): list i
    // = locations[offsets[i] .. offsets[i + 1]); a feature the table does not hold has an empty list
    struct feature_lists { std::vector<std::uint64_t> offsets; std::vector<location> locations; };
    feature_lists table_lookup(span<const std::uint32_t> features) const
    {
        static_assert(sizeof(location) == sizeof(mc_location), "location mirrors mc_location");
        feature_lists l;
        l.offsets.resize(features.size() + 1);
        int rc = mc_table_lookup(ctx_, features.begin(), features.size(), l.offsets.data(), nullptr, 0, 0);
        if (rc != MC_OK && rc != MC_ERR_NOMEM) throw std::runtime_error(mc_last_error(ctx_));   // (MC_ERR_NOMEM: offsets came back complete)
        l.locations.resize(l.offsets[features.size()]);
        if (!l.locations.empty() && mc_table_lookup(ctx_, features.begin(), features.size(), l.offsets.data(),
                                                    reinterpret_cast<mc_location*>(l.locations.data()), l.locations.size(), 0) != MC_OK)
            throw std::runtime_error(mc_last_error(ctx_));
        return l;
    }

    // database::query_gpu_async(queryBatch, hostId, querySketching, lowestRank)  database.hpp:386-397
    void query_gpu_async(query_batch& batch, unsigned hostId, taxon_rank lowestRank) const;

private:
    friend class query_batch;
    mc_ctx* ctx_ = nullptr;
    sketching_opt sk_;
    std::uint64_t targets_ = 0;
    unsigned parts_ = 0, maxCand_ = 2, slots_ = 1;
    bool copyAllhits_ = false;
};

class query_batch {
public:
    class query_host_data {                                                      // query_batch.cuh:60-280
    public:
        std::size_t num_queries() const noexcept { return res_.num_queries; }
        void wait_for_results()                                                  // query_batch.cu:147-152
        {
            if (mc_batch_wait(ctx_, slot_, &res_) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
            const std::size_t n = res_.num_queries, K = res_.max_candidates;
            tops_.resize(n * K);
            for (std::size_t i = 0; i < n * K; ++i) {
                const mc_candidate& c = res_.cands[i];
                tops_[i].tgt = c.tgt; tops_[i].hits = c.hits; tops_[i].pos.beg = c.beg; tops_[i].pos.end = c.end;
            }
        }
        span<location> allhits(std::size_t i) const noexcept                      // query_batch.cuh:212-221
        {
            span<location> s;
            if (res_.hits) {
                s.first = reinterpret_cast<const location*>(res_.hits) + res_.hit_offsets[i];
                s.last = reinterpret_cast<const location*>(res_.hits) + res_.hit_offsets[i + 1];
            }
            return s;
        }
        span<match_candidate> top_candidates(std::size_t i) const noexcept        // query_batch.cuh:223-231; unused entries: hits == 0
        {
            const std::size_t K = res_.max_candidates;
            span<match_candidate> s;
            s.first = tops_.data() + i * K; s.last = s.first + K;
            return s;
        }
        // one taxon per query of this batch from its top candidates (after wait_for_results): the ranked-LCA vote of
        // classification.cpp:146-189 on the device (mc_classify_candidates on the slot's host arrays); tally: the queries are added to
        // the context's per-rank / per-taxon counts (mc_classify_tally).  Valid until the next classify() or clear().
        span<mc_assignment> classify(const mc_classify_options& opt, bool tally = false)
        {
            assigned_.resize(res_.num_queries);
            if (mc_classify_candidates(ctx_, &opt, res_.cands, res_.num_queries, res_.max_candidates,
                                       MC_CLASSIFY_HOST | (tally ? MC_CLASSIFY_TALLY : 0), assigned_.data(), nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            span<mc_assignment> s;
            s.first = assigned_.data(); s.last = s.first + assigned_.size();
            return s;
        }
        // -precision / -taxon-coverage (after classify()): this batch's assignments against what the queries really are -- truth[i] =
        // taxon index + 1 of query i's true taxon, 0 = unknown -- counted into the context's evaluation tallies
        // (evaluate_classification, classification.cpp:272-295; mc_evaluate_assignments on the slot's host arrays; database::evaluation
        // reads them); coverage: also the confusion counters of -taxon-coverage.  The verdicts are valid until the next evaluate() or clear().
        span<mc_verdict> evaluate(span<const std::uint32_t> truth, bool coverage = false)
        {
            if (truth.size() != assigned_.size()) throw std::runtime_error("evaluate: one truth per query of the batch that classify() has judged");
            verdicts_.resize(assigned_.size());
            if (mc_evaluate_assignments(ctx_, assigned_.data(), truth.begin(), std::uint32_t(assigned_.size()),
                                        MC_EVALUATE_HOST | MC_EVALUATE_TALLY | (coverage ? MC_EVALUATE_COVERAGE : 0), verdicts_.data(), nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            span<mc_verdict> s;
            s.first = verdicts_.data(); s.last = s.first + verdicts_.size();
            return s;
        }
        // the batch's mapping lines (after classify()): what show_query_mapping prints per query (classification.cpp:432-523,
        // printing.cpp:283-380), rendered on the device from the slot's host arrays (mc_format_mappings; the string tables:
        // database::set_mapping_text).  names[nameOff[i] .. nameOff[i + 1]) is query i's name; the queries are numbered firstQueryId,
        // firstQueryId + 1, ...; flags: MC_FORMAT_QUERY_IDS, _TRUTH (truth: one taxon index + 1 per query), _TOPHITS, _LOCATIONS,
        // _MAPPED_ONLY.  Line i is text[offsets[i] .. offsets[i + 1]).  Valid until the next format_mappings() or clear().
        struct mapping_lines { const std::string& text; const std::vector<std::uint64_t>& offsets; };
        mapping_lines format_mappings(const mc_format_options& opt, int flags, const char* names, span<const std::uint64_t> nameOff,
                                      std::uint64_t firstQueryId, span<const std::uint32_t> truth = span<const std::uint32_t>(),
                                      const mapping_lines* extra = nullptr)      // extra: one more column behind the truth column, e.g. format_matches()
        {
            const std::uint32_t n = res_.num_queries;
            if (assigned_.size() != n || nameOff.size() != std::size_t(n) + 1 || ((flags & MC_FORMAT_TRUTH) && truth.size() != n))
                throw std::runtime_error("format_mappings: one assignment (classify()), one name and -- with MC_FORMAT_TRUTH -- one truth per query of the batch");
            lineOff_.resize(std::size_t(n) + 1);
            if (lines_.size() < std::size_t(n) * 128 + 16) lines_.resize(std::size_t(n) * 128 + 16);
            auto render = [&]() {
                return mc_format_mappings_with(ctx_, &opt, res_.cands, res_.max_candidates, assigned_.data(), (flags & MC_FORMAT_TRUTH) ? truth.begin() : nullptr,
                                               nullptr, firstQueryId, names, nameOff.begin(), n, flags | MC_FORMAT_HOST, &lines_[0], lines_.size(), lineOff_.data(), nullptr,
                                               extra ? extra->text.data() : nullptr, extra ? extra->offsets.data() : nullptr);
            };
            if (extra && (extra->offsets.size() != std::size_t(n) + 1 || &extra->text == &lines_))
                throw std::runtime_error("format_mappings: the extra column has one piece per query of the batch");
            int rc = render();
            if (rc == MC_ERR_NOMEM) { lines_.resize(lineOff_[n]); rc = render(); }      // (line_off came back complete: now the lines fit)
            if (rc != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
            lines_.resize(lineOff_[n]);
            return mapping_lines{lines_, lineOff_};
        }
        // the batch's all-hits column (after wait_for_results; the database was read with copy_allhits): every query's location list
        // run-length encoded as show_matches prints it (printing.cpp:315-365), rendered on the device from the slot's host arrays
        // (mc_format_matches; the table: database::set_matches_text).  flags: 0 or MC_MATCHES_WINDOWS.  Piece i is
        // text[offsets[i] .. offsets[i + 1]); format_mappings takes the result as its extra column.  Valid until the next format_matches() or clear().
        mapping_lines format_matches(int flags)
        {
            const std::uint32_t n = res_.num_queries;
            if (n && (!res_.hits || !res_.hit_offsets)) throw std::runtime_error("format_matches: the batch has no location lists (mc_config.copy_allhits)");
            static const std::uint64_t none[1] = {0};
            pieceOff_.resize(std::size_t(n) + 1);
            if (pieces_.size() < 4096) pieces_.resize(4096);
            auto render = [&]() {
                return mc_format_matches(ctx_, res_.hits, n ? res_.hit_offsets : none, n, flags | MC_FORMAT_HOST, &pieces_[0], pieces_.size(), pieceOff_.data(), nullptr);
            };
            int rc = render();
            if (rc == MC_ERR_NOMEM) { pieces_.resize(pieceOff_[n]); rc = render(); }   // (piece_off came back complete: now the pieces fit)
            if (rc != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
            pieces_.resize(pieceOff_[n]);
            return mapping_lines{pieces_, pieceOff_};
        }
        // -cov-percentile, first pass (after wait_for_results): the windows that this batch's qualifying candidates cover are marked in
        // the context's bitmap (matches_per_target::insert, matches_per_target.hpp:100-127; mc_coverage_add on the slot's host arrays)
        void cover(std::uint32_t hitsMin, int lowestRank)
        {
            if (mc_coverage_add(ctx_, res_.cands, res_.num_queries, res_.max_candidates, hitsMin, lowestRank, MC_COVERAGE_HOST, nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
        }
        // second pass, after database::keep_by_coverage: classify() from the candidates of the targets that were kept
        // (update_candidates, classification.cpp:660-671; mc_coverage_drop into a buffer of this object, then the vote)
        span<mc_assignment> classify_kept(const mc_classify_options& opt, bool tally = false)
        {
            kept_.resize(std::size_t(res_.num_queries) * res_.max_candidates);
            assigned_.resize(res_.num_queries);
            if (mc_coverage_drop(ctx_, res_.cands, res_.num_queries, res_.max_candidates, MC_COVERAGE_HOST, kept_.data(), nullptr) != MC_OK ||
                mc_classify_candidates(ctx_, &opt, kept_.data(), res_.num_queries, res_.max_candidates,
                                       MC_CLASSIFY_HOST | (tally ? MC_CLASSIFY_TALLY : 0), assigned_.data(), nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
            span<mc_assignment> s;
            s.first = assigned_.data(); s.last = s.first + assigned_.size();
            return s;
        }
        // -hits-per-ref (after wait_for_results): one record per qualifying candidate of this batch goes to the context's log
        // (matches_per_target::insert, matches_per_target.hpp:104-110; mc_target_hits_add on the slot's host arrays); the batch's
        // queries are numbered firstQueryId, firstQueryId + 1, ...
        void record_target_hits(std::uint32_t hitsMin, int lowestRank, std::uint64_t firstQueryId)
        {
            if (mc_target_hits_add(ctx_, res_.cands, nullptr, firstQueryId, res_.num_queries, res_.max_candidates, hitsMin, lowestRank,
                                   MC_TARGET_HITS_HOST, nullptr) != MC_OK)
                throw std::runtime_error(mc_last_error(ctx_));
        }
        // what the device made of a batch filled by add_file_bytes (after wait_for_results; mc_batch_records): the verdict, and with
        // MC_PARSE_OK the records' headers and the queries' lengths as views that are valid until clear()
        mc_batch_record_info records() const
        {
            mc_batch_record_info info{};
            if (mc_batch_records(ctx_, slot_, &info) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
            return info;
        }
        // the headers of a batch filled by add_device_bytes (after wait_for_results; mc_batch_headers): header r is bytes[off[r] ..
        // off[r + 1]), views that are valid until clear(); null views with another verdict than MC_PARSE_OK
        struct header_views { const char* bytes = nullptr; const std::uint64_t* off = nullptr; std::uint64_t records = 0; };
        header_views headers() const
        {
            header_views h;
            if (mc_batch_headers(ctx_, slot_, &h.bytes, &h.off, &h.records) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
            return h;
        }
        void clear() { mc_batch_clear(ctx_, slot_); res_ = mc_results{}; assigned_.clear(); kept_.clear(); verdicts_.clear(); lineOff_.clear(); pieceOff_.clear(); }   // query_batch.cuh:255-259
    private:
        friend class query_batch;
        mc_ctx* ctx_ = nullptr; std::uint32_t slot_ = 0;
        mc_results res_{};
        std::vector<match_candidate> tops_;
        std::vector<mc_assignment> assigned_;
        std::vector<mc_candidate> kept_;
        std::vector<mc_verdict> verdicts_;
        std::string lines_, pieces_;
        std::vector<std::uint64_t> lineOff_, pieceOff_;
    };

    query_batch(const database& db, unsigned numHostThreads) : ctx_(db.ctx_), hosts_(numHostThreads)
    {
        if (numHostThreads > db.slots_) throw std::runtime_error("query_batch: more host threads than slots (mc_config.num_slots)");
        for (unsigned i = 0; i < numHostThreads; ++i) { hosts_[i].ctx_ = ctx_; hosts_[i].slot_ = i; }
    }
    // returns false if the batch is full (submit, wait, clear, then add again)      query_batch.cuh:383-391
    template <class Sequence>
    bool add_paired_read(unsigned hostId, const Sequence& seq1, const Sequence& seq2, const candidate_generation_rules& rules)
    {
        const int rc = mc_batch_add(ctx_, hostId, seq1.data(), std::uint32_t(seq1.size()), seq2.data(), std::uint32_t(seq2.size()),
                                    rules.maxWindowsInRange);
        if (rc < 0) throw std::runtime_error(mc_last_error(ctx_));
        return rc == MC_OK;
    }
    // a byte range of a FASTA / FASTQ file (whole records) into an EMPTY batch: the reads are cut on the device when the batch is
    // submitted (mc_batch_add_file_bytes).  Returns false if the range exceeds the batch's character capacity.
    bool add_file_bytes(unsigned hostId, const char* bytes, std::size_t nbytes, bool pairs = false, std::uint64_t insertSizeMax = 0)
    {
        const int rc = mc_batch_add_file_bytes(ctx_, hostId, bytes, nbytes, pairs ? MC_PARSE_PAIRS : 0, insertSizeMax);
        if (rc < 0) throw std::runtime_error(mc_last_error(ctx_));
        return rc == MC_OK;
    }
    // the same for a range that lies in DEVICE memory already (any address; untouched until wait_for_results returns): one copy on the
    // device instead of the upload, and the headers come back with the results -- host_data(hostId).headers() (mc_batch_add_device_bytes)
    bool add_device_bytes(unsigned hostId, const void* deviceBytes, std::size_t nbytes, bool pairs = false, std::uint64_t insertSizeMax = 0)
    {
        const int rc = mc_batch_add_device_bytes(ctx_, hostId, deviceBytes, nbytes, pairs ? MC_PARSE_PAIRS : 0, insertSizeMax);
        if (rc < 0) throw std::runtime_error(mc_last_error(ctx_));
        return rc == MC_OK;
    }
    // the byte ranges of two mate files (whole records; query q = record q of each) into an EMPTY batch (mc_batch_add_file_mates).
    // Returns false if the two ranges together exceed the batch's character capacity.
    bool add_file_mates(unsigned hostId, const char* bytes1, std::size_t n1, const char* bytes2, std::size_t n2, std::uint64_t insertSizeMax = 0)
    {
        const int rc = mc_batch_add_file_mates(ctx_, hostId, bytes1, n1, bytes2, n2, insertSizeMax);
        if (rc < 0) throw std::runtime_error(mc_last_error(ctx_));
        return rc == MC_OK;
    }
    query_host_data& host_data(unsigned hostId) noexcept { return hosts_[hostId]; }

private:
    friend class database;
    mc_ctx* ctx_;
    std::vector<query_host_data> hosts_;
};

inline void database::query_gpu_async(query_batch& batch, unsigned hostId, taxon_rank lowestRank) const
{
    (void)batch;
    if (mc_batch_submit(ctx_, hostId, int(lowestRank)) != MC_OK) throw std::runtime_error(mc_last_error(ctx_));
}

// per-part result files merged on the device (mc_merge_results_*; the reference's mode_merge.cpp): a context of its own without a table.
// set_taxa gives every taxon's ranked lineage (taxon index + 1, 0 = none), rank and taxid; begin makes the store; add folds one file (or
// one piece of a file, in order); lists() / classify() read the store.  A range the device refuses leaves the store as it was.
class result_merger {
public:
    struct status { std::uint64_t lines, comments, lists, entries, unknown, verdict, offence, needed; };
    struct merged_lists {
        std::uint32_t max_candidates = 0;
        std::vector<mc_taxon_candidate> lists;       // [queries][max_candidates], a list ends at hits == 0
        std::vector<std::uint32_t> header_place;     // [queries][3]: call, offset, length (0: none)
        std::uint64_t queries = 0;
    };

    explicit result_merger(int device = 0)
    {
        mc_config c;
        mc_config_default(&c);
        c.device = device;
        if (mc_create(&c, &ctx_) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
    }
    result_merger(const result_merger&) = delete;
    result_merger& operator=(const result_merger&) = delete;
    ~result_merger() { if (ctx_) { mc_merge_results_end(ctx_); mc_destroy(ctx_); } }
    mc_ctx* handle() const noexcept { return ctx_; }

    void set_taxa(const std::uint32_t* lin, const std::uint8_t* rank, const std::int64_t* ids, std::uint64_t numTaxa)
    {
        check(mc_set_taxon_table(ctx_, lin, rank, nullptr, numTaxa));
        check(mc_merge_results_set_taxids(ctx_, ids, numTaxa));
    }
    void begin(std::uint64_t capacityQueries, std::uint32_t maxCandidates = 2, std::int32_t mergeBelow = 4)
    {
        check(mc_merge_results_begin(ctx_, capacityQueries, maxCandidates, mergeBelow));
        capacity_ = capacityQueries; maxCand_ = maxCandidates;
    }
    void reserve(std::uint64_t capacityQueries) { check(mc_merge_results_reserve(ctx_, capacityQueries)); capacity_ = std::max(capacity_, capacityQueries); }
    // host bytes; fileLines 0: the range is the whole file.  MC_MERGE_OVERFLOW is answered here by one reserve and a second call.
    status add(const char* bytes, std::size_t nbytes, std::uint32_t tophitsColumn, std::uint64_t fileLines = 0, bool cont = false)
    {
        std::uint64_t st[8];
        for (int attempt = 0;; ++attempt) {
            check(mc_merge_results_add(ctx_, bytes, nbytes, tophitsColumn, fileLines, MC_MERGE_HOST | (cont ? MC_MERGE_CONTINUE : 0), st, nullptr, 0, nullptr));
            ++calls_;
            if (st[5] != MC_MERGE_OVERFLOW || attempt == 1) break;
            reserve(st[7]);
        }
        return status{st[0], st[1], st[2], st[3], st[4], st[5], st[6], st[7]};
    }
    std::uint32_t calls() const noexcept { return calls_; }      // add calls so far, the retries included: the next one's number in a header place
    merged_lists lists() const
    {
        merged_lists m;
        m.max_candidates = maxCand_;
        check(mc_merge_results_lists(ctx_, 0, 0, MC_MERGE_HOST, nullptr, nullptr, &m.queries, nullptr));
        m.lists.resize(m.queries * maxCand_);
        m.header_place.resize(m.queries * 3);
        if (m.queries) check(mc_merge_results_lists(ctx_, 0, m.queries, MC_MERGE_HOST, m.lists.data(), m.header_place.data(), nullptr, nullptr));
        return m;
    }
    std::vector<mc_assignment> classify(const mc_classify_options& opt, bool tally = false) const
    {
        std::uint64_t n = 0;
        check(mc_merge_results_lists(ctx_, 0, 0, MC_MERGE_HOST, nullptr, nullptr, &n, nullptr));
        std::vector<mc_assignment> out(n);
        if (n) check(mc_merge_results_classify(ctx_, &opt, MC_CLASSIFY_HOST | (tally ? MC_CLASSIFY_TALLY : 0), 0, n, out.data(), nullptr));
        return out;
    }
    std::vector<std::uint64_t> stats() const
    {
        std::vector<std::uint64_t> s(6);
        check(mc_merge_results_stats(ctx_, s.data()));
        return s;
    }
    // the tallies of the classify(opt, true) calls (mc_classify_tally): assigned[r] = queries whose result has rank r ([MC_NUM_RANKS]:
    // unclassified); returns the queries per taxon entry
    std::vector<std::uint64_t> tally(std::uint64_t assigned[MC_NUM_RANKS + 1], bool reset = false) const
    {
        std::uint64_t n = 0;
        check(mc_classify_tally(ctx_, nullptr, nullptr, 0, &n, 0));
        std::vector<std::uint64_t> perTaxon(n);
        check(mc_classify_tally(ctx_, assigned, perTaxon.data(), n, nullptr, reset ? 1 : 0));
        return perTaxon;
    }

private:
    void check(int rc) const { if (rc < 0) throw std::runtime_error(mc_last_error(ctx_)); }
    mc_ctx* ctx_ = nullptr;
    std::uint64_t capacity_ = 0;
    std::uint32_t maxCand_ = 0, calls_ = 0;
};

// targets ranked from accession2taxid tables on the device (mc_taxmap_*; the reference's try_to_rank_unranked_targets): a context of its
// own without a table.  begin takes the target names in ascending order (a std::map's order) with a flag per name; add matches one
// piece of a table (whole lines, the file's first line dropped, in order); result() gives every name's taxid and where its row was.
// A range the device refuses changes nothing.
class accession_mapper {
public:
    struct status { std::uint64_t lines, targeted, wanted, ranked, remaining, verdict, offence; };
    struct ranking {
        std::vector<std::int64_t> taxid;             // per name; 0 where not found
        std::vector<std::uint64_t> position;         // call * 2^32 + line start; not_found: no row named the name
        std::uint64_t remaining = 0;                 // wanted names without a row
    };
    static constexpr std::uint64_t not_found = ~std::uint64_t(0);

    explicit accession_mapper(int device = 0)
    {
        mc_config c;
        mc_config_default(&c);
        c.device = device;
        if (mc_create(&c, &ctx_) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
    }
    accession_mapper(const accession_mapper&) = delete;
    accession_mapper& operator=(const accession_mapper&) = delete;
    ~accession_mapper() { if (ctx_) { mc_taxmap_end(ctx_); mc_destroy(ctx_); } }
    mc_ctx* handle() const noexcept { return ctx_; }

    // names strictly ascending (std::string's order); wanted: a flag per name, empty = all
    void begin(const std::vector<std::string>& names, const std::vector<std::uint8_t>& wanted = {})
    {
        std::string text;
        std::vector<std::uint64_t> off(1, 0);
        for (const std::string& n : names) { text += n; off.push_back(text.size()); }
        const std::vector<std::uint8_t> all(names.size(), 1);
        if (!wanted.empty() && wanted.size() != names.size()) throw std::invalid_argument("accession_mapper::begin: one flag per name");
        check(mc_taxmap_begin(ctx_, text.data(), off.data(), names.size(), (wanted.empty() ? all : wanted).data()));
        count_ = names.size();
    }
    status add(const char* bytes, std::size_t nbytes)
    {
        std::uint64_t st[8];
        check(mc_taxmap_add(ctx_, bytes, nbytes, MC_TAXMAP_HOST, st, nullptr, 0, nullptr));
        return status{st[0], st[1], st[2], st[3], st[4], st[5], st[6]};
    }
    ranking result() const
    {
        ranking r;
        r.taxid.resize(count_); r.position.resize(count_);
        check(mc_taxmap_result(ctx_, r.taxid.data(), r.position.data(), &r.remaining, MC_TAXMAP_HOST, nullptr));
        return r;
    }
    std::vector<std::uint64_t> stats() const
    {
        std::vector<std::uint64_t> s(8);
        check(mc_taxmap_stats(ctx_, s.data()));
        return s;
    }

private:
    void check(int rc) const { if (rc < 0) throw std::runtime_error(mc_last_error(ctx_)); }
    mc_ctx* ctx_ = nullptr;
    std::uint64_t count_ = 0;
};

}  // namespace mc_amd

#endif
