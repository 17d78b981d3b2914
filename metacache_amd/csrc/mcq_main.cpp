// mcq -- the reference's command lines on MI355X, host C++14 above the C ABI (include/metacache_amd.h):
//   mcq query <database> [<reads.fa|fq[.gz]|directory>...] [options]     mode_query.cpp, querying.cpp (interactive without files)
//   mcq build <database> <sequence files|directories>... [options]        mode_build.cpp, building.cpp        (mcq_build.h)
//   mcq modify <database> <sequence files|directories>... [options]       mode_build.cpp:74-88: adds to an existing database (mcq_build.h)
//   mcq build+query -targets <files>... [-query <files>...] [options]     mode_build_query.cpp                (mcq_build.h)
//   mcq merge <result files>... -taxonomy <dir> [options]                 mode_merge.cpp
//   mcq info [<database> [targets [name...] | lineages | rank <r>]]       mode_info.cpp (metadata topics)
// Query mode mirrors
//   option handling      options.cpp:860-1430 (query subset), querying.cpp:225-269 (adapt_options_to_database)
//   read ingest          sequence_io.cpp:160-228, :293-322 (FASTA / FASTQ, -pairfiles / -pairseq), database_query.hpp:258-284;
//                        files are memory-mapped (gzip: inflated into memory), record starts are indexed by all
//                        threads in parallel (query ids = record order, as reader.index()), and every worker thread drives one
//                        batch slot: parse -> mc_batch_add -> submit -> wait -> classify + format; output is written in file order
//   classification       classification.cpp:146-189 (classify: ranked-LCA vote over the top candidates), :104-137 (ground truth),
//                        :272-295 (evaluation), :304-374 (abundance estimation)
//   output lines         classification.cpp:470-526 (show_query_mapping), printing.cpp:47-620 (parameters, candidates, matches,
//                        hits per reference sequence, abundance tables, summary)
// Options: -out -split-out -lowest -highest -hitmin -hitdiff -maxcand -tophits -allhits -locations -queryids -mapped-only -no-map
//   -taxids -taxids-only -omit-ranks -separate-cols -separator -comment -lineage -pairfiles -pairseq -insertsize -min-readlen
//   -max-readlen -query-limit -sketchlen -winlen -winstride -max-locations-per-feature -remove-overpopulated-features -max-load-fac
//   -no-query-params -no-summary -no-err -threads -batch-size -abundances [file] -abundance-per <rank> -hits-per-ref [file]
//   -ground-truth -precision -taxon-coverage -cov-percentile -align (alignment on the device: mc_align_semiglobal).
#include "mcq_build.h"

#include <fcntl.h>
#include <unistd.h>

namespace {

using namespace mcq;

struct Options {
    std::string db, outfile;
    std::vector<std::string> infiles;
    int lowest = 0, highest = 19;                    // sequence .. domain (options.hpp:246-260)
    int hitsMin = 0; float hitsDiff = 1.0f;
    float covPercentile = 0.0f;          // -cov-percentile (options.cpp:918-930, :1313)
    uint64_t maxCand = 2, insertMax = 0;
    enum Pairing { unpaired, files, sequences } pairing = unpaired;
    bool tophits = false, allhits = false, locations = false, queryIds = false, lineage = false, separateCols = false;
    bool showName = true, showRank = true, showId = false;
    enum MapView { mv_none, mv_mapped, mv_all } mapView = mv_all;
    bool collapseUnclassified = true;
    std::string comment = "# ", none = "--", column = "\t|\t", taxSep = ",", rankSuffix = ":", idPrefix = "(", idSuffix = ")";
    bool showQueryParams = true, showSummary = true, showErrors = true, splitOut = false;
    uint32_t sketchlen = 0, winlen = 0, winstride = 0, batchSize = 1u << 16;
    uint32_t residentParts = 0;          // -resident-parts n (this program's own): a partitioned database n parts at a time, the next group loading behind
                                         // the queries (mc_partset_*; the reference's workflow: one query run per part + merge, docs/partitioning.md:116-153)
    std::vector<int32_t> gpus;           // -gpus a,b,...: the resident parts dealt out over these GPUs, per-part candidates gathered over RCCL
    bool shardKeys = false;              // -shard keys: ONE database key-sharded over the GPUs of -gpus (mc_keyset_*: every GPU holds the features it owns, the partial
                                         // location lists travel over RCCL to the GPU that owns the read); -shard parts = the default of -gpus (parts over GPUs)
    bool shardTargets = false;           // -shard targets: ONE database file cut into contiguous target ranges at load (mc_config.target_shard_*), a range per GPU of -gpus
    uint32_t targetShards = 0;           // -target-shards n: number of ranges (default: one per GPU of -gpus); with -resident-parts m: m ranges in HBM at a time
    uint32_t keyShards = 0;              // -key-shards n: number of key shards (default: one per GPU of -gpus; more than one per GPU on a single device)
    uint32_t replication = 1;            // -replicate: copies of the table on GPUs 0 .. n-1, the workers are dealt out over them (options.cpp:1155-1163)
    uint32_t refBatchSize = 0;           // -batch-size as given (the reference's batches matter for -cov-percentile)
    int maxLocs = -1, threads = 0;
    bool removeOverpopulated = false; float maxLoadFac = 0;
    uint64_t minReadLen = 0, maxReadLen = std::numeric_limits<uint64_t>::max();
    int64_t queryLimit = std::numeric_limits<int64_t>::max();
    bool hitsPerRef = false, abundances = false;
    bool showGroundTruth = false, determineGroundTruth = false, precision = false, taxonCoverage = false;
    bool align = false;                  // -align: the read against its best candidate's range of the target record (classification.cpp:384-426)
    int abundancePer = kNumRanks;                    // none
    std::string targetsFile, abundanceFile;
};

std::string sanitize_special_chars(const std::string& s)   // cmdline_utility: "\t" etc. typed literally
{
    std::string r;
    for (size_t i = 0; i < s.size(); ++i) {
        if (s[i] == '\\' && i + 1 < s.size()) {
            const char c = s[i + 1];
            if (c == 't') { r += '\t'; ++i; continue; }
            if (c == 'n') { r += '\n'; ++i; continue; }
        }
        r += s[i];
    }
    return r;
}

// Command line options of `metacache query` (options.cpp:860-1295); 'o' carries the defaults (interactive mode: the options of
// the initial command line).  args = everything after the database name.
Options parse(const std::vector<std::string>& args, Options o)
{
    o.infiles.clear();
    auto need = [&](size_t& i) -> std::string { if (i + 1 >= args.size()) throw std::runtime_error("value missing after '" + args[i] + "'"); return args[++i]; };
    for (size_t i = 0; i < args.size(); ++i) {
        const std::string& a = args[i];
        if (a.empty()) continue;
        if (a[0] != '-') { o.infiles.push_back(a); continue; }
        if (a == "-out") o.outfile = need(i);
        else if (a == "-split-out" || a == "-splitout") { o.splitOut = true; o.outfile = need(i); }
        else if (a == "-lowest") { int r = rank_from_name(need(i)); if (r < 0) throw std::runtime_error("unknown rank"); o.lowest = r; }
        else if (a == "-highest") { int r = rank_from_name(need(i)); if (r < 0) throw std::runtime_error("unknown rank"); o.highest = r; }
        else if (a == "-cov-percentile") { o.covPercentile = std::stof(need(i)); if (o.covPercentile > 1) o.covPercentile *= 0.01f; }
        else if (a == "-hitmin" || a == "-hit-min" || a == "-hits-min" || a == "-hitsmin") o.hitsMin = std::stoi(need(i));
        else if (a == "-hitdiff" || a == "-hit-diff" || a == "-hitsdiff" || a == "-hits-diff") o.hitsDiff = std::stof(need(i));
        else if (a == "-maxcand" || a == "-max-cand") o.maxCand = std::stoull(need(i));
        else if (a == "-tophits" || a == "-top-hits") o.tophits = true;
        else if (a == "-allhits" || a == "-all-hits") o.allhits = true;
        else if (a == "-locations") { o.locations = true; o.tophits = true; }
        else if (a == "-queryids" || a == "-query-ids") o.queryIds = true;
        else if (a == "-align" || a == "-alignment") o.align = true;
        else if (a == "-ground-truth") { o.determineGroundTruth = true; o.showGroundTruth = true; }
        else if (a == "-precision") { o.precision = true; o.determineGroundTruth = true; }
        else if (a == "-taxon-coverage") { o.taxonCoverage = true; o.precision = true; o.determineGroundTruth = true; }
        // an optional file name follows (clipp opt_value: the next word unless it is an option)
        else if (a == "-abundances" || a == "-abundance") { o.abundances = true; if (i + 1 < args.size() && args[i + 1][0] != '-') o.abundanceFile = args[++i]; }
        else if (a == "-abundance-per") { int r = rank_from_name(need(i)); if (r < 0) throw std::runtime_error("unknown rank"); if (r < kNumRanks - 1) o.abundancePer = r; }
        else if (a == "-hits-per-ref" || a == "-hits-per-seq" || a == "-hits-per-tgt" || a == "-hits-per-target") {
            o.hitsPerRef = true; if (i + 1 < args.size() && args[i + 1][0] != '-') o.targetsFile = args[++i]; }
        else if (a == "-mapped-only" || a == "-mappedonly") o.mapView = Options::mv_mapped;
        else if (a == "-no-map" || a == "-nomap") o.mapView = Options::mv_none;
        else if (a == "-taxids" || a == "-taxid") o.showId = true;
        else if (a == "-taxids-only" || a == "-taxidsonly") { o.showId = true; o.showName = false; }
        else if (a == "-omit-ranks" || a == "-omitranks") o.showRank = false;
        else if (a == "-separate-cols" || a == "-separatecols") o.separateCols = true;
        else if (a == "-separator") o.column = sanitize_special_chars(need(i));
        else if (a == "-comment") o.comment = need(i);
        else if (a == "-lineage" || a == "-lineages") o.lineage = true;
        else if (a == "-pairfiles" || a == "-pair-files" || a == "-paired-files") o.pairing = Options::files;
        else if (a == "-pairseq" || a == "-pair-seq" || a == "-paired-seq") o.pairing = Options::sequences;
        else if (a == "-insertsize" || a == "-insert-size") o.insertMax = std::stoull(need(i));
        else if (a == "-min-readlen") o.minReadLen = std::stoull(need(i));
        else if (a == "-max-readlen") o.maxReadLen = std::stoull(need(i));
        else if (a == "-query-limit") o.queryLimit = std::stoll(need(i));
        else if (a == "-sketchlen") o.sketchlen = (uint32_t)std::stoul(need(i));
        else if (a == "-winlen") o.winlen = (uint32_t)std::stoul(need(i));
        else if (a == "-winstride") o.winstride = (uint32_t)std::stoul(need(i));
        else if (a == "-max-locations-per-feature") o.maxLocs = std::stoi(need(i));
        else if (a == "-remove-overpopulated-features") o.removeOverpopulated = true;
        else if (a == "-max-load-fac" || a == "-max-load-factor") o.maxLoadFac = std::stof(need(i));
        else if (a == "-no-query-params" || a == "-no-queryparams") o.showQueryParams = false;
        else if (a == "-no-summary" || a == "-nosummary") o.showSummary = false;
        else if (a == "-no-err" || a == "-no-errors") o.showErrors = false;
        else if (a == "-threads") o.threads = std::stoi(need(i));
        else if (a == "-replicate") o.replication = (uint32_t)std::max(1, std::stoi(need(i)));
        else if (a == "-resident-parts") o.residentParts = (uint32_t)std::max(1, std::stoi(need(i)));
        else if (a == "-shard") {
            const std::string v = need(i);
            o.shardKeys = v == "keys"; o.shardTargets = v == "targets";
            if (v != "keys" && v != "parts" && v != "targets") throw std::runtime_error("-shard parts|keys|targets");
        }
        else if (a == "-target-shards") o.targetShards = (uint32_t)std::max(1, std::stoi(need(i)));
        else if (a == "-key-shards") o.keyShards = (uint32_t)std::max(1, std::stoi(need(i)));
        else if (a == "-gpus") {
            std::stringstream ss(need(i));
            for (std::string t; std::getline(ss, t, ',');) if (!t.empty()) o.gpus.push_back((int32_t)std::stoi(t));
        }
        else if (a == "-batch-size" || a == "-batchsize") { o.batchSize = (uint32_t)std::stoul(need(i)); o.refBatchSize = o.batchSize; }
        else throw std::runtime_error("unknown option '" + a + "'");
    }
    // process_query_options (options.cpp:1297-1366)
    {   // replace_directories_with_contained_files (options.cpp:146-165)
        std::vector<std::string> expanded;
        for (const auto& name : o.infiles) {
            auto sub = files_in_directory(name);
            if (sub.empty()) expanded.push_back(name); else expanded.insert(expanded.end(), sub.begin(), sub.end());
        }
        o.infiles.swap(expanded);
    }
    if (o.pairing == Options::files) { if (o.infiles.size() > 1) std::sort(o.infiles.begin(), o.infiles.end()); else o.pairing = Options::unpaired; }
    if (o.hitsDiff > 1) o.hitsDiff *= 0.01;       // double factor, as options.cpp:1312
    if (o.lowest > o.highest) o.lowest = o.highest;
    if (o.batchSize < 1) o.batchSize = 1;
    if (o.queryLimit < 0) o.queryLimit = 0;
    if (o.targetsFile == o.outfile) o.targetsFile.clear();
    if (o.abundanceFile == o.outfile) o.abundanceFile.clear();
    if (o.hitsPerRef) o.queryIds = true;
    if (o.separateCols) { o.collapseUnclassified = false; o.taxSep = o.column; o.rankSuffix = o.column; o.idPrefix = o.column; o.idSuffix = ""; }
    if (o.mapView == Options::mv_none && o.tophits) o.mapView = Options::mv_mapped;
    else if (o.allhits) o.mapView = Options::mv_all;
    return o;
}

// host threads worth running: the cgroup's CPU quota where there is one (a box may show 256 CPUs and grant 16), else the hardware threads
static unsigned granted_cpus()
{
    unsigned n = std::max(1u, std::thread::hardware_concurrency());
    if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
        char q[32] = {0}; long long period = 0;
        if (std::fscanf(f, "%31s %lld", q, &period) == 2 && std::strcmp(q, "max") != 0 && period > 0) {
            const long long quota = std::atoll(q);
            if (quota > 0) n = std::max(1u, std::min(n, (unsigned)((quota + period / 2) / period)));
        }
        std::fclose(f);
    }
    return n;
}

// ---- output (printing.cpp:160-365) ----------------------------------------------------------------------------------
// The mapping lines of a batch are put together by its worker thread in a plain byte buffer: the inserters the line formatters use,
// without a stream's locale and sentry work per field (10^7 lines of `-tophits -queryids` took 5.7 s of CPU through std::ostringstream --
// 0.36 s of a 0.52 s query phase on the 16 granted cores -- against 0.6 s of kernels).  Same bytes as operator<< of std::ostream writes
// for these types (integers in decimal, strings and characters as they are).
struct FastOut {
    std::string s;
    FastOut& operator<<(char c) { s.push_back(c); return *this; }
    FastOut& operator<<(const char* p) { s.append(p); return *this; }
    FastOut& operator<<(const std::string& t) { s.append(t); return *this; }
    FastOut& put_u64(uint64_t v)
    {
        char b[24]; int i = 24;
        do { b[--i] = (char)('0' + v % 10); v /= 10; } while (v);
        s.append(b + i, (size_t)(24 - i));
        return *this;
    }
    FastOut& put_i64(int64_t v) { if (v < 0) { s.push_back('-'); return put_u64(0 - (uint64_t)v); } return put_u64((uint64_t)v); }
    template <class T, typename std::enable_if<std::is_integral<T>::value && std::is_unsigned<T>::value && !std::is_same<T, char>::value && !std::is_same<T, bool>::value, int>::type = 0>
    FastOut& operator<<(T v) { return put_u64((uint64_t)v); }
    template <class T, typename std::enable_if<std::is_integral<T>::value && std::is_signed<T>::value && !std::is_same<T, char>::value, int>::type = 0>
    FastOut& operator<<(T v) { return put_i64((int64_t)v); }
    FastOut& write(const char* p, std::streamsize n) { s.append(p, (size_t)n); return *this; }
    void str(const std::string& t) { s = t; }                  // (reset, as std::ostringstream::str(std::string()))
    const std::string& str() const { return s; }
};

template <class OS>
void print_taxon(OS& os, const Options& o, const std::string& name, int64_t id, int rank)
{
    if (o.showRank) { if (rank == kNumRanks) os << o.none; else os << kRankNames[rank]; os << o.rankSuffix; }
    if (o.showName) { os << name; if (o.showId) os << o.idPrefix << id << o.idSuffix; }
    else if (o.showId) os << id;
}

template <class OS>
void show_lineage(OS& os, const Options& o, const Taxonomy& tx, const Lineage& lin, int lowest, int highest)
{
    if (lowest == kNumRanks) return;
    if (highest == kNumRanks) highest = kNumRanks - 1;
    for (int r = lowest; r <= highest; ++r) {
        const Taxon* t = tx.taxon(lin[r]);
        if (t) print_taxon(os, o, t->name, t->id, t->rank); else print_taxon(os, o, o.none, 0, r);
        if (r < highest) os << o.taxSep;
    }
}

template <class OS>
void show_taxon(OS& os, const Options& o, const Taxonomy& tx, uint32_t best /* idx+1 */, bool bestIsTarget, uint32_t bestTgt)
{
    const Taxon* t = tx.taxon(best);
    if (!t || t->rank > o.highest) {
        if (o.collapseUnclassified) {
            if (o.showId && !o.showName && !o.showRank) os << 0; else os << o.none;
        } else {
            const int rmax = o.lineage ? o.highest : o.lowest;
            for (int r = o.lowest; r <= rmax; ++r) { print_taxon(os, o, o.none, 0, kNumRanks); if (r < rmax) os << o.taxSep; }
        }
    } else {
        const int rmin = o.lowest < t->rank ? t->rank : o.lowest;
        const int rmax = o.lineage ? o.highest : rmin;
        const Lineage lin = bestIsTarget ? tx.target_ranks(bestTgt) : tx.ranks_of(best);
        show_lineage(os, o, tx, lin, rmin, rmax);
    }
}

struct Cand { uint32_t tgt, hits, beg, end; uint32_t tax; /* idx+1 */ };

template <class OS>
void show_candidates(OS& os, const Options& o, const Taxonomy& tx, const std::vector<Cand>& c)
{
    for (size_t i = 0; i < c.size() && c[i].hits > 0; ++i) {
        if (i > 0) os << ',';
        const Taxon* t = tx.taxon(c[i].tax);
        if (o.lowest == 0) { if (t) os << t->name << ':' << c[i].hits; }
        else {
            const Taxon* a = t;
            if (t && t->rank < o.lowest) a = tx.taxon(tx.target_ranks(c[i].tgt)[o.lowest]);
            if (a) os << a->id; else os << t->name;
            os << ':' << c[i].hits;
        }
    }
}

template <class OS>
void show_matches(OS& os, const Options& o, const Taxonomy& tx, const mc_location* hits, uint64_t n)
{
    if (n == 0) return;
    auto emit = [&](const mc_location& cur, int count) {
        const Lineage lin = tx.target_ranks(cur.tgt);
        if (o.lowest == 0) { const Taxon* t = tx.taxon(lin[0]); if (t) os << t->name << '/' << int(cur.win) << ':' << count << ','; }
        else { const Taxon* t = tx.taxon(lin[o.lowest]); if (!t) t = tx.taxon(lin[0]); os << t->name << ':' << count << ','; }
    };
    uint64_t cur = 0; int count = 1;
    for (uint64_t i = 1; i < n; ++i) {
        if (hits[cur].tgt == hits[i].tgt && hits[cur].win == hits[i].win) ++count;
        else { emit(hits[cur], count); cur = i; count = 1; }
    }
    emit(hits[cur], count);
}

// ---- ground truth from the query header (classification.cpp:104-137; sequence_io.cpp:479-673) ---------------------------
uint32_t ground_truth(const Taxonomy& tx, const std::string& header)
{
    if (header.empty()) return 0;
    std::smatch m;
    std::regex_search(header, m, accession_regex());
    uint32_t t = tx.with_name(m[4].length() ? m[2].str() : std::string());      // accession.version
    if (t) return tx.next_ranked_ancestor(t);
    t = tx.with_similar_name(m[3].str());                                       // accession, any version
    if (t) return tx.next_ranked_ancestor(t);
    t = tx.with_id(taxon_id_in_header(header));
    if (t) return tx.next_ranked_ancestor(t);
    t = tx.with_name(header);
    if (t) return tx.next_ranked_ancestor(t);
    t = tx.with_name(leading_word(header));
    if (t) return tx.next_ranked_ancestor(t);
    t = tx.with_name(filename_without_extension(header));
    if (t) return tx.next_ranked_ancestor(t);
    return 0;
}

// classification.cpp:146-189
uint32_t classify(const Options& o, const Taxonomy& tx, const std::vector<Cand>& cand, bool& isTarget, uint32_t& tgt)
{
    isTarget = false; tgt = 0;
    if (cand.empty() || cand[0].hits == 0 || !cand[0].tax) return 0;
    if (cand[0].hits < (uint32_t)o.hitsMin) return 0;
    uint32_t lca = cand[0].tax;
    const float threshold = cand[0].hits > (uint32_t)o.hitsMin ? (cand[0].hits - o.hitsMin) * o.hitsDiff : 0;
    auto ranks = [&](const Cand& c) { return c.tgt < tx.numTargets ? tx.target_ranks(c.tgt) : tx.ranks_of(c.tax); };   // classification.cpp:166-176
    const Lineage top = ranks(cand[0]);
    for (size_t i = 1; i < cand.size() && cand[i].hits > 0; ++i) {
        if (cand[i].hits > threshold) {
            const Lineage cr = ranks(cand[i]);
            const int from = tx.taxon(lca)->rank;
            uint32_t l = 0;
            for (int r = from; r <= kNumRanks - 1; ++r) if (top[r] && top[r] == cr[r]) { l = top[r]; break; }   // ranked_lca
            lca = l;
            if (!lca || tx.taxon(lca)->rank > o.highest) return 0;
        } else break;
    }
    if (!lca || tx.taxon(lca)->rank > o.highest) return 0;
    if (lca == cand[0].tax && tx.taxon(lca)->rank == 0) { isTarget = true; tgt = cand[0].tgt; }
    return lca;
}

// lowest_ranked_ancestor of a target's taxon: on rank 'lowest' or the closest one above it (0: none, or not a target)
uint32_t lowest_ranked_ancestor(const Taxonomy& tx, uint32_t tgt, int lowest)
{
    if (tgt >= tx.numTargets) return 0;
    const uint32_t* lin = tx.targetLineages + (size_t)tgt * kNumRanks;
    if (lowest <= 0) return lin[0];
    for (int rk = lowest; rk < kNumRanks; ++rk) if (lin[rk]) return lin[rk];
    return 0;
}

// one query's device candidate list (K entries, the used ones first) as Cands
void device_candidates(const mc_candidate* c, uint32_t K, const Taxonomy& tx, int lowest, std::vector<Cand>& out)
{
    out.clear();
    for (uint32_t j = 0; j < K && c[j].hits != 0; ++j) out.push_back(Cand{c[j].tgt, c[j].hits, c[j].beg, c[j].end, lowest_ranked_ancestor(tx, c[j].tgt, lowest)});
}

// ---- database session: the loaded context is kept between jobs (interactive mode) as long as its load-time settings fit ----
// Rows 9-10 on the host for ONE read's sorted location list: the reference's loop (for_all_contiguous_window_ranges,
// candidate_generation.hpp:47-108) and its sorted insert without a limit (:172-231, same std:: calls so that equal hit counts fall
// the same way).  Used when -maxcand 0 meets a read with more candidates than the device list holds.
static void host_candidates(const mc_location* h, uint64_t n, uint32_t maxWin, const Taxonomy& tx, int lowest, std::vector<Cand>& top)
{
    top.clear();
    auto greater = [](const Cand& a, const Cand& b) { return a.hits > b.hits; };
    auto insert = [&](Cand c) {
        c.tax = lowest_ranked_ancestor(tx, c.tgt, lowest);
        if (!c.tax) return;
        if (lowest <= 0) { top.insert(std::upper_bound(top.begin(), top.end(), c, greater), c); return; }
        auto i = std::find_if(top.begin(), top.end(), [&](const Cand& x) { return x.tax == c.tax; });
        if (i != top.end()) { if (c.hits > i->hits) { *i = c; std::sort(top.begin(), i + 1, greater); } }
        else top.insert(std::upper_bound(top.begin(), top.end(), c, greater), c);
    };
    if (n == 0) return;
    uint64_t fst = 0;
    uint32_t hits = 1;
    Cand best{h[0].tgt, 1, h[0].win, h[0].win, 0};
    for (uint64_t lst = 1; lst < n; ++lst) {
        if (h[lst].tgt == best.tgt) {
            ++hits;
            while (fst != lst && (uint32_t)(h[lst].win - h[fst].win) >= maxWin) { --hits; ++fst; }
            if (hits > best.hits) { best.hits = hits; best.beg = h[fst].win; best.end = h[lst].win; }
        } else {
            insert(best);
            fst = lst; hits = 1;
            best = Cand{h[lst].tgt, 1, h[lst].win, h[lst].win, 0};
        }
    }
    insert(best);
}

void read_taxa(mc_ctx* ctx, Taxonomy& tx)                                  // the taxa of a context's metadata
{
    uint64_t nt = 0; mc_db_num_taxa(ctx, &nt); tx.taxa.resize(nt);
    for (uint64_t i = 0; i < nt; ++i) {
        uint32_t rk; const char* nm;
        mc_db_taxon(ctx, i, &tx.taxa[i].id, &tx.taxa[i].parent, &rk, &nm);
        tx.taxa[i].rank = int(rk); tx.taxa[i].name = nm;
        const char* src = nullptr;
        mc_db_taxon_source(ctx, i, &src, &tx.taxa[i].srcIndex, &tx.taxa[i].windows);
        if (src) tx.taxa[i].srcFile = src;
    }
}

struct Session {
    mc_ctx* ctx = nullptr;
    mc_config cfg{};
    std::string db;
    Taxonomy tx;
    uint32_t dbStride = 0, dbSketch = 0, dbWinlen = 0;
    unsigned threads = 1, workers = 1;
    std::vector<mc_ctx*> replicas;                   // -replicate n: the same table on the GPUs 1 .. n-1 (ctx is the one on GPU 0)
    uint32_t replication = 1;
    mc_partset* partset = nullptr;                   // -resident-parts / -gpus: the parts as contexts of their own (ctx then holds the metadata only)
    mc_keyset* keyset = nullptr;                     // -shard keys: key shards as contexts of their own (ctx holds the metadata only)
    mc_ctx* replica(unsigned i) const { return i == 0 ? ctx : replicas[i - 1]; }
    void close_replicas() { for (mc_ctx* r : replicas) mc_destroy(r); replicas.clear(); }
    ~Session() { close_replicas(); if (partset) mc_partset_close(partset); if (keyset) mc_keyset_close(keyset); if (ctx) mc_destroy(ctx); }

    BuiltDatabase* built = nullptr;                  // build+query: the table comes from the builder's device arrays, not from files
    std::vector<uint32_t> builtLineages;

    static uint32_t unlimitedCap()
    {
        const char* e = std::getenv("MCQ_UNLIMITED_CAP");                       // tests: a small cap makes the host path run on toy data
        return e ? (uint32_t)std::max(1, std::atoi(e)) : 256u;
    }
    void open(const Options& o)
    {
        mc_config c; mc_config_default(&c);
        c.kmerlen = 0; c.sketchlen = o.sketchlen; c.winlen = o.winlen; c.winstride = o.winstride;
        // -maxcand 0 = no limit (options.cpp:1315-1317): the device lists hold unlimitedCap() candidates; a read that fills its list gets
        // its candidates from the HOST instead -- rows 9-10 over the read's sorted location list, which is copied back for that
        c.max_candidates = o.maxCand < 1 ? unlimitedCap() : (uint32_t)std::min<uint64_t>(o.maxCand, 4096);
        c.copy_allhits = (o.allhits || o.maxCand < 1) ? 1 : 0;
        const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
        threads = o.threads > 0 ? (unsigned)o.threads : hw;                     // options.hpp: numThreads defaults to all hardware threads
        workers = std::min(threads, 64u);                                      // one batch slot (pinned staging) per worker
        if (o.threads <= 0) workers = std::min(workers, std::max(8u, 2u * granted_cpus()));   // (a container's CPU quota: more runnable threads than twice that only get the group throttled)
        const uint32_t nrep = built ? 1u : std::max(1u, o.replication);
        workers = std::max(workers, nrep);
        c.num_slots = (workers + nrep - 1) / nrep;                              // worker w: replica w % n, slot w / n
        c.slot_max_queries = o.batchSize;
        c.slot_max_chars = std::max<uint32_t>(1u << 24, o.batchSize * 320u);
        // MCQ_PARSE_DEVICE=2 with -pairfiles: a slot takes the BYTES of a batch's records of both files, twice what one file's records take
        if (const char* sw = std::getenv("MCQ_PARSE_DEVICE"))
            if (std::atoi(sw) >= 2 && o.pairing == Options::files)
                c.slot_max_chars = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(c.slot_max_chars, (uint64_t)o.batchSize * 640u), 0xFFFFFF00ull);
        c.max_load_factor = o.maxLoadFac;
        if (built) {
            if (built->opt.maxLoadFac > 0.4f && built->opt.maxLoadFac < 0.99f) c.max_load_factor = built->opt.maxLoadFac;
        } else if (o.removeOverpopulated) {                                     // read_database, mode_query.cpp:69-92
            int maxlpf = o.maxLocs - 1;
            if (maxlpf < 0 || maxlpf >= 254) maxlpf = 253;
            c.remove_overpopulated = (uint32_t)maxlpf;                             // clamped to the DB's cap - 1 by mc_open_database
            c.max_locations_per_feature = o.maxLocs < 0 ? 0 : (uint32_t)std::max(1, o.maxLocs);
        } else if (o.maxLocs > 1) c.max_locations_per_feature = (uint32_t)o.maxLocs;
        const bool wantKeys = !built && o.shardKeys;
        const bool wantTargets = !built && o.shardTargets;
        const bool wantSet = !built && (o.residentParts > 0 || !o.gpus.empty() || wantKeys || wantTargets);
        if (ctx && db == o.db && std::memcmp(&c, &cfg, sizeof(c)) == 0 && replication == nrep && !wantSet && !partset && !keyset) return;  // same table, same slots: keep it
        close_replicas();
        if (partset) { mc_partset_close(partset); partset = nullptr; }
        if (keyset) { mc_keyset_close(keyset); keyset = nullptr; }
        if (ctx) { mc_destroy(ctx); ctx = nullptr; }
        replication = nrep;
        tx = Taxonomy{};
        if (wantSet) {
            if (o.allhits || o.maxCand < 1 || o.maxCand > 4 || o.covPercentile > 0)
                throw std::runtime_error("-resident-parts / -gpus / -shard: top candidates only (-maxcand 1..4, no -allhits, no -cov-percentile)");
            c.num_slots = 1;
            c.slot_max_queries = std::max<uint32_t>(o.batchSize, 1u << 16);
            c.slot_max_chars = std::max<uint32_t>(1u << 24, c.slot_max_queries * 320u);
            // (-shard targets: the part set's "parts" are the target ranges of the one file, mc_config.target_shard_count)
            if (wantTargets) c.target_shard_count = o.targetShards ? o.targetShards : (uint32_t)std::max<size_t>(o.gpus.size(), 1);
            if (wantKeys) {
                if (mc_keyset_open(o.db.c_str(), &c, o.keyShards, o.gpus.empty() ? nullptr : o.gpus.data(), (uint32_t)o.gpus.size(), &keyset) != MC_OK)
                    throw std::runtime_error(mc_keyset_last_error(nullptr));
            } else if (mc_partset_open(o.db.c_str(), &c, o.residentParts, o.gpus.empty() ? nullptr : o.gpus.data(), (uint32_t)o.gpus.size(), &partset) != MC_OK)
                throw std::runtime_error(mc_partset_last_error(nullptr));
            if (mc_open_metadata(o.db.c_str(), &ctx) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
            read_taxa(ctx, tx);
        } else if (built) {
            // add_to_database_and_query (mode_build_query.cpp:41-77): a query context over the builder's arrays
            for (mc_builder* b : built->bs) if (mc_build_set_query_config(b, &c) != MC_OK) throw std::runtime_error(mc_build_last_error(b));
            if (mc_build_finish_shards(built->bs.data(), (uint32_t)built->bs.size(), &ctx) != MC_OK)
                throw std::runtime_error(mc_build_last_error(built->bs[0]));
            tx.taxa = built->nonTarget;
            tx.taxa.insert(tx.taxa.end(), built->targets.begin(), built->targets.end());
        } else {
            if (mc_open_database(o.db.c_str(), &c, &ctx) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
            for (uint32_t r = 1; r < nrep; ++r) {                                // database::read with replication (database.cpp:207-215)
                mc_config cr = c; cr.device = (int32_t)r;
                mc_ctx* rc = nullptr;
                if (mc_open_database(o.db.c_str(), &cr, &rc) != MC_OK)
                    throw std::runtime_error(std::string("-replicate ") + std::to_string(nrep) + ": GPU " + std::to_string(r) + ": " + mc_last_error(nullptr));
                replicas.push_back(rc);
            }
            read_taxa(ctx, tx);
        }
        cfg = c; db = o.db;
        uint64_t info[8]; mc_db_info(ctx, info);
        dbSketch = (uint32_t)info[1]; dbWinlen = (uint32_t)info[2]; dbStride = (uint32_t)info[3];
        for (size_t i = 0; i < tx.taxa.size(); ++i) {
            tx.byId.emplace(tx.taxa[i].id, (uint32_t)i);
            if (tx.taxa[i].rank == 0 && tx.taxa[i].id < 0) tx.targetByName.emplace(tx.taxa[i].name, (uint32_t)i + 1);
        }
        if (built) {                                                            // ranked lineages of the targets (taxonomy.hpp:576-597)
            const size_t nt = built->targets.size(), base = built->nonTarget.size();
            builtLineages.assign(nt * kNumRanks, 0);
            for (size_t t = 0; t < nt; ++t) {
                const Lineage l = tx.ranks_of((uint32_t)(base + t) + 1);
                std::copy(l.begin(), l.end(), builtLineages.begin() + t * kNumRanks);
            }
            if (mc_set_lineages(ctx, builtLineages.data(), nt) != MC_OK) throw std::runtime_error(mc_last_error(ctx));
        }
        mc_db_lineages(ctx, &tx.targetLineages, &tx.numTargets);
        tx.build_covered();
    }
};

// process_input_files (querying.cpp:40-128): parameters, table layout, mappings of all given files, summary -> one output
// merge mode (mode_merge.cpp): the candidates come from result files instead of the database
struct MergedInput {
    std::vector<std::string> files, headers; std::vector<std::vector<Cand>> cands;
    std::vector<mc_assignment> assigned;     // MCQ_MERGE_DEVICE: the library's vote over cands (empty: the host classifies)
};

// ---- per-query statistics: classification_statistics (classification_statistics.hpp), queries per taxon, matches per target ----------
struct Cover { uint32_t tgt; uint64_t qid; uint32_t beg, end, hits; };

struct Tally {
    uint64_t assigned[kNumRanks + 1] = {}, known[kNumRanks + 1] = {}, correct[kNumRanks + 1] = {}, wrong[kNumRanks + 1] = {};
    uint64_t covFalsePos[kNumRanks + 1] = {}, covDomain = 0;
    std::map<uint32_t, double> counts;                                      // taxon (index + 1) -> queries classified as it
    std::vector<Cover> covers;                                              // matches_per_target
    Tally& operator+=(const Tally& t)
    {
        for (int r = 0; r <= kNumRanks; ++r) { assigned[r] += t.assigned[r]; known[r] += t.known[r]; correct[r] += t.correct[r]; wrong[r] += t.wrong[r]; covFalsePos[r] += t.covFalsePos[r]; }
        covDomain += t.covDomain;
        for (const auto& kv : t.counts) counts[kv.first] += kv.second;
        covers.insert(covers.end(), t.covers.begin(), t.covers.end());
        return *this;
    }
    uint64_t classified() const { uint64_t n = 0; for (int r = 0; r < kNumRanks; ++r) n += assigned[r]; return n; }
    uint64_t unclassified() const { return assigned[kNumRanks]; }
    uint64_t total() const { return classified() + unclassified(); }
};

struct Deferred { uint64_t id; View header; std::vector<Cand> cands; size_t q; };   // (q: the query's place in its batch, BatchQueue::read)
struct ResidentFile;
struct Batch {
    size_t f1, f2; size_t qBeg, qEnd; uint64_t idBase; std::string prefix; const std::vector<uint64_t>* sel; bool halfLast;
    std::vector<Deferred> deferred;                                         // -cov-percentile: its reads' candidates
    std::vector<mc_candidate> carried;                                      // part groups: its reads' candidate lists from the groups so far
    // MCQ_INPUT_DEVICE: the batch is a range of a file that is resident on the device (no SeqFile behind f1); records: what the cut counted
    ResidentFile* res = nullptr; const char* dev = nullptr; uint64_t devBytes = 0; uint32_t devRecords = 0; bool tooBig = false;
};
struct Profile {                                                            // MCQ_PROFILE: phase times on stderr (development aid)
    const bool on = std::getenv("MCQ_PROFILE") != nullptr;
    std::atomic<uint64_t> parse{0}, submit{0}, wait{0}, classify{0};
};

#include "mcq_device_steps.h"

// -align: where a batch's text gets alignment lines (behind a mapping line's taxon text, before its '\n'), for which query of the
// batch, against which candidate; the Aligner below turns these into problems for the device and into lines
struct AlignWant { size_t at, q; Cand c; };
inline size_t out_pos(const FastOut& o) { return o.s.size(); }
inline size_t out_pos(std::ostringstream& o) { return (size_t)o.tellp(); }

// ---- one query: classification, statistics, mapping line (classify_and_evaluate, classification.cpp:470-559) ------------------------
struct MappingWriter {
    const Options& o; const Taxonomy& tx; const uint32_t stride, winlen;
    const bool deferred;                     // -cov-percentile: the workers keep the candidates, the lines come after the coverage filter
    Tally& tally;
    // the text show_taxon writes for a classification (taxon, or target for sequence-level results): the same few thousand over and
    // over -- its lineage walk (hash lookups up the taxonomy, taxonomy.hpp:576-597) is done once per worker and taxon
    std::unordered_map<uint64_t, std::string> taxText = {};
    std::vector<AlignWant>* wants = nullptr;    // -align: the printed lines of classified reads ask for their alignment here
    HitsClient hits = {};                       // -hits-per-ref: the batch's candidates go to the library's log instead of tally.covers
    EvalClient eval = {};                       // -precision: the batch's (assigned, truth) pairs go to the library instead of tally.known / correct / wrong
    FormatClient fmt = {};                      // MCQ_FORMAT_DEVICE: the batch's lines come from the library (FormatClient::lines) instead of operator()

    // evaluate_classification + update_coverage_statistics (classification.cpp:237-295) for one read on the host
    void count_truth(uint32_t best, uint32_t truth)
    {
        const int bestRank = best ? tx.taxon(best)->rank : kNumRanks;
        const int knownRank = truth ? tx.taxon(truth)->rank : kNumRanks;
        int correctRank = kNumRanks;                         // rank of the ranked LCA of mapping and truth
        if (best && truth) {
            const Lineage la = tx.ranks_of(best), lb = tx.ranks_of(truth);
            for (int r = 0; r < kNumRanks; ++r) if (la[r] && la[r] == lb[r]) { correctRank = tx.taxon(la[r])->rank; break; }
        }
        // assign_known_correct (classification_statistics.hpp:86-106)
        if (correctRank < bestRank) correctRank = bestRank;
        if (correctRank < knownRank) correctRank = knownRank;
        ++tally.known[knownRank];
        if (knownRank != kNumRanks) {
            ++tally.correct[correctRank];
            if (correctRank > knownRank && correctRank > bestRank) ++tally.wrong[correctRank - 1];
        }
        if (o.taxonCoverage && truth) {                       // update_coverage_statistics, classification.cpp:242-265
            for (uint32_t t : tx.ranks_of(truth)) {
                if (!t) continue;
                const int r = tx.taxon(t)->rank;
                const bool classifiedOnRank = best && r >= bestRank;
                if (!tx.covers(t) && classifiedOnRank) ++tally.covFalsePos[r];
                if (r == 19) ++tally.covDomain;
            }
        }
    }

    // the end of a batch: what its reads gathered for the library goes there, the pairs first, then the candidates
    void flush() { eval.flush(o, [&](uint32_t best, uint32_t truth) { count_truth(best, truth); }); hits.flush(o, tx, tally.covers); }

    // One read's statistics from its assignment (taxon, rank) and its candidates, counted here or gathered for the library
    void count_read(uint64_t id, mc_assignment a, uint32_t truth, const std::vector<Cand>& cands)
    {
        ++tally.assigned[a.info & 0xFFu];
        if (o.precision) { if (eval.step) eval.add(a, truth); else count_truth(a.taxon, truth); }    // evaluate_classification, classification.cpp:272-295
        if ((o.abundances || o.abundancePer != kNumRanks) && a.taxon) ++tally.counts[a.taxon];       // classify_and_evaluate, classification.cpp:552-554
        if (o.hitsPerRef && !deferred) {                         // matches_per_target::insert (records_match)
            if (hits.step) hits.add(id, cands);
            else for (const Cand& c : cands) if (records_match(c.tax, c.hits, o)) tally.covers.push_back(Cover{c.tgt, id, c.beg, c.end, c.hits});
        }
    }

    template <class OS>
    void operator()(OS& out, uint64_t id, View header, const std::vector<Cand>& cands, const mc_location* hits, uint64_t nhits, size_t q = 0, const mc_assignment* given = nullptr)
    {
        bool isTarget = false; uint32_t tgt = 0;
        // a merged query's assignment may come from the library; sequence-level results (rank 0) go through the host's rule for isTarget
        const uint32_t best = (given && (given->info & 0xFFu) != 0) ? given->taxon : classify(o, tx, cands, isTarget, tgt);
        const int bestRank = best ? tx.taxon(best)->rank : kNumRanks;
        uint32_t truth = 0;
        if (o.determineGroundTruth) truth = ground_truth(tx, std::string(header.p, header.n));
        count_read(id, mc_assignment{best, (uint32_t)bestRank}, truth, cands);
        if (o.mapView == Options::mv_none || (o.mapView == Options::mv_mapped && !best)) return;
        if (o.queryIds) out << id << o.column;
        const void* sp = memchr(header.p, ' ', header.n);
        out.write(header.p, sp ? (const char*)sp - header.p : (std::streamsize)header.n);
        out << o.column;
        if (o.showGroundTruth) { show_taxon(out, o, tx, truth, false, 0); out << o.column; }
        if (o.allhits) { if (hits) show_matches(out, o, tx, hits, nhits); out << o.column; }
        if (o.tophits) { show_candidates(out, o, tx, cands); out << o.column; }
        if (o.locations) {                                       // show_candidate_ranges, printing.cpp:370-380
            for (const Cand& c : cands) out << '[' << (uint64_t)stride * c.beg << ',' << (uint64_t)stride * c.end + winlen << "] ";
            out << o.column;
        }
        {
            const uint64_t key = isTarget ? ((1ull << 32) | tgt) : (uint64_t)best;
            auto it = taxText.find(key);
            if (it == taxText.end()) {
                FastOut t;
                show_taxon(t, o, tx, best, isTarget, tgt);
                it = taxText.emplace(key, std::move(t.s)).first;
            }
            out << it->second;
        }
        if (wants && best && !cands.empty()) wants->push_back(AlignWant{out_pos(out), q, cands[0]});   // show_query_mapping, classification.cpp:521-523
        out << '\n';
    }
};

// fn(0) on the calling thread, fn(1) .. fn(n - 1) on threads of their own; back when all are through
template <class Fn>
void run_workers(unsigned n, Fn&& fn)
{
    std::vector<std::thread> pool;
    for (unsigned w = 1; w < n; ++w) pool.emplace_back(fn, w);
    fn(0);
    for (auto& t : pool) t.join();
}

// ---- the batches: runs of consecutive queries of one file (pair of files), ids continuing across files -----------------------------
// Batches are produced while the workers already run: plain files are indexed chunk by chunk (SeqFile::stream_*), and a batch goes out
// as soon as its records are known -- the first one after a few megabytes instead of after the whole file.
struct Records { View h1, s1, h2, s2; std::string scratch1, scratch2; };    // one query's records (scratch: multi-line sequences)

struct BatchQueue {
    const Options& o; const unsigned workers; const std::chrono::steady_clock::time_point t0;
    std::vector<std::unique_ptr<SeqFile>> files;
    const GzInflater* inflater = nullptr;                                   // MCQ_INFLATE_DEVICE: who takes a compressed query file before SeqFile's own loop
    InputStep* input = nullptr;                                             // MCQ_INPUT_DEVICE: who makes a query file resident on the device before anything else looks at it
    std::vector<std::unique_ptr<std::vector<uint64_t>>> selections;
    std::deque<Batch> batches;                                              // grows at the back only: references stay valid
    std::mutex mu; std::condition_variable cv;
    size_t next = 0; bool producing = true;                                 // (under mu)
    std::atomic<bool> stopped{false}; std::string producerError, firstError;
    double tIndexed = 0; std::thread producer;

    BatchQueue(const Options& o, unsigned workers, std::chrono::steady_clock::time_point t0) : o(o), workers(workers), t0(t0) {}
    void start()
    {
        files.reserve(o.infiles.size() + 2);                                // workers read files[...] while the producer appends
        producer = std::thread([this] { produce(); });
    }
    void finish() { { std::lock_guard<std::mutex> l(mu); } cv.notify_all(); producer.join(); }
    // the next batch, or false when none is left (or the job has failed)
    bool take(size_t& b, Batch*& B)
    {
        std::unique_lock<std::mutex> l(mu);
        cv.wait(l, [&] { return stopped || next < batches.size() || !producing; });
        if (stopped || next >= batches.size()) return false;
        b = next++;
        B = &batches[b];                                                    // (under the lock: operator[] walks the deque's map, which push_back may reallocate)
        return true;
    }
    void rewind() { std::lock_guard<std::mutex> l(mu); next = 0; }          // the next part group's pass
    void fail(const std::string& m) { std::lock_guard<std::mutex> l(mu); if (!stopped.exchange(true)) firstError = m; }
    bool failed() const { return stopped; }
    void rethrow() const { if (!producerError.empty()) throw std::runtime_error(producerError); if (stopped) throw std::runtime_error(firstError); }
    // One query's records by pairing mode and its id: the reader's index after the read (database_query.hpp:264); a last pair without its
    // second sequence does not advance the index (sequence_io.cpp:312-318), so it shares the id of the pair before it
    uint64_t read(const Batch& B, size_t q, Records& r) const
    {
        const size_t qi = B.sel ? (size_t)(*B.sel)[q] : q;                  // query index inside the file (pair)
        const bool halfPair = B.halfLast && q + 1 == B.qEnd;
        r.h2 = r.s2 = View{};
        if (o.pairing == Options::sequences) {
            files[B.f1]->record(2 * qi, r.h1, r.s1, r.scratch1);
            if (!halfPair) files[B.f1]->record(2 * qi + 1, r.h2, r.s2, r.scratch2);
        } else {
            files[B.f1]->record(qi, r.h1, r.s1, r.scratch1);
            if (o.pairing == Options::files) files[B.f2]->record(qi, r.h2, r.s2, r.scratch2);
        }
        return B.idBase + qi + (halfPair ? 0 : 1);
    }

    void push(size_t f1, size_t f2, size_t qBeg, size_t qEnd, uint64_t idBase, const std::string& prefix, const std::vector<uint64_t>* sel, bool halfLast)
    {
        { std::lock_guard<std::mutex> l(mu); batches.push_back(Batch{f1, f2, qBeg, qEnd, idBase, prefix, sel, halfLast, {}, {}}); }
        cv.notify_all();
    }
    void produce()
    {
        const bool lengthFilter = o.minReadLen > 0 || o.maxReadLen < std::numeric_limits<uint64_t>::max();
        try {
            uint64_t idOffset = 0;
            const size_t stride = o.pairing == Options::files ? 2 : 1;
            for (size_t fi = 0; fi < o.infiles.size(); fi += stride) {
                if (o.pairing == Options::files && fi + 1 >= o.infiles.size()) break;
                std::string prefix = o.comment + o.infiles[fi];                  // appendToOutput, classification.cpp:825-827
                if (o.pairing == Options::files) prefix += " + " + o.infiles[fi + 1];
                prefix += '\n';
                size_t nq = 0, f1 = files.size(), f2 = files.size();
                std::vector<char> inflated;                                      // MCQ_INPUT_DEVICE: the file's bytes where the device inflated it and then refused it
                if (input && input->ctx) {
                    ResidentFile* rf = nullptr;
                    std::vector<mc_input_batch> rows;
                    if (input->take(o.infiles[fi], stopped, rf, rows, inflated)) {
                        files.emplace_back(nullptr);                             // (the file's place: its batches need no SeqFile)
                        const size_t per = o.pairing == Options::sequences ? 2 : 1;
                        size_t q = 0; uint64_t recs = 0;
                        for (size_t i = 0; i < rows.size(); ++i) {
                            Batch B{f1, f2, q, q + rows[i].queries, idOffset, i == 0 ? prefix : std::string(), nullptr, rows[i].half_pair != 0, {}, {}};
                            B.res = rf; B.dev = rf->dev + rows[i].offset; B.devBytes = rows[i].nbytes; B.devRecords = rows[i].records; B.tooBig = rows[i].too_big != 0;
                            { std::lock_guard<std::mutex> l(mu); batches.push_back(std::move(B)); }
                            cv.notify_all();
                            q += rows[i].queries; recs += rows[i].records;
                        }
                        size_t nread = q;
                        if (per == 2 && q > 0 && (recs & 1u)) --nread;           // (the half pair did not count)
                        idOffset += nread;
                        continue;
                    }
                    if (stopped) break;
                }
                const GzInflater once = [&inflated](const std::string&, const unsigned char*, size_t, std::vector<char>& out, size_t& size) { out.swap(inflated); size = out.size(); return true; };
                const GzInflater* const inflater = inflated.empty() ? this->inflater : &once;
                try {
                    files.emplace_back(new SeqFile(o.infiles[fi], inflater));
                    SeqFile& F = *files.back();
                    if (F.can_stream() && o.pairing != Options::files && !lengthFilter && o.queryLimit >= (int64_t)1 << 62 && !std::getenv("MCQ_NO_STREAM")) {
                        // streaming: batches of this file go out while its later chunks are still being indexed
                        const size_t per = o.pairing == Options::sequences ? 2 : 1;
                        F.stream_begin(std::max(1u, std::min(workers, 16u)));
                        size_t q = 0;
                        bool first = true;
                        for (;;) {
                            const size_t readable = F.stream_wait((q + o.batchSize) * per);
                            const bool done = F.stream_done();
                            const size_t qAvail = done ? (F.records() + per - 1) / per : readable / per;
                            while (q + o.batchSize <= qAvail || (done && q < qAvail)) {
                                const size_t qe = std::min(qAvail, q + o.batchSize);
                                const bool half = done && per == 2 && qe == qAvail && (F.records() & 1u);
                                push(f1, f2, q, qe, idOffset, first ? prefix : std::string(), nullptr, half);
                                first = false; q = qe;
                            }
                            if (done) break;
                        }
                        F.stream_end();
                        if (first) push(f1, f2, 0, 0, idOffset, prefix, nullptr, false);             // no records: the file's comment line only
                        nq = (F.records() + per - 1) / per;
                        size_t nread = nq;
                        if (per == 2 && nq > 0 && (F.records() & 1u)) --nread;                       // (the half pair did not count)
                        idOffset += nread;
                        continue;
                    }
                    files.back()->index(workers);
                    nq = files.back()->records();
                    if (o.pairing == Options::sequences) nq = (nq + 1) / 2;
                    if (o.pairing == Options::files) {
                        f2 = files.size();
                        files.emplace_back(new SeqFile(o.infiles[fi + 1], inflater));
                        files.back()->index(workers);
                        nq = std::min(nq, files.back()->records());
                    }
                } catch (std::exception& e) { if (o.showErrors) std::cerr << "FAIL: " << e.what() << '\n'; nq = 0; }   // database_query.hpp:397-399
                // query_batched (database_query.hpp:258-284): at most -query-limit queries per file; with a read length filter a
                // query that fails it is replaced by the next record -- except when the file ends there
                const std::vector<uint64_t>* sel = nullptr;
                size_t nsel = std::min<uint64_t>(nq, (uint64_t)o.queryLimit), nread = nsel;
                if (lengthFilter && nq > 0) {
                    std::vector<uint32_t> len(nq);
                    const size_t per = (nq + workers - 1) / workers;
                    run_workers(workers, [&](unsigned t) {
                        View h, sq; std::string scratch;
                        for (size_t q = t * per; q < std::min(nq, (t + 1) * per); ++q) {
                            files[f1]->record(o.pairing == Options::sequences ? 2 * q : q, h, sq, scratch);
                            len[q] = (uint32_t)std::min<size_t>(sq.n, 0xFFFFFFFFu);
                        }
                    });
                    auto fails = [&](size_t q) { return len[q] < o.minReadLen || len[q] > o.maxReadLen; };
                    selections.emplace_back(new std::vector<uint64_t>());
                    auto& kept = *selections.back();
                    size_t q = 0;
                    for (int64_t limit = o.queryLimit; q < nq && limit >= 1; --limit) {
                        size_t cur = q++;
                        while (fails(cur)) { if (q >= nq) break; cur = q++; }
                        kept.push_back(cur);
                    }
                    nread = q; nsel = kept.size(); sel = &kept;
                }
                const bool oddFile = o.pairing == Options::sequences && nq > 0 && (files[f1]->records() & 1u);
                for (size_t q = 0; q == 0 || q < nsel; q += o.batchSize) {
                    const size_t qe = std::min<size_t>(nsel, q + o.batchSize);
                    // the file's last query is a half pair: when it is among the selected ones, it is the last of them
                    const bool half = oddFile && qe == nsel && nsel > 0 && (sel ? (*sel)[nsel - 1] : nsel - 1) == nq - 1;
                    push(f1, f2, q, qe, idOffset, q == 0 ? prefix : std::string(), sel, half);
                    if (nsel == 0) break;
                }
                if (oddFile && nread == nq) --nread;                             // (the half pair did not count)
                idOffset += nread;                                               // reader.index(): records (pairs) consumed
            }
        } catch (std::exception& e) { std::lock_guard<std::mutex> l(mu); producerError = e.what(); }
        tIndexed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        { std::lock_guard<std::mutex> l(mu); producing = false; }
        cv.notify_all();
    }
};

// ---- -align (show_alignment, classification.cpp:384-426) ---------------------------------------------------------------------------
// The target records a run aligns to, by file name and record number: loaded through SeqFile on first use and kept for the run (the
// reference opens the file again for every read); a file that cannot be read is remembered as such.
struct TargetCache {
    const bool showErrors;
    std::mutex mu;
    std::map<std::string, std::unique_ptr<SeqFile>> files;                  // (null: could not be read)
    std::map<std::pair<std::string, uint64_t>, std::unique_ptr<std::string>> recs;   // (null: no such record)
    explicit TargetCache(bool showErrors) : showErrors(showErrors) {}
    const std::string* get(const std::string& file, uint64_t index)
    {
        std::lock_guard<std::mutex> l(mu);
        const auto key = std::make_pair(file, index);
        auto it = recs.find(key);
        if (it != recs.end()) return it->second.get();
        auto f = files.find(file);
        if (f == files.end()) {
            std::unique_ptr<SeqFile> sf;
            try { sf.reset(new SeqFile(file)); sf->index(1); }
            catch (std::exception& e) { if (showErrors) std::cerr << e.what() << '\n'; sf.reset(); }
            f = files.emplace(file, std::move(sf)).first;
        }
        std::unique_ptr<std::string> rec;
        if (f->second && index < f->second->records()) {
            View h, sq; std::string scratch;
            f->second->record((size_t)index, h, sq, scratch);
            rec.reset(new std::string(sq.p, sq.n));
        }
        return recs.emplace(key, std::move(rec)).first->second.get();
    }
};

// One batch's alignments: the lines that asked for one (MappingWriter::wants) become problems -- read 1, its mate, the candidate's window
// range cut out of the target's record (make_view_from_window_range, classification.cpp:56-65) -- for ONE mc_align_semiglobal call, and
// the three lines per read are put into the batch's text.  The target's record is number srcIndex of its file, counted from 0 as the
// database stores it (the reference reads the record before it: DESIGN.md 7a).
struct Aligner {
    mc_ctx* const ctx; const Options& o; const Taxonomy& tx; TargetCache& cache; const BatchQueue& Q; const uint64_t stride, winlen;
    std::vector<AlignWant> wants = {};
    struct Job { size_t at; const Taxon* t; uint32_t beg, end; };
    std::vector<Job> jobs = {};
    std::string reads = {}, mates = {}, subjects = {}, aligned = {}, spliced = {};
    std::vector<uint64_t> roff = {}, moff = {}, soff = {}, aoff = {};
    std::vector<int32_t> sc[4] = {};
    std::vector<uint8_t> rev = {};
    Records rec = {};
    bool noReads = false;       // -cov-percentile: the reference keeps id, header and candidates of a read for the pass after the coverage filter, not its
                                // sequences (classification.cpp:790-799), and so aligns an EMPTY query there: score 0, one column of gaps.  Kept as it is.

    // false: the device call failed (err)
    bool finish(const Batch& B, std::string& text, std::string& err)
    {
        jobs.clear(); reads.clear(); mates.clear(); subjects.clear(); roff.assign(1, 0); moff.assign(1, 0); soff.assign(1, 0);
        uint64_t cap = 0;
        for (const AlignWant& w : wants) {
            const Taxon* t = tx.taxon(w.c.tax);
            if (!t || t->rank != 0) continue;                               // candidates above sequence level (-lowest): nothing to align to
            const std::string* target = cache.get(t->srcFile, t->srcIndex);
            if (!target) continue;
            const uint64_t sb = std::min<uint64_t>(stride * w.c.beg, target->size()), se = std::max(sb, std::min<uint64_t>(stride * w.c.end + winlen, target->size()));
            if (noReads) rec = Records{}; else Q.read(B, w.q, rec);
            reads.append(rec.s1.p, rec.s1.n); roff.push_back(reads.size());
            mates.append(rec.s2.p, rec.s2.n); moff.push_back(mates.size());
            subjects.append(*target, (size_t)sb, (size_t)(se - sb)); soff.push_back(subjects.size());
            cap += 2 * std::max<uint64_t>(1, rec.s1.n + (se - sb));
            jobs.push_back(Job{w.at, t, w.c.beg, w.c.end});
        }
        wants.clear();
        const size_t n = jobs.size();
        if (n == 0) return true;
        for (auto& v : sc) v.resize(n);
        rev.resize(n); aoff.resize(n + 1); aligned.resize(cap);
        if (mc_align_semiglobal(ctx, reads.data(), roff.data(), mates.empty() ? nullptr : mates.data(), moff.data(), subjects.data(), soff.data(), n,
                                sc[0].data(), sc[1].data(), sc[2].data(), sc[3].data(), rev.data(), &aligned[0], cap, aoff.data()) != MC_OK) {
            err = mc_last_error(ctx);
            return false;
        }
        FastOut out;
        out.s.swap(spliced); out.s.clear();
        size_t from = 0;
        for (size_t j = 0; j < n; ++j) {
            const Job& J = jobs[j];
            out.write(text.data() + from, (std::streamsize)(J.at - from)); from = J.at;
            const uint64_t half = (aoff[j + 1] - aoff[j]) / 2;
            out << '\n' << o.comment << "  score  " << (rev[j] ? sc[1][j] : sc[0][j]) << "  aligned to " << J.t->srcFile << " #" << J.t->srcIndex
                << " in range [" << stride * J.beg << ',' << stride * J.end + stride << "]\n" << o.comment << "  query  ";
            out.write(aligned.data() + aoff[j], (std::streamsize)half);
            out << '\n' << o.comment << "  target ";
            out.write(aligned.data() + aoff[j] + half, (std::streamsize)half);
        }
        out.write(text.data() + from, (std::streamsize)(text.size() - from));
        text.swap(out.s);
        spliced.swap(out.s);
        return true;
    }
};

// ---- the mapping lines of the batches, in batch order ---------------------------------------------------------------------------
// Output file: the batches' texts go out in batch order, but not one after the other -- under the lock a finished batch only gets its
// place in the file (the sizes of the batches before it are known then); the bytes are written by the worker that formatted them,
// side by side with the others' (pwrite).  10^7 lines of `-tophits -queryids` are 1.1 GB: one thread copying them into the page cache
// was a quarter of a second of a 0.3 s query phase.  (No file: std::cout, in order.)
struct OrderedOut {
    std::ostream& os; std::ofstream& fout; const std::string name;
    int fd = -1; uint64_t off = 0;                                          // where the next batch goes (under mu)
    std::mutex mu; std::map<size_t, std::string> finished; size_t next = 0;
    std::vector<std::string> pool;                                          // written batches' buffers, for the next batches (a fresh 7 MB buffer per batch is 1 700 page faults)

    OrderedOut(std::ostream& os, std::ofstream& fout, const std::string& name) : os(os), fout(fout), name(name)
    {
        if (name.empty()) return;
        const std::streamoff at = fout.flush().tellp();
        if (at >= 0) { fd = ::open(name.c_str(), O_WRONLY); off = (uint64_t)at; }
    }
    void take_buffer(std::string& into)
    {
        std::lock_guard<std::mutex> l(mu);
        if (!pool.empty()) { into = std::move(pool.back()); pool.pop_back(); into.clear(); }
    }
    // batch b's text; false when the file could not be written
    bool deliver(size_t b, std::string&& text)
    {
        std::vector<std::pair<uint64_t, std::string>> mine;
        {
            std::lock_guard<std::mutex> l(mu);
            finished.emplace(b, std::move(text));
            for (auto it = finished.begin(); it != finished.end() && it->first == next; it = finished.erase(it), ++next) {
                if (fd >= 0) { const uint64_t n = it->second.size(); mine.emplace_back(off, std::move(it->second)); off += n; }
                else os.write(it->second.data(), (std::streamsize)it->second.size());
            }
        }
        bool ok = true;
        for (auto& m : mine) {
            const char* p = m.second.data();
            uint64_t left = m.second.size(), at = m.first;
            while (left) {
                const ssize_t w = ::pwrite(fd, p, (size_t)std::min<uint64_t>(left, 1ull << 30), (off_t)at);
                if (w <= 0) { ok = false; break; }
                p += w; left -= (uint64_t)w; at += (uint64_t)w;
            }
            m.second.clear();
            std::lock_guard<std::mutex> l(mu);
            if (pool.size() < 64) pool.push_back(std::move(m.second));
        }
        return ok;
    }
    void close() { if (fd >= 0) { ::close(fd); fout.seekp((std::streamoff)off); } }   // (the stream goes on behind the batches' lines)
};

// ---- the device steps: a batch's queries in, their candidate lists out (emit(queries, results) once or more) ----------------------
struct Query { uint64_t id; View header; bool empty; uint64_t len; size_t q; };   // (q: its place in the batch, BatchQueue::read)

uint64_t now_ns() { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// maxWindowsInRange (candidate_structs.hpp:143-145)
uint32_t max_windows(uint64_t len, uint64_t insertMax, uint32_t stride) { return (uint32_t)(2 + std::max<uint64_t>(len, insertMax) / stride); }

// The slot path: the worker's own batch slot on one replica (worker w: replica w % n, slot w / n).  A batch goes through it in as many
// rounds as the slot needs: parse -> mc_batch_add -> submit -> wait -> emit -> clear.
struct SlotStep {
    const Session& S; const Options& o; BatchQueue& Q; Profile& P; mc_ctx* const ctx; const unsigned slot;
    const bool prints = true;
    std::vector<Query> queries = {}; Records rec = {};
    ParseStep* parse = nullptr;                                             // MCQ_PARSE_DEVICE: the batch's byte range goes to the slot, the library cuts it
    InputStep* input = nullptr;                                             // MCQ_INPUT_DEVICE: batches of resident files are device ranges already

    // a batch of a resident file: mc_batch_add_device_bytes -> submit -> wait -> mc_batch_records + mc_batch_headers -> emit -> clear.  A record
    // count that differs from the cut's is an error of the run, not a fall-back.  false: the job has failed
    template <class Emit>
    bool resident(Batch& B, Emit&& emit)
    {
        struct Done { InputStep* in; ResidentFile* r; ~Done() { in->done(r); } } done{input, B.res};   // (behind the clear: the range stays untouched until then)
        if (B.tooBig) { std::cerr << "query batch is too small for a single read!\n"; return true; }    // database_query.hpp:103
        const size_t per = o.pairing == Options::sequences ? 2 : 1;
        const uint64_t tp0 = now_ns();
        const int rc = mc_batch_add_device_bytes(ctx, slot, B.dev, B.devBytes, input->flags, o.insertMax);
        if (rc != MC_OK) { Q.fail(rc == MC_BATCH_FULL ? "resident input: a batch exceeds the slot it was cut for" : mc_last_error(ctx)); return false; }
        mc_results r;
        mc_batch_record_info info;
        const char* text = nullptr; const uint64_t* off = nullptr; uint64_t nheaders = 0;
        const uint64_t tp1 = now_ns();
        if (mc_batch_submit(ctx, slot, o.lowest) != MC_OK) { Q.fail(mc_last_error(ctx)); mc_batch_clear(ctx, slot); return false; }
        const uint64_t tp2 = now_ns();
        if (mc_batch_wait(ctx, slot, &r) != MC_OK || mc_batch_records(ctx, slot, &info) != MC_OK || mc_batch_headers(ctx, slot, &text, &off, &nheaders) != MC_OK) {
            Q.fail(mc_last_error(ctx)); mc_batch_clear(ctx, slot); return false;
        }
        const uint64_t tp3 = now_ns();
        if (info.verdict == MC_PARSE_OVERFLOW && B.qEnd - B.qBeg == 1) {      // one read (pair) beyond what a slot's kernels take
            mc_batch_clear(ctx, slot);
            std::cerr << "query batch is too small for a single read!\n";
            return true;
        }
        if (info.verdict != MC_PARSE_OK || info.records != B.devRecords || r.num_queries != B.qEnd - B.qBeg || nheaders != info.records || !off) {
            Q.fail("resident input: the device parse gives verdict " + std::to_string(info.verdict) + " and " + std::to_string(info.records) + " records, the cut " + std::to_string(B.devRecords));
            mc_batch_clear(ctx, slot);
            return false;
        }
        queries.clear();
        for (size_t q = B.qBeg; q < B.qEnd; ++q) {
            const size_t i = q - B.qBeg, rr = i * per;
            const bool halfPair = B.halfLast && q + 1 == B.qEnd;
            const View h{text + off[rr], (size_t)(off[rr + 1] - off[rr])};
            const uint64_t l1 = info.qinfo[4 * i + 1], l2 = info.qinfo[4 * i + 3];
            queries.push_back(Query{B.idBase + q + (halfPair ? 0 : 1), h, h.empty() || l1 == 0, l1 + l2, q});
        }
        emit(queries, r);
        mc_batch_clear(ctx, slot);
        if (P.on) { P.parse += tp1 - tp0; P.submit += tp2 - tp1; P.wait += tp3 - tp2; P.classify += now_ns() - tp3; }
        return true;
    }

    // the whole batch through mc_batch_add_file_bytes.  true: it was emitted; false: nothing was, and the host loop takes it (or the job has failed)
    template <class Emit>
    bool parsed_on_device(Batch& B, Emit&& emit)
    {
        const bool mates = o.pairing == Options::files;                       // (MCQ_PARSE_DEVICE=2: record q of each file, mc_batch_add_file_mates)
        const size_t per = o.pairing == Options::sequences ? 2 : 1;
        if (B.sel || B.qEnd <= B.qBeg) return false;
        const size_t r0 = B.qBeg * per, r1 = B.qEnd * per - (B.halfLast ? 1 : 0);
        const char* base = nullptr; size_t b = 0, e = 0;
        const char* base2 = nullptr; size_t b2 = 0, e2 = 0;
        if (!Q.files[B.f1]->byte_range(r0, r1, base, b, e) || (mates && !Q.files[B.f2]->byte_range(r0, r1, base2, b2, e2))) { parse->note("its records come from the exact reader"); return false; }
        const uint64_t tp0 = now_ns();
        const int rc = mates ? mc_batch_add_file_mates(ctx, slot, base + b, e - b, base2 + b2, e2 - b2, o.insertMax)
                             : mc_batch_add_file_bytes(ctx, slot, base + b, e - b, parse->flags, o.insertMax);
        if (rc == MC_BATCH_FULL) { parse->note("its bytes exceed the slot's character capacity"); return false; }
        if (rc < 0) { Q.fail(mc_last_error(ctx)); return false; }
        mc_results r;
        mc_batch_record_info info;
        const uint64_t tp1 = now_ns();
        if (mc_batch_submit(ctx, slot, o.lowest) != MC_OK) { Q.fail(mc_last_error(ctx)); mc_batch_clear(ctx, slot); return false; }
        const uint64_t tp2 = now_ns();
        if (mc_batch_wait(ctx, slot, &r) != MC_OK || mc_batch_records(ctx, slot, &info) != MC_OK) { Q.fail(mc_last_error(ctx)); mc_batch_clear(ctx, slot); return false; }
        const uint64_t tp3 = now_ns();
        std::string why;
        const size_t indexed = mates ? 2 * (r1 - r0) : r1 - r0;
        if (info.verdict == MC_PARSE_IRREGULAR) why = mates ? "irregular at byte " + std::to_string(info.offence) + " of one of the two ranges" : "irregular at byte " + std::to_string(b + info.offence);
        else if (info.verdict == MC_PARSE_UNEQUAL) why = "the device counts different numbers of records in the two files' ranges";
        else if (info.verdict != MC_PARSE_OK) why = "more reads or characters than the slot takes";
        else if (info.records != indexed || r.num_queries != B.qEnd - B.qBeg) why = "the device counts " + std::to_string(info.records) + " records, the index " + std::to_string(indexed);
        if (!why.empty()) { mc_batch_clear(ctx, slot); parse->note(why); return false; }
        queries.clear();
        for (size_t q = B.qBeg; q < B.qEnd; ++q) {
            const size_t i = q - B.qBeg, rr = i * (mates ? 2 : per);          // (mates: row 2i is the first mate's header, a place in the first file's range)
            const bool halfPair = B.halfLast && q + 1 == B.qEnd;
            const View h{base + b + info.hdr[2 * rr], info.hdr[2 * rr + 1]};
            const uint64_t l1 = info.qinfo[4 * i + 1], l2 = info.qinfo[4 * i + 3];
            queries.push_back(Query{B.idBase + q + (halfPair ? 0 : 1), h, h.empty() || l1 == 0, l1 + l2, q});
        }
        emit(queries, r);
        mc_batch_clear(ctx, slot);
        parse->took((e - b) + (e2 - b2), info.records);
        if (P.on) { P.parse += tp1 - tp0; P.submit += tp2 - tp1; P.wait += tp3 - tp2; P.classify += now_ns() - tp3; }
        return true;
    }

    template <class Emit>
    bool operator()(Batch& B, Emit&& emit)
    {
        if (B.res) return resident(B, emit);
        if (parse && parse->ctx) {
            if (parsed_on_device(B, emit)) return true;
            if (Q.failed()) return false;
        }
        for (size_t q = B.qBeg; q < B.qEnd;) {
            if (Q.failed()) return false;
            queries.clear();
            const uint64_t tp0 = now_ns();
            for (; q < B.qEnd; ++q) {
                const uint64_t id = Q.read(B, q, rec);
                if (std::max(rec.s1.n, rec.s2.n) >= 0xFFFFFFF0ull) { Q.fail("sequence too long"); return false; }
                const uint64_t len = (uint64_t)rec.s1.n + rec.s2.n;
                const bool tooBig = len + 8 > S.cfg.slot_max_chars;
                const int rc = tooBig ? MC_BATCH_FULL : mc_batch_add(ctx, slot, rec.s1.p, (uint32_t)rec.s1.n, rec.s2.p, (uint32_t)rec.s2.n, max_windows(len, o.insertMax, S.dbStride));
                if (rc == MC_BATCH_FULL) {
                    if (!tooBig && !queries.empty()) break;                   // submit what is there, then retry this query
                    std::cerr << "query batch is too small for a single read!\n";                                    // database_query.hpp:103
                    continue;
                }
                if (rc < 0) { Q.fail(mc_last_error(ctx)); return false; }
                queries.push_back(Query{id, rec.h1, rec.h1.empty() || rec.s1.empty(), len, q});
            }
            if (Q.failed()) return false;
            mc_results r;
            const uint64_t tp1 = now_ns();
            if (mc_batch_submit(ctx, slot, o.lowest) != MC_OK) { Q.fail(mc_last_error(ctx)); return false; }
            const uint64_t tp2 = now_ns();
            if (mc_batch_wait(ctx, slot, &r) != MC_OK) { Q.fail(mc_last_error(ctx)); return false; }
            const uint64_t tp3 = now_ns();
            emit(queries, r);
            mc_batch_clear(ctx, slot);
            if (P.on) { P.parse += tp1 - tp0; P.submit += tp2 - tp1; P.wait += tp3 - tp2; P.classify += now_ns() - tp3; }
        }
        return true;
    }
};

// The set path (-shard keys / -resident-parts / -gpus): a batch's records are packed and go to mc_keyset_classify or
// mc_partset_classify_resident in one call.  The sets share their two device lanes among the callers: this worker's batch runs beside
// another worker's, its upload under the other's kernels.  A partitioned database is gone through part group by part group (the job
// selects the group: the next one loads behind this one's queries); between the groups a batch keeps nothing but its reads' candidate
// lists (Batch::carried), and only the last group's pass prints.
struct SetStep {
    const Session& S; const Options& o; BatchQueue& Q;
    const bool hasPrior, prints;                                            // the part group pass: after another one; the last one
    std::vector<Query> queries = {}; Records rec = {};
    std::string seq1 = {}, seq2 = {}; std::vector<uint64_t> off1 = {}, off2 = {}; std::vector<mc_candidate> all = {};

    template <class Emit>
    bool operator()(Batch& B, Emit&& emit)
    {
        const bool paired = o.pairing != Options::unpaired;
        const uint32_t K = S.cfg.max_candidates;
        queries.clear(); seq1.clear(); seq2.clear(); off1.assign(1, 0); off2.assign(1, 0);
        for (size_t q = B.qBeg; q < B.qEnd; ++q) {
            const uint64_t id = Q.read(B, q, rec);
            const uint64_t len = (uint64_t)rec.s1.n + rec.s2.n;
            if (len + 8 > S.cfg.slot_max_chars) { std::cerr << "query batch is too small for a single read!\n"; continue; }
            queries.push_back(Query{id, rec.h1, rec.h1.empty() || rec.s1.empty(), len, q});
            seq1.append(rec.s1.p, rec.s1.n); off1.push_back(seq1.size());
            if (paired) { seq2.append(rec.s2.p, rec.s2.n); off2.push_back(seq2.size()); }
        }
        const size_t n = queries.size();
        if (hasPrior) all.swap(B.carried);                                  // what the earlier part groups left for this batch's reads
        else all.assign(n * K, mc_candidate{});
        if (all.size() != n * K) { Q.fail("internal: a batch changed between two part groups"); return false; }
        seq1.push_back('\0'); seq2.push_back('\0');
        const char* s2 = paired ? seq2.data() : nullptr;
        const uint64_t* o2 = paired ? off2.data() : nullptr;
        const int rc = !n ? MC_OK
                     : S.keyset ? mc_keyset_classify(S.keyset, seq1.data(), off1.data(), s2, o2, n, o.lowest, o.insertMax, all.data())
                                : mc_partset_classify_resident(S.partset, seq1.data(), off1.data(), s2, o2, n, o.lowest, o.insertMax, hasPrior ? 1 : 0, all.data());
        if (rc != MC_OK) { Q.fail(S.keyset ? mc_keyset_last_error(S.keyset) : mc_partset_last_error(S.partset)); return false; }
        if (!prints) { B.carried.swap(all); return true; }                  // more part groups to come: nothing is printed yet
        mc_results r{};
        r.num_queries = (uint32_t)n; r.max_candidates = K; r.cands = all.data();
        emit(queries, r);
        return true;
    }
};

// One worker: batches until none is left.  The device step classifies a batch's queries; here their candidates become lines in a buffer,
// which goes to the ordered writer whole (a batch the job failed in is not written).
template <class Step>
void work(BatchQueue& Q, OrderedOut& W, MappingWriter& L, Step& step, Aligner* aligner = nullptr)
{
    const Options& o = L.o;
    const bool unlimited = o.maxCand < 1;
    FastOut out;
    std::vector<Cand> cands;
    size_t b; Batch* B;
    while (Q.take(b, B)) {
        // (a moved-from string keeps its 15-character SSO capacity, never 0)
        if (step.prints) { out.s.clear(); if (out.s.capacity() < 64) W.take_buffer(out.s); out << B->prefix; }
        const bool done = step(*B, [&](const std::vector<Query>& queries, const mc_results& r) {
            if (L.fmt.step && L.fmt.lines(out, queries, r, L)) return;              // (false: the batch is classified and formatted here, as a whole)
            for (uint32_t i = 0; i < r.num_queries; ++i) {
                const Query& m = queries[i];
                if (m.empty) continue;                                      // processQuery, classification.cpp:780
                device_candidates(r.cands + (size_t)i * r.max_candidates, r.max_candidates, L.tx, o.lowest, cands);
                const mc_location* hits = nullptr; uint64_t nhits = 0;
                if (o.allhits || unlimited) { hits = r.hits + r.hit_offsets[i]; nhits = r.hit_offsets[i + 1] - r.hit_offsets[i]; }
                if (unlimited && cands.size() == r.max_candidates)          // list full: there may be more candidates than it holds
                    host_candidates(hits, nhits, max_windows(m.len, o.insertMax, L.stride), L.tx, o.lowest, cands);
                if (L.deferred) B->deferred.push_back(Deferred{m.id, m.header, cands, m.q});
                else L(out, m.id, m.header, cands, o.allhits ? hits : nullptr, o.allhits ? nhits : 0, m.q);
            }
        });
        L.flush();                                                          // (also for a batch the job failed in: what it gathered is recorded or kept, never dropped)
        if (!done) break;
        if (aligner && step.prints && !L.deferred) {                        // the batch's alignments: one device call, then the lines go into its text
            std::string err;
            if (!aligner->finish(*B, out.s, err)) { Q.fail(err); break; }
        }
        if (step.prints && !W.deliver(b, std::move(out.s))) Q.fail("Could not write to file " + W.name);
    }
}

// ---- reports ----------------------------------------------------------------------------------------------------------------------
void show_query_params(std::ostream& os, const Options& o, unsigned threads)   // printing.cpp:47-131
{
    if (o.mapView != Options::mv_none) {
        os << o.comment << "Reporting per-read mappings (non-mapping lines start with '" << o.comment << "').\n";
        os << o.comment << (o.lineage ? "The complete lineage will be reported starting with the lowest match.\n" : "Only the lowest matching rank will be reported.\n");
    } else os << o.comment << "Per-Read mappings will not be shown.\n";
    if (o.minReadLen > 0) os << o.comment << "Only reads with a minimum length of " << o.minReadLen << " bp will be mapped.\n";
    if (o.maxReadLen < std::numeric_limits<uint64_t>::max()) os << o.comment << "Only reads with a maximum length of " << o.maxReadLen << " bp will be mapped.\n";
    os << o.comment << "Classification will be constrained to ranks from '" << kRankNames[o.lowest] << "' to '" << kRankNames[o.highest] << "'.\n";
    os << o.comment << "Classification hit threshold is " << o.hitsMin << " per query\n";
    os << o.comment << "At maximum " << (o.maxCand < 1 ? std::numeric_limits<size_t>::max() : o.maxCand) << " classification candidates will be considered per query.\n";
    if (o.pairing == Options::files) os << o.comment << "File based paired-end mode:\n" << o.comment << "  Reads from two consecutive files will be interleaved.\n" << o.comment << "  Max insert size considered " << o.insertMax << ".\n";
    else if (o.pairing == Options::sequences) os << o.comment << "Per file paired-end mode:\n" << o.comment << "  Reads from two consecutive sequences in each file will be paired up.\n" << o.comment << "  Max insert size considered " << o.insertMax << ".\n";
    if (o.align) os << o.comment << "Query sequences will be aligned to best candidate target => SLOW!\n";
    if (o.hitsPerRef) os << o.comment << "A list of hits per reference sequence will be generated after the read mapping.\n";
    if (o.abundances) os << o.comment << "A list of absolute and relative abundances per taxon will be generated after the read mapping.\n";
    if (o.abundancePer != kNumRanks) os << o.comment << "A list of absolute and relative abundances for each '" << kRankNames[o.abundancePer] << "' will be generated after the read mapping.\n";
    os << o.comment << "Using " << threads << " threads\n";
}

void show_mapping_header(std::ostream& os, const Options& o)               // show_query_mapping_header, classification.cpp:432-460
{
    os << o.comment << "TABLE_LAYOUT: ";
    if (o.queryIds) os << "query_id" << o.column;
    os << "query_header" << o.column;
    const int rmax = o.lineage ? o.highest : o.lowest;
    auto taxon_header = [&](const std::string& prefix) {                  // show_taxon_header, printing.cpp:133-172
        auto hdr = [&](int r, bool named) {
            if (o.showRank) os << prefix << (named ? kRankNames[r] : "rank") << o.rankSuffix;
            if (o.showName) { os << prefix << "taxname"; if (o.showId) os << o.idPrefix << prefix << "taxid" << o.idSuffix; }
            else if (o.showId) os << prefix << "taxid";
        };
        if (o.lowest == rmax) hdr(o.lowest, false);
        else for (int r = o.lowest; r <= rmax; ++r) { hdr(r, true); if (r < rmax) os << o.taxSep; }
    };
    if (o.showGroundTruth) { taxon_header("truth_"); os << o.column; }
    if (o.allhits) os << "all_hits" << o.column;
    if (o.tophits) os << "top_hits" << o.column;
    if (o.locations) os << "candidate_locations" << o.column;
    taxon_header("");
    os << '\n';
}

// -cov-percentile (map_queries_to_targets_default, classification.cpp:747-838): nothing is classified while the reads are queried; every
// read's candidates are kept (Batch::deferred), the targets are filtered by their coverage afterwards, and the reads are classified from
// the candidates that are left.
// The reference keeps (target -> candidates) in std::unordered_map objects: one per batch of -batch-size reads (4096 unless given,
// options.hpp:232; batches do not span input files), merged into a global one batch after batch (matches_per_target.hpp:100-125).
// filter_targets_by_coverage (classification.cpp:591-634) then walks the global map in ITS iteration order, sums float coverages in that
// order, std::sorts them and erases targets from the low end: the order of equal coverages and the rounding of the sums come from the
// containers.  Same containers, same insertion sequence here (the reference's -threads 1 order), so the same targets go.
// What the containers do NOT decide -- how many windows of a target are covered -- comes from the library (CoverageStep): a batch's
// deferred candidate lists go there as flat rows, and where the library cannot count, the reference's own count below is used.

// the reference's own count (classification.cpp:603-609): one set of windows per target
static size_t host_covered_windows(const std::vector<Cover>& covers)
{
    std::unordered_set<uint32_t> hitWindows;
    for (const Cover& c : covers) for (uint32_t w = c.beg; w <= c.end; ++w) hitWindows.emplace(w);
    return hitWindows.size();
}

void classify_by_coverage(std::ostream& os, const Options& o, const std::deque<Batch>& batches, MappingWriter& L, mc_ctx* ctx, const Profile& P, Aligner* aligner = nullptr)
{
    const Taxonomy& tx = L.tx;
    const size_t refBatch = o.refBatchSize ? o.refBatchSize : 4096;
    std::unordered_map<uint32_t, std::vector<Cover>> tgtMatches;
    {
        std::unordered_map<uint32_t, std::vector<Cover>> batchMap;
        size_t inBatch = 0, curFile = (size_t)-1;
        auto flush = [&]() {
            for (auto& m : batchMap) { auto& t = tgtMatches[m.first]; t.insert(t.end(), m.second.begin(), m.second.end()); }
            batchMap = std::unordered_map<uint32_t, std::vector<Cover>>();
            inBatch = 0;
        };
        for (const Batch& B : batches) {
            if (B.f1 != curFile || B.qBeg == 0) { if (inBatch) flush(); curFile = B.f1; }
            for (const Deferred& d : B.deferred) {
                for (const Cand& c : d.cands) if (records_match(c.tax, c.hits, o)) batchMap[c.tgt].push_back(Cover{c.tgt, d.id, c.beg, c.end, c.hits});
                if (++inBatch == refBatch) flush();
            }
        }
        if (inBatch) flush();
    }
    {
        using CovP = std::pair<uint32_t, float>;
        std::vector<CovP> cov;
        cov.reserve(tgtMatches.size());
        float sum = 0;
        CoverageStep dev;
        dev.open(ctx, o, batches);
        dev.report(P);
        for (const auto& m : tgtMatches) {
            float covP;
            if (dev.ctx && m.first < dev.covered.size()) covP = float(dev.covered[m.first]) / dev.windows[m.first];
            else {
                const Lineage lin = tx.target_ranks(m.first);
                const uint32_t targetSize = tx.taxon(lin[0]) ? (uint32_t)tx.taxon(lin[0])->windows : 0u;
                covP = float(host_covered_windows(m.second)) / targetSize;
            }
            sum += covP;
            cov.emplace_back(m.first, covP);
        }
        std::sort(cov.begin(), cov.end(), [](CovP& a, CovP& b) { return a.second < b.second; });
        float part = 0;
        for (auto it = cov.begin(); it != cov.end(); ++it) {
            part += it->second;
            if (part > o.covPercentile * sum) break;
            tgtMatches.erase(it->first);
        }
    }
    // redo_classification_batched: candidates of erased targets go, then classification and output as usual
    std::ostringstream out;
    std::vector<Cand> left;
    for (const Batch& B : batches) {
        for (const Deferred& d : B.deferred) {
            left.clear();
            for (const Cand& c : d.cands) if (tgtMatches.find(c.tgt) != tgtMatches.end()) left.push_back(c);
            L(out, d.id, d.header, left, nullptr, 0, d.q);
        }
        std::string text = out.str(), err;
        if (aligner && !aligner->finish(B, text, err)) throw std::runtime_error(err);
        os << text;
        out.str(std::string());
    }
    for (const auto& m : tgtMatches) L.tally.covers.insert(L.tally.covers.end(), m.second.begin(), m.second.end());
}

// covers: what stayed on the host (every list where the device was not used); dev: the library's sorted records.  The two are merged
// while they are printed (the device's record first where the four fields the lists are ordered by are equal).
void show_hits_per_ref(std::ostream& os, const Options& o, const Taxonomy& tx, uint32_t stride, std::vector<Cover>& covers,
                       const std::vector<mc_target_hit>& dev = {})   // show_matches_per_targets, printing.cpp:385-420
{
    auto less = [](const Cover& a, const Cover& b) {                               // per target: by window range, then query id
        if (a.tgt != b.tgt) return a.tgt < b.tgt;
        if (a.beg != b.beg) return a.beg < b.beg;
        if (a.end != b.end) return a.end < b.end;
        return a.qid < b.qid;
    };
    std::sort(covers.begin(), covers.end(), less);
    os << o.comment << "--- list of hits for each reference sequence ---\n"
       << o.comment << "window start position within sequence = window_index * window_stride(=" << stride << ")\n";
    os << o.comment << "TABLE_LAYOUT: " << " sequence " << o.column << " windows_in_sequence " << o.column
       << "queryid/first_window_index+additional_windows:hits,queryid/...\n";
    size_t i = 0, j = 0;                                                           // next of covers, of dev
    auto of = [](const mc_target_hit& h) { return Cover{h.tgt, h.query, h.beg, h.end, h.hits}; };
    auto from_dev = [&]() { return j < dev.size() && (i >= covers.size() || !less(covers[i], of(dev[j]))); };
    auto peek = [&](Cover& c) {
        if (i >= covers.size() && j >= dev.size()) return false;
        c = from_dev() ? of(dev[j]) : covers[i];
        return true;
    };
    auto take = [&]() { if (from_dev()) ++j; else ++i; };
    Cover c;
    while (peek(c)) {
        const uint32_t tgt = c.tgt;
        const Lineage lin = tx.target_ranks(tgt);
        show_lineage(os, o, tx, lin, 0, o.lineage ? o.highest : 0);
        os << o.column << (tx.taxon(lin[0]) ? tx.taxon(lin[0])->windows : 0) << o.column;
        for (bool first = true; peek(c) && c.tgt == tgt; take(), first = false) {
            if (!first) os << ',';
            os << c.qid << '/' << c.beg << '+' << (c.end - c.beg) << ':' << c.hits;
        }
        os << '\n';
    }
}

// -abundances: queries per taxon; -abundance-per: the estimate for one rank (estimate_abundance, classification.cpp:304-374)
void show_abundances(std::ostream& os, const Options& o, const Taxonomy& tx, const Tally& T)
{
    const uint64_t nUnassigned = T.unclassified(), nTotal = T.total();
    // taxon_count_map (classification.hpp:48-56): higher ranks first, then ascending taxon id
    auto higher = [&tx](uint32_t a, uint32_t b) {
        const Taxon* x = tx.taxon(a); const Taxon* y = tx.taxon(b);
        if (x->rank != y->rank) return x->rank > y->rank;
        return x->id < y->id;
    };
    std::map<uint32_t, double, decltype(higher)> counts(higher);
    for (const auto& kv : T.counts) counts[kv.first] = kv.second;
    auto table = [&]() {                                                    // show_abundance_table, printing.cpp:424-468
        os << o.comment << "rank" << o.rankSuffix << "name" << o.column << "taxid" << o.column << "number of reads" << o.column << "abundance\n";
        double ipart = 0.0;
        for (const auto& tc : counts) {
            const Taxon* t = tx.taxon(tc.first);
            os << (t->rank == kNumRanks ? "none" : kRankNames[t->rank]) << o.rankSuffix << t->name << o.column;
            os << (t->rank == 0 ? t->parent : t->id) << o.column;
            if (std::modf(tc.second, &ipart) == 0.0) os << ipart;
            else os << std::setprecision(15) << tc.second << std::setprecision(6);
            os << o.column << (tc.second / double(nTotal) * 100) << "%\n";
        }
        os << "unclassified" << o.column << "--" << o.column << '0' << o.column << nUnassigned << o.column
           << (nTotal > 0 ? nUnassigned / double(nTotal) : 0.0) * 100 << "%\n";
    };
    if (o.abundances) { os << o.comment << "query summary: number of queries mapped per taxon\n"; table(); }
    if (o.abundancePer == kNumRanks) return;
    const int rank = o.abundancePer;
    auto first_ancestor = [&](uint32_t t, int from, auto&& accept) -> uint32_t {
        const Lineage lin = tx.ranks_of(t);
        for (int r = from; r < kNumRanks; ++r) if (lin[r] && accept(lin[r])) return lin[r];
        return 0;
    };
    if (rank != 0) {
        // counts below the estimation rank move up to the closest ancestor on or above it (first position that is not
        // "higher" than an imaginary taxon of rank-1 with id 0)
        auto it = counts.begin();
        while (it != counts.end()) {
            const Taxon* t = tx.taxon(it->first);
            if (t->rank > rank - 1 || (t->rank == rank - 1 && t->id < 0)) ++it; else break;
        }
        while (it != counts.end()) {
            const uint32_t anc = first_ancestor(it->first, rank, [](uint32_t) { return true; });
            if (anc) { counts[anc] += it->second; it = counts.erase(it); } else ++it;
        }
    }
    std::unordered_map<uint32_t, std::vector<uint32_t>> children;
    std::unordered_map<uint32_t, uint64_t> weight;
    for (const auto& tc : counts) weight[tc.first] = 0;
    for (auto it = counts.rbegin(); it != counts.rend(); ++it) {           // leaves to root: own count + weight go to the closest counted ancestor
        const uint32_t parent = first_ancestor(it->first, tx.taxon(it->first)->rank + 1, [&](uint32_t a) { return weight.count(a) > 0; });
        if (parent) {
            weight[parent] = (uint64_t)(weight[parent] + (weight[it->first] + it->second));
            children[parent].push_back(it->first);
        }
    }
    for (auto it = counts.begin(); it != counts.end();) {                  // root to leaves: a parent's count is shared out proportionally
        auto ch = children.find(it->first);
        if (ch != children.end()) {
            const uint64_t sumChildren = weight[it->first];
            for (uint32_t c : ch->second) counts[c] += it->second * (counts[c] + weight[c]) / sumChildren;
            it = counts.erase(it);
        } else ++it;
    }
    os << o.comment << "estimated abundance (number of queries) per " << kRankNames[rank] << "\n";
    table();
}

void show_summary(std::ostream& os, const Options& o, const Tally& T, double seconds)   // show_summary, printing.cpp:601-620
{
    const uint64_t nassigned = T.classified(), unassigned = T.unclassified(), total = T.total();
    const uint64_t nq = o.pairing == Options::unpaired ? total : 2 * total;
    os << o.comment << "queries: " << nq << '\n' << o.comment << "time:    " << (long long)(seconds * 1000) << " ms\n"
       << o.comment << "speed:   " << nq / (seconds / 60.0) << " queries/min\n";
    if (total == 0) { std::cerr << o.comment << "No valid query sequences found.\n"; return; }
    // show_taxon_statistics, printing.cpp:502-535
    if (nassigned < 1) { os << "None of the input sequences could be classified.\n"; return; }
    if (unassigned > 0) os << o.comment << "unclassified: " << (100 * (unassigned / double(total))) << "% (" << unassigned << ")\n";
    os << o.comment << "classified:\n";
    const int shown[] = {0, 3, 4, 6, 10, 12, 14, 16, 18, 19, 20};
    auto upto = [](const uint64_t* a, int r) { uint64_t s = 0; for (int x = 0; x <= r; ++x) s += a[x]; return s; };
    auto padded = [](int r) { std::string rn = kRankNames[r]; rn.resize(11, ' '); return rn; };
    for (int r : shown)
        if (upto(T.assigned, r) > 0) os << o.comment << "  " << padded(r) << (100 * (upto(T.assigned, r) / double(total))) << "% (" << upto(T.assigned, r) << ")\n";
    if (upto(T.known, kNumRanks - 1) == 0) return;
    // ground truth block, printing.cpp:537-592
    if (T.known[kNumRanks] > 0) os << o.comment << "ground truth unknown: " << (100 * (T.known[kNumRanks] / double(total))) << "% (" << T.known[kNumRanks] << ")\n";
    os << o.comment << "ground truth known:\n";
    for (int r : shown) if (upto(T.assigned, r) > 0) os << o.comment << "  " << padded(r) << (100 * (upto(T.known, r) / double(total))) << "% (" << upto(T.known, r) << ")\n";
    os << o.comment << "correctly classified:\n";
    for (int r : shown) if (upto(T.assigned, r) > 0) os << o.comment << "  " << padded(r) << upto(T.correct, r) << '\n';
    auto wrongFrom = [&](int r) { uint64_t s = 0; for (int x = r; x < kNumRanks; ++x) s += T.wrong[x]; return s; };
    os << o.comment << "precision (correctly classified / classified) if ground truth known:\n";
    for (int r : shown) if (upto(T.assigned, r) > 0) {
        const double tot = double(upto(T.correct, r)) + double(wrongFrom(r));
        os << o.comment << "  " << padded(r) << (100 * (tot > 0 ? upto(T.correct, r) / tot : 0.0)) << "%\n";
    }
    os << o.comment << "sensitivity (correctly classified / all) if ground truth known:\n";
    for (int r : shown) if (upto(T.assigned, r) > 0)
        os << o.comment << "  " << padded(r) << (100 * (upto(T.known, r) > 0 ? upto(T.correct, r) / double(upto(T.known, r)) : 0.0)) << "%\n";
    if (T.covDomain > 0) {
        os << o.comment << "false positives (hit on taxa not covered in DB):\n";
        for (int r : shown) if (upto(T.assigned, r) > 0) os << o.comment << "  " << padded(r) << T.covFalsePos[r] << "\n";
    }
}

// ---- one query job: the files of one command (or of one -split-out group) -> mapping lines and reports --------------------------------
void run_job(Session& S, Options o, const std::vector<std::string>& infiles, const std::string& outfile, const std::string& targetsFile,
             const std::string& abundanceFile, const MergedInput* merged = nullptr)
{
    if (!merged) S.open(o);
    const Taxonomy& tx = S.tx;
    if (o.hitsMin < 1) o.hitsMin = S.dbSketch >= 6 ? int(S.dbSketch / 3.0) : (S.dbSketch >= 4 ? 2 : 1);     // querying.cpp:257-268
    o.infiles = infiles;
    std::ofstream fout, ftargets, ftaxa;                                    // process_input_files, querying.cpp:84-112
    if (!outfile.empty()) { fout.open(outfile); if (!fout.good()) throw std::runtime_error("Could not write to file " + outfile); }
    if (!targetsFile.empty()) { ftargets.open(targetsFile); if (!ftargets.good()) throw std::runtime_error("Could not write to file " + targetsFile); }
    if (!abundanceFile.empty()) { ftaxa.open(abundanceFile); if (!ftaxa.good()) throw std::runtime_error("Could not write to file " + abundanceFile); }
    std::ostream& os = outfile.empty() ? std::cout : fout;
    std::ostream& perTargetOut = targetsFile.empty() ? os : ftargets;
    std::ostream& perTaxonOut = abundanceFile.empty() ? os : ftaxa;

    if (o.showQueryParams) show_query_params(os, o, S.threads);
    if (merged) {                                                           // merge_result_files, mode_merge.cpp:266-269
        os << o.comment << "Merging " << merged->files.size() << " files:\n";
        for (const auto& f : merged->files) os << o.comment << f << '\n';
    }
    if (o.mapView != Options::mv_none) show_mapping_header(os, o);

    const auto t0 = std::chrono::steady_clock::now();
    const bool covMode = o.covPercentile > 0 && !merged;
    Profile P;
    BatchQueue Q(o, S.workers, t0);
    OrderedOut W(os, fout, outfile);
    std::vector<Tally> tallies(S.workers);
    TargetCache targets(o.showErrors);                                      // -align: the target records of this job
    const bool aligning = o.align && !merged;
    HitsStep hitsStep; EvalStep evalStep; FormatStep fmtStep; ParseStep parseStep; InflateStep inflateStep; InputStep inputStep;   // the hand-offs to the library (mcq_device_steps.h)
    inflateStep.open(S, merged != nullptr);
    if (inflateStep.ctx) Q.inflater = &inflateStep.inflater;
    parseStep.open(S, o, merged != nullptr);
    inputStep.open(S, o, merged != nullptr, covMode, aligning);
    if (inputStep.ctx) Q.input = &inputStep;
    hitsStep.open(S, o, merged != nullptr, covMode);
    evalStep.open(S, o, merged != nullptr, covMode);
    fmtStep.open(S, o, merged != nullptr, covMode, aligning);
    auto worker = [&](unsigned w, auto&& step) {
        MappingWriter L{o, tx, S.dbStride, S.dbWinlen, covMode, tallies[w]};
        if (hitsStep.ctx) L.hits.step = &hitsStep;
        if (evalStep.ctx) L.eval.step = &evalStep;
        if (fmtStep.ctx) L.fmt.step = &fmtStep;
        Aligner A{S.ctx, o, tx, targets, Q, S.dbStride, S.dbWinlen};
        if (aligning && !covMode) L.wants = &A.wants;
        work(Q, W, L, step, aligning ? &A : nullptr);
    };
    Q.start();                                                              // (with part groups: the first pass streams behind the files' indexing)
    if (S.keyset) run_workers(S.workers, [&](unsigned w) { worker(w, SetStep{S, o, Q, false, true}); });
    else if (S.partset) {
        uint64_t pinfo[6] = {0, 0, 1, 0, 0, 0};
        mc_partset_info(S.partset, pinfo);
        const uint32_t groups = (uint32_t)std::max<uint64_t>(pinfo[2], 1);
        for (uint32_t g = 0; g < groups && !Q.failed(); ++g) {
            if (mc_partset_select_group(S.partset, g) != MC_OK) { Q.fail(mc_partset_last_error(S.partset)); break; }
            Q.rewind();
            run_workers(S.workers, [&](unsigned w) { worker(w, SetStep{S, o, Q, g > 0, g + 1 == groups}); });
        }
    } else run_workers(S.workers, [&](unsigned w) { worker(w, SlotStep{S, o, Q, P, S.replica(w % S.replication), w / S.replication, true, {}, {}, &parseStep, &inputStep}); });
    Q.finish();
    W.close();
    Q.rethrow();

    Tally T;
    for (const Tally& t : tallies) T += t;
    evalStep.finish(T);
    hitsStep.finish();
    if (covMode) {
        MappingWriter L{o, tx, S.dbStride, S.dbWinlen, true, T};
        Aligner A{S.ctx, o, tx, targets, Q, S.dbStride, S.dbWinlen};
        A.noReads = true;
        if (aligning) L.wants = &A.wants;
        classify_by_coverage(os, o, Q.batches, L, S.ctx, P, aligning ? &A : nullptr);
    }
    if (merged) {                                                           // map_candidates_to_targets, classification.cpp:891-911
        MappingWriter L{o, tx, S.dbStride, S.dbWinlen, false, T};
        std::ostringstream out;
        for (size_t i = 0; i < merged->headers.size(); ++i) L(out, i + 1, View{merged->headers[i].data(), merged->headers[i].size()}, merged->cands[i], nullptr, 0, 0, merged->assigned.empty() ? nullptr : &merged->assigned[i]);
        os << out.str();
    }
    if (P.on)
        std::cerr << "mcq profile: index " << Q.tIndexed * 1e3 << " ms, total " << std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() * 1e3
                  << " ms; summed over " << S.workers << " workers: parse+add " << P.parse / 1e6 << " ms, submit " << P.submit / 1e6 << " ms, wait "
                  << P.wait / 1e6 << " ms, classify+format " << P.classify / 1e6 << " ms; batches " << Q.batches.size() << "\n";
    inputStep.report(P);
    inflateStep.report(P);
    parseStep.report(P);
    fmtStep.report(P);
    evalStep.report(P);
    hitsStep.report(P, T.covers.size());
    if (o.hitsPerRef) show_hits_per_ref(perTargetOut, o, tx, S.dbStride, T.covers, hitsStep.records);
    if (o.abundances || o.abundancePer != kNumRanks) show_abundances(perTaxonOut, o, tx, T);
    if (o.showSummary) show_summary(os, o, T, std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
}

// ---- merge mode (mode_merge.cpp): result files of queries against single database parts -> one classification ------------------
// get_results_file_properties (mode_merge.cpp:79-150): no sequence-level results, the column of the top hits, number of result lines
struct ResultsSource { std::string filename; size_t firstLine = 0, numQueries = 0; int tophitsColumn = 0; std::vector<std::string> lines; };

// the leading comment block of res.lines (which hold at least that block and the line behind it): its checks, tophitsColumn, firstLine
void results_head(ResultsSource& res)
{
    const std::string& filename = res.filename;
    size_t i = 0;
    for (;; ++i) {
        if (i >= res.lines.size() || res.lines[i].empty() || res.lines[i][0] != '#') throw std::runtime_error("classificaion ranks not found in file " + filename);
        if (res.lines[i].compare(0, 16, "# Classification") == 0) {
            if (res.lines[i].find("sequence") != std::string::npos) throw std::runtime_error("cannot merge results on sequence level");
            break;
        }
    }
    for (++i;; ++i) {
        if (i >= res.lines.size() || res.lines[i].empty() || res.lines[i][0] != '#') throw std::runtime_error("TABLE_LAYOUT not found in file " + filename);
        if (res.lines[i].compare(0, 15, "# TABLE_LAYOUT:") == 0) {
            std::istringstream ls(res.lines[i].substr(15));
            std::string column;
            ls >> column;
            if (column != "query_id") throw std::runtime_error("no query_id in file " + filename);
            int col = 0;
            while (ls.good()) {
                ls.ignore(std::numeric_limits<std::streamsize>::max(), '|');
                ls >> column;
                ++col;
                if (column == "top_hits") { res.tophitsColumn = col; break; }
            }
            break;
        }
    }
    if (res.tophitsColumn < 1) throw std::runtime_error("no top_hits in file " + filename);
    for (++i; i < res.lines.size() && !res.lines[i].empty() && res.lines[i][0] == '#'; ++i) {}
    res.firstLine = i;
}

ResultsSource results_file_properties(const std::string& filename)
{
    ResultsSource res;
    res.filename = filename;
    std::ifstream is(filename);
    if (!is.good()) throw std::runtime_error("could not open file " + filename);
    for (std::string l; std::getline(is, l);) res.lines.push_back(std::move(l));
    results_head(res);
    for (size_t i = res.firstLine; i < res.lines.size(); ++i) if (res.lines[i].empty() || res.lines[i][0] != '#') ++res.numQueries;
    return res;
}

// MCQ_MERGE_DEVICE: a result file mapped into memory; only its leading comment block is read line by line
struct MappedResults {
    MergeFile file;
    int fd = -1;
    explicit MappedResults(const std::string& filename)
    {
        file.name = filename;
        fd = ::open(filename.c_str(), O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) throw std::runtime_error("could not open file " + filename);
        file.size = (size_t)st.st_size;
        if (file.size) {
            void* m = mmap(nullptr, file.size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) throw std::runtime_error("could not open file " + filename);
            file.data = (const char*)m;
        }
        ResultsSource head;
        head.filename = filename;
        size_t s = 0;
        while (s < file.size) {                                                 // the comment block and the line behind it
            const char* nl = (const char*)memchr(file.data + s, '\n', file.size - s);
            const size_t e = nl ? (size_t)(nl - file.data) : file.size;
            head.lines.emplace_back(file.data + s, e - s);
            if (head.lines.back().empty() || head.lines.back()[0] != '#') break;
            s = nl ? e + 1 : file.size;
        }
        file.body = s;
        results_head(head);
        file.tophitsColumn = head.tophitsColumn;
    }
    ~MappedResults() { if (file.data) munmap((void*)file.data, file.size); if (fd >= 0) ::close(fd); }
    MappedResults(const MappedResults&) = delete;
};

// best_distinct_matches_in_contiguous_window_ranges::insert for a candidate that names its taxon (candidate_generation.hpp:172-231)
void insert_taxon_candidate(std::vector<Cand>& top, Cand c, int mergeBelow, size_t maxCand)
{
    if (top.size() == maxCand && top.back().hits >= c.hits) return;
    if (!c.tax) return;
    auto upper = [&] { size_t j = 0; while (j < top.size() && top[j].hits >= c.hits) ++j; return j; };   // upper_bound, hits descending
    auto place = [&] {
        const size_t j = upper();
        if (j != top.size() || top.size() < maxCand) { top.insert(top.begin() + j, c); if (top.size() > maxCand) top.resize(maxCand); }
    };
    if (mergeBelow == 0) { place(); return; }
    size_t i = 0;
    while (i < top.size() && top[i].tax != c.tax) ++i;
    if (i == top.size()) { place(); return; }
    if (c.hits > top[i].hits) {
        top[i] = c;
        for (size_t j = i; j > 0 && top[j].hits > top[j - 1].hits; --j) std::swap(top[j], top[j - 1]);   // std::sort on <= 16 elements: insertion sort
    }
}

// read_results (mode_merge.cpp:158-244)
void read_results(const ResultsSource& res, const Taxonomy& tx, int mergeBelow, size_t maxCand, MergedInput& M, bool info)
{
    // "preallocate" (mode_merge.cpp:172-174) is a plain resize to this file's number of result lines: when ids have gaps (skipped
    // reads) the lists of the highest ids collected from earlier files are cut off here and start again -- kept as the reference has it
    M.cands.resize(res.numQueries); M.headers.resize(res.numQueries);
    for (size_t li = res.firstLine; li < res.lines.size(); ++li) {
        const std::string& l = res.lines[li];
        if (l.empty() || l[0] == '#') continue;
        const char* p = l.c_str();
        char* end = nullptr;
        size_t queryId = (size_t)std::strtoull(p, &end, 10);
        p = end;
        if (queryId > 0) --queryId;
        if (queryId + 1 > M.cands.size()) { M.cands.resize(queryId + 1); M.headers.resize(queryId + 1); }
        auto forward = [&](char c) { const char* q = std::strchr(p, c); p = q ? q + 1 : l.c_str() + l.size(); };
        forward('|');
        if (M.headers[queryId].empty()) {
            const char* a = p;
            while (*a && std::isspace((unsigned char)*a)) ++a;
            const char* b = a;
            while (*b && !std::isspace((unsigned char)*b)) ++b;
            if (b > a) M.headers[queryId].assign(a, b);
        }
        for (int i = 1; i < res.tophitsColumn; ++i) forward('|');
        forward('\t');
        while (*p && *p != '\t') {
            int64_t taxid = std::strtoll(p, &end, 10);
            if (end == p) { taxid = 0; if (info) std::cerr << "Query " << queryId + 1 << ": Could not read taxid.\n"; }
            p = end;
            forward(':');
            const uint32_t hits = (uint32_t)std::strtoul(p, &end, 10);
            p = end;
            const uint32_t t = tx.with_id(taxid);
            if (t) insert_taxon_candidate(M.cands[queryId], Cand{0xFFFFFFFFu, hits, 0, 0, t}, mergeBelow, maxCand);
            else if (info) std::cerr << "Query " << queryId + 1 << ": taxid " << taxid << " not found. Skipping hit.\n";
            if (!*p) break;
            if (*p == '\t') break;                                              // end of the top hits
            ++p;                                                                // ',' between them
        }
    }
}

int merge_main(const std::vector<std::string>& args)
{
    // get_merge_options (options.cpp:1776-1887)
    std::vector<std::string> qargs;
    std::vector<std::string> none;
    std::string taxPath;
    int info = 1;
    for (size_t i = 0; i < args.size(); ++i) {
        if (args[i] == "-taxonomy") { if (i + 1 >= args.size()) throw std::runtime_error("Taxonomy path missing after '-taxonomy'"); taxPath = args[++i]; }
        else if (args[i] == "-silent") info = 0;
        else if (args[i] == "-verbose") info = 2;
        else qargs.push_back(args[i]);
    }
    if (taxPath.empty()) throw std::runtime_error("Taxonomy path missing. Use '-taxonomy <path>'");
    Options o;
    o = parse(qargs, o);
    if (o.infiles.empty()) throw std::runtime_error("No query output filenames provided");
    std::sort(o.infiles.begin(), o.infiles.end());
    if (o.hitsMin == 0) o.hitsMin = 5;
    if (o.lowest < 4) o.lowest = 4;                                             // species
    if (o.infiles.size() < 2) throw std::runtime_error("At least two files are needed for merging");
    // main_mode_merge (mode_merge.cpp:401-432): a database without targets, taxa from the dumps
    BuildOptions bo;
    bo.taxPath = taxPath;
    if (bo.taxPath.back() != '/') bo.taxPath += '/';
    bo.info = info == 0 ? BuildOptions::silent : BuildOptions::moderate;
    Session S;
    {
        std::ostringstream quiet;                                               // the dump reader reports on stdout
        std::streambuf* old = std::cout.rdbuf(quiet.rdbuf());
        TaxTree t = read_taxonomy_dumps(bo);
        std::cout.rdbuf(old);
        if (info) std::cout << quiet.str();
        S.tx.taxa = std::move(t.taxa);
    }
    for (size_t i = 0; i < S.tx.taxa.size(); ++i) S.tx.byId.emplace(S.tx.taxa[i].id, (uint32_t)i);
    S.tx.build_covered();
    if (info) std::cerr << "Applied taxonomy to database.\n";
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    S.threads = o.threads > 0 ? (unsigned)o.threads : hw;
    S.workers = 1;
    if (info) std::cerr << "Merging result files.\n";
    bool anyReadable = false;
    for (const auto& f : o.infiles) { std::ifstream is(f); anyReadable = anyReadable || is.good(); }
    if (!anyReadable) throw std::runtime_error("None of the query sequence files could be opened");
    if (!o.outfile.empty() && info) std::cout << "Per-Read mappings will be written to file: " << o.outfile << std::endl;
    MergedInput M;
    M.files = o.infiles;
    const size_t maxCand = o.maxCand > 0 ? (size_t)o.maxCand : 2;               // merge_result_files, mode_merge.cpp:254-258
    MergeStep mergeStep;                                                        // MCQ_MERGE_DEVICE (mcq_device_steps.h)
    bool onDevice = false;
    if (mergeStep.on) {
        std::vector<std::unique_ptr<MappedResults>> maps;
        std::vector<MergeFile> mfiles;
        for (const auto& f : o.infiles) { maps.emplace_back(new MappedResults(f)); mfiles.push_back(maps.back()->file); }
        onDevice = mergeStep.run(o, S.tx, mfiles, maxCand, M);
        if (!onDevice) { M.cands.clear(); M.headers.clear(); M.assigned.clear(); }
        else if (mergeStep.unknown && info)                                     // (the host path names every such hit; here they are only counted)
            std::cerr << mergeStep.unknown << " hits name taxids that are not in the taxonomy. Skipping them.\n";
        mergeStep.report(Profile(), onDevice, info != 0);
    }
    if (!onDevice) for (const auto& f : o.infiles) read_results(results_file_properties(f), S.tx, o.lowest, maxCand, M, info != 0);
    if (info) std::cerr << "Completed merge. Starting classification.\n";
    run_job(S, o, {}, o.outfile, "", o.abundanceFile, &M);
    return 0;
}

#include "mcq_table_info.h"

// ---- info mode (mode_info.cpp): database properties, targets, lineage table, rank statistics from the metadata alone; the topics that
// describe the table's content (statistics, featurecounts, featuremap) from the table on the device, behind MCQ_INFO_DEVICE=1 ----
int info_main(const std::vector<std::string>& args)
{
    auto static_properties = [](uint32_t tb, uint64_t k, uint64_t sk, uint64_t w, uint64_t stride, uint64_t maxLocs) {   // printing.cpp:625-657
        const char* tid = tb == 2 ? "unsigned short int 16 bits" : "unsigned int 32 bits";
        std::cout << "------------------------------------------------\n"
                  << "MetaCache version  mcq / metacache_amd (MI355X)\n"
                  << "database version   20200820\n"
                  << "------------------------------------------------\n"
                  << "sequence type      mc::char_sequence\n"
                  << "target id type     " << tid << "\n"
                  << "target limit       " << (tb == 2 ? 65535ull : 4294967295ull) << "\n"
                  << "------------------------------------------------\n"
                  << "window id type     unsigned int 32 bits\n"
                  << "window limit       4294967295\n"
                  << "window length      " << w << "\n"
                  << "window stride      " << stride << "\n"
                  << "------------------------------------------------\n"
                  << "sketcher type      mc::single_function_unique_min_hasher<unsigned int, mc::same_size_hash<unsigned int> >\n"
                  << "feature type       unsigned int 32 bits\n"
                  << "feature hash       mc::same_size_hash<unsigned int>\n"
                  << "kmer size          " << k << "\n"
                  << "kmer limit         16\n"
                  << "sketch size        " << sk << "\n"
                  << "------------------------------------------------\n"
                  << "bucket size type   unsigned char 8 bits\n"
                  << "max. locations     " << maxLocs << "\n"
                  << "location limit     254\n"
                  << "------------------------------------------------" << std::endl;
    };
    auto query_config = [] {
        std::cout << "hit classifier       mc::best_distinct_matches_in_contiguous_window_ranges\n"
                  << "------------------------------------------------\n";
    };
    if (args.empty()) { static_properties(4, 0, 0, 0, 0, 254); query_config(); std::cout << std::endl; return 0; }   // show_basic_exec_info: an empty database
    std::string name = args[0];
    { auto pos = name.find(".meta"); if (pos != std::string::npos) name.erase(pos); else { pos = name.find(".cache"); if (pos != std::string::npos) name.erase(pos); } }
    const std::string what = args.size() > 1 ? args[1] : "";
    const char* infoDevice = std::getenv("MCQ_INFO_DEVICE");
    if (info_table_topic(what) && !(infoDevice && std::atoi(infoDevice) != 0))
        throw std::runtime_error("'info " + what + "' describes the reference's host hash table; not available here");
    std::cerr << "Reading database '" << name << "' ... Reading database metadata ...\nCompleted database reading.\ndone." << std::endl;
    mc_ctx* ctx = nullptr;
    if (mc_open_metadata(name.c_str(), &ctx) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
    struct Guard { mc_ctx* c; ~Guard() { mc_destroy(c); } } guard{ctx};
    uint64_t info[8]; mc_db_info(ctx, info);
    Taxonomy tx;
    read_taxa(ctx, tx);
    std::vector<std::string> srcFile(tx.taxa.size()); std::vector<uint64_t> srcIndex(tx.taxa.size());
    for (size_t i = 0; i < tx.taxa.size(); ++i) {
        const char* fn;
        mc_db_taxon_source(ctx, i, &fn, &srcIndex[i], nullptr);
        srcFile[i] = fn;
        tx.byId.emplace(tx.taxa[i].id, (uint32_t)i);
        if (tx.taxa[i].rank == 0 && tx.taxa[i].id < 0) tx.targetByName.emplace(tx.taxa[i].name, (uint32_t)i + 1);
    }
    mc_db_lineages(ctx, &tx.targetLineages, &tx.numTargets);
    uint32_t tb = 4;
    { std::ifstream is(name + ".meta", std::ios::binary); char hdr[10] = {}; is.read(hdr, 10); if (is.gcount() == 10) tb = (uint8_t)hdr[9]; }
    if (info_table_topic(what)) {                                                // show_database_statistics / show_feature_map / show_feature_counts
        static_properties(tb, info[0], info[1], info[2], info[3], info[4]);
        uint64_t ranked = 0, inTree = 0;
        for (const Taxon& t : tx.taxa) {
            const bool target = t.rank == 0 && t.id < 0;
            if (target && t.parent != 0) ++ranked;
            if (!target) ++inTree;
        }
        return info_table_content(name, what, info[6], info[5], ranked, inTree);
    }
    if (what.empty()) {                                                          // show_database_config
        static_properties(tb, info[0], info[1], info[2], info[3], info[4]);
        query_config();
        std::cout << "database parts       " << info[6] << "\n------------------------------------------------\n";
        return 0;
    }
    auto show_target = [&](uint32_t tgt) {                                       // show_target_info, mode_info.cpp:106-121
        const Lineage lin = tx.target_ranks(tgt);
        const Taxon* t = tx.taxon(lin[0]);
        if (!t) return;
        std::cout << "Target " << t->name << "):\n    source:     " << srcFile[lin[0] - 1] << " / " << srcIndex[lin[0] - 1]
                  << "\n    length:     " << t->windows << " windows";
        for (uint32_t l : lin) {
            const Taxon* a = tx.taxon(l);
            if (!a) continue;
            std::string rn = std::string(kRankNames[a->rank]) + ":";
            rn.resize(12, ' ');
            std::cout << "\n    " << rn << "(" << a->id << ") " << a->name;
        }
        std::cout << '\n';
    };
    if (what == "targets" || what == "target" || what == "reference" || what == "references" || what == "ref" || what == "sequence" || what == "sequences" || what == "seq") {
        if (args.size() > 2) {
            for (size_t i = 2; i < args.size(); ++i) {
                const uint32_t t = tx.with_name(args[i]);
                if (t && tx.taxon(t)->id < 0) show_target((uint32_t)(-tx.taxon(t)->id - 1));
                else std::cout << "Target (reference sequence) '" << args[i] << "' not found in database.\n";
            }
        } else {
            std::cout << "Targets (reference sequences) in database:\n";
            for (uint64_t t = 0; t < tx.numTargets; ++t) show_target((uint32_t)t);
        }
        return 0;
    }
    if (what == "lineages" || what == "lineage" || what == "lin") {              // show_lineage_table, mode_info.cpp:157-186
        if (tx.numTargets < 1) return 0;
        std::cout << "name";
        for (int r = 0; r <= 19; ++r) std::cout << '\t' << kRankNames[r];
        std::cout << '\n';
        for (uint64_t t = 0; t < tx.numTargets; ++t) {
            const Lineage lin = tx.target_ranks((uint32_t)t);
            const Taxon* me = tx.taxon(lin[0]);
            std::cout << (me ? me->name : std::string());
            for (int r = 0; r <= 19; ++r) { const Taxon* a = tx.taxon(lin[r]); std::cout << '\t' << (a ? a->id : 0); }
            std::cout << '\n';
        }
        return 0;
    }
    if (what == "rank") {                                                        // show_rank_statistics, mode_info.cpp:193-232
        const int rank = args.size() > 2 ? rank_from_name(args[2]) : -1;
        if (rank < 0 || rank >= kNumRanks) {
            std::cerr << "Please specify a taxonomic rank:\n";
            for (int r = 0; r <= 19; ++r) std::cerr << "    " << kRankNames[r] << '\n';
            return 0;
        }
        std::vector<std::pair<uint32_t, size_t>> stat;                           // the reference walks a map keyed by taxon address
        for (uint64_t t = 0; t < tx.numTargets; ++t) {
            const uint32_t a = tx.target_ranks((uint32_t)t)[rank];
            if (!a) continue;
            auto it = std::find_if(stat.begin(), stat.end(), [&](const std::pair<uint32_t, size_t>& x) { return x.first == a; });
            if (it == stat.end()) stat.emplace_back(a, 1); else ++it->second;
        }
        std::cout << "Sequence distribution for rank '" << kRankNames[rank] << "':\n" << "taxid \t taxon_name \t sequences" << std::endl;
        for (const auto& x : stat) std::cout << tx.taxon(x.first)->id << " \t " << tx.taxon(x.first)->name << " \t " << x.second << '\n';
        return 0;
    }
    throw std::runtime_error("unknown info topic '" + what + "'");
}

// query mode proper / the query half of build+query: files of the command line, or the interactive loop
int query_main(Session& S, const Options& init)
{
    auto process = [&](const Options& o) {                                   // process_input_files, querying.cpp:141-222
        if (!o.splitOut) { run_job(S, o, o.infiles, o.outfile, o.targetsFile, o.abundanceFile); return; }
        const size_t stride = (o.pairing == Options::files && o.infiles.size() > 1) ? 2 : 1;
        for (size_t i = 0; i + stride <= o.infiles.size(); i += stride) {
            std::vector<std::string> in(o.infiles.begin() + i, o.infiles.begin() + i + stride);
            std::string suffix;
            for (const auto& f : in) suffix += "_" + f.substr(f.find_last_of("/\\") + 1);
            auto named = [&](const std::string& f) { return f.empty() ? std::string() : f + suffix + ".txt"; };
            run_job(S, o, in, named(o.outfile), named(o.targetsFile), named(o.abundanceFile));
        }
    };
    if (!init.infiles.empty()) { process(init); return 0; }
    // run_interactive_query_mode (querying.cpp:274-322)
    S.open(init);
    std::cout << "Running in interactive mode:\n"
                 " - Enter input file name(s) and command line options and press return.\n"
                 " - The initially given command line options will be used as defaults.\n"
                 " - All command line options that would modify the database are ignored.\n"
                 " - Each line will be processed separately.\n"
                 " - Lines starting with '#' will be ignored.\n"
                 " - Enter an empty line or press Ctrl-D to quit MetaCache.\n" << std::endl;
    for (;;) {
        std::cout << "$> " << std::flush;
        std::string line;
        std::getline(std::cin, line);
        if (line.empty() || line.find(":q") == 0) { std::cout << "Terminate." << std::endl; return 0; }
        if (line[0] == '#') continue;
        std::vector<std::string> args;
        std::istringstream iss(line);
        for (std::string w; iss >> w;) args.push_back(w);
        try {
            Options o = parse(args, init);
            // load-time settings stay those of the initial command line
            o.maxLocs = init.maxLocs; o.removeOverpopulated = init.removeOverpopulated; o.maxLoadFac = init.maxLoadFac;
            if (o.infiles.empty()) { if (init.showErrors) std::cerr << "No input filenames provided!\n"; continue; }
            process(o);
        } catch (std::exception& e) { if (init.showErrors) std::cerr << e.what() << '\n'; }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    // The HIP runtime's "direct dispatch" (the calling thread writes the queue packets itself) made the query phase of this program -- many
    // worker threads, eight streams -- run at one of two speeds from process to process: hipMemcpyAsync and the kernel launches of a batch
    // took 0.2 or 3-10 ms (150 Gbp: 81-130 or 300-480 ms per 10^7 reads, the kernels' time the same).  With the runtime's own
    // submission threads every run is the fast kind.  The runtime reads the switch when it starts, i.e. before main: the program starts
    // itself again with it set (once; a value the user has set is left alone).
    if (!std::getenv("AMD_DIRECT_DISPATCH") && !std::getenv("MCQ_NO_REEXEC")) {
        setenv("AMD_DIRECT_DISPATCH", "0", 0);
        setenv("MCQ_NO_REEXEC", "1", 1);
        execv("/proc/self/exe", argv);
        // (no /proc: go on as we are)
    }
    try {
        const std::string mode = argc > 1 ? argv[1] : "";
        const std::vector<std::string> args(argv + std::min(argc, 2), argv + argc);
        if (mode == "query") {
            if (args.empty()) throw std::runtime_error("usage: mcq query <database> [<sequence file/directory>...] [options]");
            Options init;
            init.db = args[0];
            init = parse(std::vector<std::string>(args.begin() + 1, args.end()), init);
            Session S;
            return query_main(S, init);
        }
        if (mode == "merge") return merge_main(args);
        if (mode == "info") return info_main(args);
        if (mode == "build") {                                                  // main_mode_build, mode_build.cpp:93-106, :41-66
            using clock = std::chrono::steady_clock;
            std::vector<std::string> none;
            const BuildOptions bo = parse_build(args, false, none);
            if (InflateStep::wanted() && std::getenv("MCQ_PROFILE")) std::cerr << "mcq: gzip input inflated on the host (build)\n";
            const bool info = bo.info != BuildOptions::silent;
            if (info) std::cout << "Building new database '" << bo.dbfile << "' from reference sequences." << std::endl;
            const auto t0 = clock::now();
            BuiltDatabase db;
            build_database(bo, db);
            const double btime = std::chrono::duration<double>(clock::now() - t0).count();
            db.write();
            const double total = std::chrono::duration<double>(clock::now() - t0).count();
            if (info)
                std::cout << "------------------------------------------------\n"
                          << "Construction time: " << btime << " s\n"
                          << "Writing time:      " << total - btime << " s\n"
                          << "Total build time:  " << total << " s" << std::endl;
            return 0;
        }
        if (mode == "modify") {                                                 // main_mode_modify, mode_build.cpp:74-88
            std::vector<std::string> none;
            BuildOptions bo = parse_build(args, false, none);
            if (InflateStep::wanted() && std::getenv("MCQ_PROFILE")) std::cerr << "mcq: gzip input inflated on the host (modify)\n";
            std::cout << "Modify database " << bo.dbfile << std::endl;
            {   // get_modify_options (options.cpp:765-795): sketching and limits of the database file are the defaults
                mc_ctx* meta = nullptr;
                if (mc_open_metadata(bo.dbfile.c_str(), &meta) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
                uint64_t info[8]; mc_db_info(meta, info);
                mc_destroy(meta);
                bo.k = (uint32_t)info[0]; bo.s = (uint32_t)info[1]; bo.w = (uint32_t)info[2]; bo.stride = (uint32_t)info[3];
                if (!bo.maxLocsGiven) bo.maxLocs = (int)info[4];
                std::ifstream is(bo.dbfile + ".meta", std::ios::binary);
                char hdr[10] = {};
                is.read(hdr, 10);
                bo.targetIdBytes = (is.gcount() == 10 && (uint8_t)hdr[9] == 2) ? 2 : 4;
            }
            bo.modify = true;
            // the reference parses the command line twice (options.cpp:772 and :786) and its value list grows both times: every new
            // file is added twice, the second copy's sequences under '<id>!1' names
            { const std::vector<std::string> once = bo.infiles; bo.infiles.insert(bo.infiles.end(), once.begin(), once.end()); }
            if (bo.info != BuildOptions::silent) std::cout << "Adding reference sequences to database..." << std::endl;
            BuiltDatabase db;
            build_database(bo, db);
            db.write();
            return 0;
        }
        if (mode == "build+query") {                                            // main_mode_build_query, mode_build_query.cpp:41-94
            std::vector<std::string> qargs;
            const BuildOptions bo = parse_build(args, true, qargs);
            if (bo.info != BuildOptions::silent) std::cout << "Building new database from reference sequences." << std::endl;
            BuiltDatabase db;
            build_database(bo, db);
            Options init;
            init.db = "<built in memory>";
            init = parse(qargs, init);
            int rc = 0;
            {
                Session S;
                S.built = &db;
                rc = query_main(S, init);
            }
            if (bo.saveDb) db.write();
            return rc;
        }
        throw std::runtime_error("usage: mcq query|build|modify|build+query|merge|info ... (see the header of mcq_main.cpp / mcq_build.h)");
    } catch (std::exception& e) {
        std::cerr << "ABORT: " << e.what() << "!" << std::endl;                  // main.cpp:65-68
        return 1;
    }
    return 0;
}
