// mcq_device_steps.h -- `mcq query`: handing a batch's work to the library instead of doing it in the host loop.
// A hand-off -- coverage, hits, evaluate, format: the four sections below -- is one DeviceStep per job with three steps for run_job: open (the
// switch, the reasons to stay on the host, the opening library call), finish (the library's results into the Tally / its sorted records)
// and report (the stderr lines); and one client per worker, which owns the buffers a batch is gathered in and their flush.  A call that
// fails leaves its whole batch to the host loop, so that nothing is counted twice, and the step keeps the reason of the first such batch.
// Part of mcq_main.cpp's one translation unit: included there behind what it uses (Options, FastOut, show_taxon, Cand, ground_truth,
// lowest_ranked_ancestor, device_candidates, Session, Cover, Tally, Batch, Profile).
#ifndef MCQ_DEVICE_STEPS_H_
#define MCQ_DEVICE_STEPS_H_

struct DeviceStep {
    mc_ctx* ctx = nullptr;                   // the context the batches go to (null: the host loop does the work)
    std::string off;                         // asked for and not on the device: why
    std::mutex mtx; std::string firstError;  // firstError: why the first batch that stayed on the host did
    uint64_t calls = 0, reads = 0, hostBatches = 0;
    void took(uint64_t n) { std::lock_guard<std::mutex> l(mtx); ++calls; reads += n; }
    void note(const std::string& why) { std::lock_guard<std::mutex> l(mtx); if (hostBatches++ == 0) firstError = why; }
    // under MCQ_PROFILE: what the library did (`device`, up to the number of batches it left to the host), or that the host did it all and why
    void report(const Profile& P, const std::string& device, const char* left, const char* host) const
    {
        if (P.on && ctx) std::cerr << "mcq profile: " << device << hostBatches << left << (hostBatches ? " (" + firstError + ")" : std::string()) << "\n";
        else if (P.on && !off.empty()) std::cerr << "mcq: " << host << " (" << off << ")\n";
    }
};

// The reasons to stay on the host that the hand-offs share, in the order they are looked at ("": none).  A hand-off words what -cov-percentile
// means to it, and its own reasons stand between the shared ones: ownFirst in front of -cov-percentile, ownSecond in front of the contexts.
static std::string shared_host_reason(const Session& S, bool merged, bool covMode, const char* covWording, const char* ownFirst = nullptr, const char* ownSecond = nullptr)
{
    if (merged) return "merge mode";
    if (ownFirst) return ownFirst;
    if (covMode) return covWording;
    if (ownSecond) return ownSecond;
    return S.keyset || S.partset || S.replication > 1 || !S.ctx ? "the run uses more than one context" : "";   // (the sharded command lines, -replicate)
}

// matches_per_target::insert's rule (matches_per_target.hpp:100-110): a record for every candidate whose target has a taxon on rank `lowest`
// or the closest one above it, and whose hits reach -hitmin.  For a candidate from the device Cand::tax IS that taxon -- device_candidates
// and host_candidates set it to lowest_ranked_ancestor(tx, tgt, lowest), nothing changes it -- so `Cand::tax != 0` and
// `lowest_ranked_ancestor(tx, tgt, lowest) != 0` are the same predicate there: lists of Cands pass the first, flat rows the second.
// (Merge mode's candidates have a taxon and no target, and exist as Cands only.)
inline bool records_match(uint32_t tax, uint32_t hits, const Options& o) { return tax && hits >= (uint32_t)o.hitsMin; }
inline mc_candidate as_candidate(const Cand& c) { return mc_candidate{c.tgt, c.hits, c.beg, c.end}; }

// n candidate lists (len(i) entries: at(i, j)) as flat rows padded to the longest list, as mc_coverage_add and mc_target_hits_add take them; -> a row's length
template <class Len, class At>
size_t padded_rows(size_t n, Len&& len, At&& at, std::vector<mc_candidate>& rows)
{
    size_t rowLen = 0;
    for (size_t i = 0; i < n; ++i) rowLen = std::max<size_t>(rowLen, len(i));
    rows.assign(n * rowLen, mc_candidate{0, 0, 0, 0});
    for (size_t i = 0; i < n; ++i) for (size_t j = 0, m = len(i); j < m; ++j) rows[i * rowLen + j] = at(i, j);
    return rowLen;
}

// ---- coverage (mc_coverage_*): how many windows of a target -cov-percentile's deferred candidates cover -----------------
// The lists (Batch::deferred) go through mc_coverage_add batch by batch, one mc_coverage_counts gives every target's count and size.  Off: the
// context cannot do it (no window counts, no lineages) or saw entries outside their targets (an inconsistent database) -- the caller counts on
// the host then, and report() says so: the fall-back is never silent.  A candidate list never holds an entry without hits in front of one with
// hits (its rows end at the first hits == 0), so the kernel's "a row ends at hits == 0" and the host's loop over every entry see the same entries.
struct CoverageStep : DeviceStep {
    std::vector<uint32_t> covered, windows;  // per target
    uint64_t stats[4] = {0, 0, 0, 0};
    void open(mc_ctx* c, const Options& o, const std::deque<Batch>& batches)
    {
        uint64_t nt = 0; std::vector<mc_candidate> rows;
        if (!c) { off = "no context"; return; }
        if (mc_coverage_counts(c, nullptr, nullptr, 0, &nt, nullptr, 1) != MC_OK) { off = mc_last_error(c); return; }   // (an empty bitmap to begin with)
        for (const Batch& B : batches) {
            const auto& reads = B.deferred;
            const size_t rowLen = padded_rows(reads.size(), [&](size_t i) { return reads[i].cands.size(); }, [&](size_t i, size_t j) { return as_candidate(reads[i].cands[j]); }, rows);
            if (rowLen && mc_coverage_add(c, rows.data(), (uint32_t)reads.size(), (uint32_t)rowLen, (uint32_t)o.hitsMin, o.lowest, MC_COVERAGE_HOST, nullptr) != MC_OK) { off = mc_last_error(c); return; }
        }
        covered.assign(nt, 0); windows.assign(nt, 0);
        if (mc_coverage_counts(c, covered.data(), windows.data(), nt, nullptr, stats, 1) != MC_OK) off = mc_last_error(c);
        else if (stats[1] != 0) off = std::to_string(stats[1]) + " candidates lie outside their targets' windows";
        else ctx = c;
    }
    void report(const Profile& P) const
    {
        if (!ctx) std::cerr << "mcq: -cov-percentile: covered windows counted on the host (" << off << ")\n";
        else if (P.on) std::cerr << "mcq profile: coverage on the device: " << stats[3] << " mc_coverage_add calls, " << stats[0] << " candidates marked, " << stats[2] << " windows covered\n";
    }
};

// ---- hits (mc_target_hits_*): -hits-per-ref's records in the library's log ---------------------------------------------
// The lists are built by the library where one context serves the whole run; under -cov-percentile, in the sharded command lines and in
// merge they are built on the host.  A batch the library does not take (MC_ERR_NOMEM: the log may not grow further) stays on the host too.
constexpr bool kTargetHitsOnDevice = false;  // the default of `mcq query -hits-per-ref` (DESIGN.md 7d says what decides it); MCQ_TARGET_HITS_DEVICE overrides
struct HitsStep : DeviceStep {
    uint32_t hostEvery = 0;                  // MCQ_TARGET_HITS_HOST_EVERY=k (tests): every k-th batch of a worker stays on the host as if its call had failed
    uint64_t stats[4] = {0, 0, 0, 0};
    std::vector<mc_target_hit> records;      // the library's sorted records, after finish()
    void open(const Session& S, const Options& o, bool merged, bool covMode)
    {
        if (!o.hitsPerRef) return;
        const char* sw = std::getenv("MCQ_TARGET_HITS_DEVICE");                // 1 / 0: the library's log / the host vector, whatever the default
        if (!(sw ? std::atoi(sw) != 0 : kTargetHitsOnDevice)) off = "the host sort is the default here (MCQ_TARGET_HITS_DEVICE=1 selects the library's log)";
        else off = shared_host_reason(S, merged, covMode, "-cov-percentile keeps the candidates on the host");
        if (off.empty() && mc_target_hits_collect(S.ctx, nullptr, 0, nullptr, nullptr, 0, nullptr, nullptr, 1) != MC_OK) off = mc_last_error(S.ctx);   // (an empty log to begin with)
        if (off.empty()) ctx = S.ctx;
        if (const char* e = std::getenv("MCQ_TARGET_HITS_HOST_EVERY")) hostEvery = (uint32_t)std::max(0, std::atoi(e));
    }
    void finish()                            // mc_target_hits_collect replaces the sort of all records on one host thread
    {
        if (!ctx) return;
        uint64_t nt = 0, nr = 0;
        if (mc_target_hits_collect(ctx, nullptr, 0, &nt, nullptr, 0, &nr, nullptr, 0) != MC_OK) throw std::runtime_error(mc_last_error(ctx));
        records.resize(nr);
        if (mc_target_hits_collect(ctx, nullptr, 0, nullptr, records.data(), nr, nullptr, stats, 1) != MC_OK) throw std::runtime_error(mc_last_error(ctx));
        mc_target_hits_reserve(ctx, 0);                                         // (the log's memory goes back)
    }
    void report(const Profile& P, size_t hostRecords) const
    {
        DeviceStep::report(P, "hits per target on the device: " + std::to_string(stats[2]) + " mc_target_hits_add calls, " + std::to_string(stats[0]) + " records, " + std::to_string(stats[3]) + " targets, " + std::to_string(hostRecords) + " records of ",
                           " batches kept on the host", "-hits-per-ref: lists built on the host");
    }
};
struct HitsClient {                          // a worker's candidates since its last flush: list after list, with their query ids
    HitsStep* step = nullptr;                // (null: the records go to Tally::covers one by one)
    std::vector<mc_candidate> cands, rows; std::vector<uint64_t> ids;
    std::vector<size_t> ends; uint32_t flushes = 0;   // list i: cands[ends[i - 1] .. ends[i])
    void add(uint64_t id, const std::vector<Cand>& list)
    {
        for (const Cand& c : list) cands.push_back(as_candidate(c));
        if (!list.empty()) { ids.push_back(id); ends.push_back(cands.size()); }
    }
    // through mc_target_hits_add (the library applies records_match's rule); if the call fails nothing of the batch was recorded: its entries go to `covers`
    void flush(const Options& o, const Taxonomy& tx, std::vector<Cover>& covers)
    {
        const size_t n = ids.size();
        if (step && n) {
            auto begin = [&](size_t i) { return i ? ends[i - 1] : 0; };
            const size_t rowLen = padded_rows(n, [&](size_t i) { return ends[i] - begin(i); }, [&](size_t i, size_t j) { return cands[begin(i) + j]; }, rows);
            const bool held = step->hostEvery && ++flushes % step->hostEvery == 0;
            if (held || mc_target_hits_add(step->ctx, rows.data(), ids.data(), 0, (uint32_t)n, (uint32_t)rowLen, (uint32_t)o.hitsMin, o.lowest, MC_TARGET_HITS_HOST, nullptr) != MC_OK) {
                step->note(held ? "MCQ_TARGET_HITS_HOST_EVERY" : mc_last_error(step->ctx));
                for (size_t i = 0, j = 0; i < n; ++i) for (; j < ends[i]; ++j)
                    if (records_match(lowest_ranked_ancestor(tx, cands[j].tgt, o.lowest), cands[j].hits, o)) covers.push_back(Cover{cands[j].tgt, ids[i], cands[j].beg, cands[j].end, cands[j].hits});
            }
        }
        cands.clear(); ends.clear(); ids.clear();
    }
};

// ---- evaluate (mc_evaluate_*): -precision / -taxon-coverage counted by the library -------------------------------------
// The workers hand every batch's (assigned taxon, truth) pairs over instead of counting them, where MCQ_EVALUATE_DEVICE=1 asks for it and one
// context serves the whole run; under -cov-percentile, in the sharded command lines and in merge the host loop stays.
struct EvalStep : DeviceStep {
    void open(const Session& S, const Options& o, bool merged, bool covMode)
    {
        const char* sw = std::getenv("MCQ_EVALUATE_DEVICE");
        if (!o.precision || !sw || std::atoi(sw) == 0) return;
        mc_evaluation e0;
        off = shared_host_reason(S, merged, covMode, "-cov-percentile classifies on the host after the coverage filter");
        if (off.empty() && mc_evaluate_tally(S.ctx, &e0, 1) != MC_OK) off = mc_last_error(S.ctx);      // (counters at zero to begin with)
        if (off.empty()) ctx = S.ctx;
    }
    void finish(Tally& T)                    // what the library counted, beside what stayed on the host
    {
        if (!ctx) return;
        mc_evaluation E;
        if (mc_evaluate_tally(ctx, &E, 1) != MC_OK) throw std::runtime_error(mc_last_error(ctx));
        for (int r = 0; r <= kNumRanks; ++r) { T.known[r] += E.known[r]; T.correct[r] += E.correct[r]; T.wrong[r] += E.wrong[r]; T.covFalsePos[r] += E.coverage[r][1]; }
        for (int c = 0; c < 4; ++c) T.covDomain += E.coverage[19][c];
    }
    void report(const Profile& P) const
    {
        DeviceStep::report(P, "evaluation on the device: " + std::to_string(calls) + " mc_evaluate_assignments calls, " + std::to_string(reads) + " reads, ", " batches counted on the host", "-precision: evaluated on the host");
    }
};
struct EvalClient {                          // a worker's pairs since its last flush
    EvalStep* step = nullptr;                // (null: the reads are counted on the host one by one)
    std::vector<mc_assignment> assigned; std::vector<uint32_t> truth;
    void add(mc_assignment a, uint32_t t) { assigned.push_back(a); truth.push_back(t); }
    // through mc_evaluate_assignments; if the call fails the batch's reads are counted by onHost(taxon, truth) as they always were.  A batch is one staged piece (a few
    // thousand reads against the library's 4 * 10^6), so a call that failed has counted nothing of it there; a failure after the first of several pieces would count those twice.
    template <class OnHost>
    void flush(const Options& o, OnHost&& onHost)
    {
        if (!step || truth.empty()) return;
        const int flags = MC_EVALUATE_HOST | MC_EVALUATE_TALLY | (o.taxonCoverage ? MC_EVALUATE_COVERAGE : 0);
        if (mc_evaluate_assignments(step->ctx, assigned.data(), truth.data(), (uint32_t)truth.size(), flags, nullptr, nullptr) == MC_OK) step->took(truth.size());
        else { step->note(mc_last_error(step->ctx)); for (size_t i = 0; i < truth.size(); ++i) onHost(assigned[i].taxon, truth[i]); }
        assigned.clear(); truth.clear();
    }
};

// ---- format (mc_format_*): the mapping lines rendered by the library --------------------------------------------------
// With MCQ_FORMAT_DEVICE=1 a worker lays a batch's candidates out as flat rows, has the library vote (mc_classify_candidates) and render the
// lines (mc_format_mappings), and takes its tallies from the assignments.  What the library does not print (the alignment lines; -allhits unless
// MCQ_ALLHITS_DEVICE=1 asks for mc_format_matches too), what classifies later or elsewhere (-cov-percentile, -maxcand 0's host candidates, the
// sharded command lines, merge) keeps the host loop.
// The three string tables of mc_format_set_text for this job's output options, from the functions the host loop prints with: the result
// text of every taxon (entry 0: unclassified), the result text of every target (sequence-level results print the TARGET's lineage) and
// the text a candidate of every target has in front of ":hits" (show_candidates).  false + why: the library did not take a table.
static bool set_format_tables(mc_ctx* ctx, const Options& o, const Taxonomy& tx, std::string& why)
{
    FastOut t;
    std::vector<uint64_t> off;
    auto begin = [&]() { t.s.clear(); off.assign(1, 0); };
    auto set = [&](int which) { const bool ok = mc_format_set_text(ctx, which, t.s.data(), off.data(), off.size() - 1) == MC_OK; if (!ok) why = mc_last_error(ctx); return ok; };
    begin();
    for (uint32_t x = 0; x <= tx.taxa.size(); ++x) { show_taxon(t, o, tx, x, false, 0); off.push_back(t.s.size()); }
    if (!set(MC_TEXT_RESULT)) return false;
    begin();
    for (uint64_t tgt = 0; tgt < tx.numTargets; ++tgt) { show_taxon(t, o, tx, tx.targetLineages[tgt * kNumRanks], true, (uint32_t)tgt); off.push_back(t.s.size()); }
    if (!set(MC_TEXT_TARGET_RESULT)) return false;
    begin();
    for (uint64_t tgt = 0; tgt < tx.numTargets; ++tgt) {
        const Taxon* x = tx.taxon(lowest_ranked_ancestor(tx, (uint32_t)tgt, o.lowest));
        if (x && o.lowest == 0) t << x->name;
        else if (x) {
            const Taxon* a = x->rank < o.lowest ? tx.taxon(tx.target_ranks((uint32_t)tgt)[o.lowest]) : x;
            if (a) t << a->id; else t << x->name;
        }
        off.push_back(t.s.size());
    }
    return set(MC_TEXT_CANDIDATE);
}
// The table of mc_format_matches_set_text: what show_matches' emit prints in front of "/window:count," (-lowest sequence: the name of the target's
// own taxon, nothing for a target without one) or ":count," (the name of the ancestor on exactly rank -lowest, else of the target's own taxon).
static bool set_matches_table(mc_ctx* ctx, const Options& o, const Taxonomy& tx, std::string& why)
{
    FastOut t;
    std::vector<uint64_t> off(1, 0);
    for (uint64_t tgt = 0; tgt < tx.numTargets; ++tgt) {
        const Lineage lin = tx.target_ranks((uint32_t)tgt);
        const Taxon* x = tx.taxon(lin[o.lowest]);
        if (!x && o.lowest != 0) x = tx.taxon(lin[0]);
        if (x) t << x->name;
        off.push_back(t.s.size());
    }
    const bool ok = mc_format_matches_set_text(ctx, t.s.data(), off.data(), off.size() - 1) == MC_OK;
    if (!ok) why = mc_last_error(ctx);
    return ok;
}
struct FormatStep : DeviceStep {
    mc_format_options opt{}; mc_classify_options vote{};
    uint64_t lines = 0; int flags = 0;       // flags: MC_FORMAT_HOST | what the output options ask for
    bool allhits = false; int matchFlags = 0;   // MCQ_ALLHITS_DEVICE with -allhits: the column comes from mc_format_matches
    uint64_t matchCalls = 0, matchReads = 0, matchBytes = 0;
    void took(uint64_t n, uint64_t l) { std::lock_guard<std::mutex> g(mtx); ++calls; reads += n; lines += l; }
    void took_matches(uint64_t n, uint64_t bytes) { std::lock_guard<std::mutex> g(mtx); ++matchCalls; matchReads += n; matchBytes += bytes; }
    void open(const Session& S, const Options& o, bool merged, bool covMode, bool aligning)
    {
        const char* sw = std::getenv("MCQ_FORMAT_DEVICE");
        if (!sw || std::atoi(sw) == 0) return;
        const char* sa = std::getenv("MCQ_ALLHITS_DEVICE");
        const bool matchesToo = o.allhits && sa && std::atoi(sa) != 0;
        const char* first = o.mapView == Options::mv_none ? "no mapping lines are printed" : o.allhits && !matchesToo ? "-allhits: the library does not print location lists"
                          : aligning ? "-align: the alignment lines are put into the host's lines" : nullptr;
        const char* second = o.maxCand < 1 ? "-maxcand 0: lists longer than the device's are made on the host" : nullptr;
        off = shared_host_reason(S, merged, covMode, "-cov-percentile classifies on the host after the coverage filter", first, second);
        if (off.empty() && o.column.size() > sizeof opt.column) off = "a column separator of more than 16 bytes";
        if (!off.empty() || !set_format_tables(S.ctx, o, S.tx, off) || (matchesToo && !set_matches_table(S.ctx, o, S.tx, off))) return;
        ctx = S.ctx;
        allhits = matchesToo; matchFlags = MC_FORMAT_HOST | (o.lowest == 0 ? MC_MATCHES_WINDOWS : 0);
        std::memcpy(opt.column, o.column.data(), o.column.size());
        opt.column_len = (uint32_t)o.column.size(); opt.win_stride = S.dbStride; opt.win_len = S.dbWinlen;
        vote = mc_classify_options{(uint32_t)o.hitsMin, o.hitsDiff, o.lowest, o.highest};
        flags = MC_FORMAT_HOST | (o.queryIds ? MC_FORMAT_QUERY_IDS : 0) | (o.showGroundTruth ? MC_FORMAT_TRUTH : 0) | (o.tophits ? MC_FORMAT_TOPHITS : 0) |
                (o.locations ? MC_FORMAT_LOCATIONS : 0) | (o.mapView == Options::mv_mapped ? MC_FORMAT_MAPPED_ONLY : 0);
    }
    void report(const Profile& P) const
    {
        DeviceStep::report(P, "mapping lines on the device: " + std::to_string(calls) + " mc_format_mappings calls, " + std::to_string(reads) + " reads, " + std::to_string(lines) + " lines, ",
                           " batches formatted on the host", "mapping lines formatted on the host");
        if (P.on && ctx && allhits)
            std::cerr << "mcq profile: all-hits columns on the device: " << matchCalls << " mc_format_matches calls, " << matchReads << " reads, " << matchBytes << " bytes\n";
    }
};
struct FormatClient {                        // a worker's batch as the library takes it, and what comes back
    FormatStep* step = nullptr;              // (null: the host loop classifies and prints read by read)
    std::vector<mc_candidate> rows; std::vector<mc_assignment> assigned; std::vector<uint32_t> truth;
    std::vector<uint64_t> ids, nameOff, lineOff; std::string names, bytes;
    std::vector<mc_location> locs; std::vector<uint64_t> locOff, pieceOff; std::string pieces;   // (-allhits: the reads' lists, flat, and their rendered column)
    std::vector<Cand> cands;                 // (one read's, for -hits-per-ref)
    // One batch through the library: what the writer L (MappingWriter) does read by read -- vote, tallies, line -- for all its reads at once.
    // false: a call failed (the step says why) and NOTHING of the batch was counted or written, so that the caller's host loop does the whole batch.
    template <class OS, class Queries, class Writer>
    bool lines(OS& out, const Queries& queries, const mc_results& r, Writer& L)
    {
        const Options& o = L.o;
        const uint32_t K = r.max_candidates;
        rows.clear(); ids.clear(); truth.clear(); names.clear(); nameOff.assign(1, 0);
        locs.clear(); locOff.assign(1, 0);
        for (uint32_t i = 0; i < r.num_queries; ++i) {
            const auto& m = queries[i];
            if (m.empty) continue;                                   // processQuery, classification.cpp:780
            rows.insert(rows.end(), r.cands + (size_t)i * K, r.cands + (size_t)(i + 1) * K);
            ids.push_back(m.id);
            const void* sp = memchr(m.header.p, ' ', m.header.n);
            names.append(m.header.p, sp ? (size_t)((const char*)sp - m.header.p) : m.header.n);
            nameOff.push_back(names.size());
            if (o.determineGroundTruth) truth.push_back(ground_truth(L.tx, std::string(m.header.p, m.header.n)));
            if (step->allhits) { locs.insert(locs.end(), r.hits + r.hit_offsets[i], r.hits + r.hit_offsets[i + 1]); locOff.push_back(locs.size()); }
        }
        const size_t n = ids.size();
        if (n == 0) return true;
        assigned.resize(n);
        if (mc_classify_candidates(step->ctx, &step->vote, rows.data(), (uint32_t)n, K, MC_CLASSIFY_HOST, assigned.data(), nullptr) != MC_OK) { step->note(mc_last_error(step->ctx)); return false; }
        if (step->allhits) {                                         // the all-hits column first: its pieces go into the lines
            pieceOff.resize(n + 1);
            if (pieces.size() < locs.size() * 8 + 16) pieces.resize(locs.size() * 8 + 16);
            auto column = [&]() { return mc_format_matches(step->ctx, locs.data(), locOff.data(), (uint32_t)n, step->matchFlags, &pieces[0], pieces.size(), pieceOff.data(), nullptr); };
            int mrc = column();
            if (mrc == MC_ERR_NOMEM) { pieces.resize(pieceOff[n] + pieceOff[n] / 4); mrc = column(); }   // (piece_off came back complete: now they fit)
            if (mrc != MC_OK) { step->note(mc_last_error(step->ctx)); return false; }
        }
        lineOff.resize(n + 1);
        if (bytes.size() < n * 128) bytes.resize(n * 128);
        auto render = [&]() {
            return mc_format_mappings_with(step->ctx, &step->opt, rows.data(), K, assigned.data(), (step->flags & MC_FORMAT_TRUTH) ? truth.data() : nullptr,
                                           ids.data(), 0, names.data(), nameOff.data(), (uint32_t)n, step->flags, &bytes[0], bytes.size(), lineOff.data(), nullptr,
                                           step->allhits ? pieces.data() : nullptr, step->allhits ? pieceOff.data() : nullptr);
        };
        int rc = render();
        if (rc == MC_ERR_NOMEM) { bytes.resize(lineOff[n] + lineOff[n] / 4); rc = render(); }      // (line_off came back complete: now they fit)
        if (rc != MC_OK) { step->note(mc_last_error(step->ctx)); return false; }
        uint64_t printed = 0;
        for (size_t j = 0; j < n; ++j) {
            printed += lineOff[j + 1] > lineOff[j];
            if (o.hitsPerRef) device_candidates(&rows[j * K], K, L.tx, o.lowest, cands);
            L.count_read(ids[j], assigned[j], o.determineGroundTruth ? truth[j] : 0, cands);
        }
        out.write(bytes.data(), (std::streamsize)lineOff[n]);
        step->took(n, printed);
        if (step->allhits) step->took_matches(n, pieceOff[n]);
        return true;
    }
};

// ---- parse (mc_batch_add_file_bytes): a batch's reads cut out of the file's bytes on the device ---------------------------
// MCQ_PARSE_DEVICE=1; =2 means the same, and -pairfiles batches too, as two ranges through mc_batch_add_file_mates (7h.1).
// The host index (SeqFile) stays: it numbers the queries, cuts the batches and hands irregular files to its exact
// reader.  A batch whose records all come from the fast scan of a plain mapped file goes to its slot as ONE byte range; the library cuts
// it, and the step takes the headers' places and the reads' lengths from mc_batch_records.  Whatever the device refuses, a record count
// that differs from the index's, or a range the slot cannot take leaves the WHOLE batch to the host loop (SlotStep).
struct ParseStep : DeviceStep {
    uint64_t bytes = 0, records = 0; int flags = 0;
    void took(uint64_t nbytes, uint64_t nrecords) { std::lock_guard<std::mutex> g(mtx); ++calls; bytes += nbytes; records += nrecords; }
    static bool any_gzip(const Options& o)
    {
        for (const std::string& f : o.infiles) {
            unsigned char m[2] = {0, 0};
            std::ifstream is(f, std::ios::binary);
            if (is.read((char*)m, 2) && m[0] == 0x1f && m[1] == 0x8b) return true;
        }
        return false;
    }
    void open(const Session& S, const Options& o, bool merged)
    {
        const char* sw = std::getenv("MCQ_PARSE_DEVICE");
        if (!sw || std::atoi(sw) == 0) return;
        const bool selects = o.minReadLen > 0 || o.maxReadLen < std::numeric_limits<uint64_t>::max() || o.queryLimit < ((int64_t)1 << 62);
        const char* first = (o.pairing == Options::files && std::atoi(sw) < 2) ? "-pairfiles: a query's two reads lie in two files"
                          : selects ? "length filters and -query-limit select the reads on the host"
                          : any_gzip(o) ? "gzip input is inflated on the host" : nullptr;
        off = shared_host_reason(S, merged, false, "", first);
        if (!off.empty()) return;
        ctx = S.ctx;
        flags = o.pairing == Options::sequences ? MC_PARSE_PAIRS : 0;
    }
    void report(const Profile& P) const
    {
        DeviceStep::report(P, "reads parsed on the device: " + std::to_string(calls) + " batches, " + std::to_string(bytes) + " bytes, " + std::to_string(records) + " records, ",
                           " batches parsed on the host", "reads parsed on the host");
    }
};

// ---- inflate (mc_bgzf_index + mc_inflate_blocks): BGZF input inflated on the device ---------------------------------
// MCQ_INFLATE_DEVICE=1.  A compressed input file is mapped and indexed on the host; a BGZF file goes to mc_inflate_blocks(MC_INFLATE_HOST)
// and into a buffer sized once from the index.  A file that is not BGZF, a verdict other than MC_INFLATE_OK and any library error leave
// the file to SeqFile's gzread loop; the step keeps every such file with its reason.  Everything behind the bytes is unchanged -- inflated
// input still does not take the device parse (SeqFile::byte_range).  build, modify and the reference files of -align never ask.
struct InflateStep : DeviceStep {
    uint64_t files = 0, blocks = 0, bytesIn = 0, bytesOut = 0;
    std::vector<std::string> left;           // the files left to the host, each with its reason
    GzInflater inflater;                     // empty: SeqFile inflates
    static bool wanted() { const char* sw = std::getenv("MCQ_INFLATE_DEVICE"); return sw && std::atoi(sw) != 0; }
    void open(const Session& S, bool merged)
    {
        if (!wanted()) return;
        off = shared_host_reason(S, merged, false, "", S.built ? "build+query" : nullptr);
        if (!off.empty()) return;
        ctx = S.ctx;
        inflater = [this](const std::string& fn, const unsigned char* bytes, size_t n, std::vector<char>& out, size_t& size) { return run(fn, bytes, n, out, size); };
    }
    bool leave(const std::string& fn, const std::string& why) { std::lock_guard<std::mutex> g(mtx); left.push_back(fn + ": " + why); return false; }
    bool run(const std::string& fn, const unsigned char* bytes, size_t n, std::vector<char>& out, size_t& size)
    {
        uint64_t info[4] = {0, 0, 0, 0}, status[4] = {0, 0, 0, 0};
        if (mc_bgzf_index(bytes, n, nullptr, 0, info) != MC_OK) return leave(fn, mc_last_error(nullptr));
        if (info[2] != MC_BGZF_OK) return leave(fn, "not BGZF at byte " + std::to_string(info[3]));
        std::vector<mc_bgzf_block> rows(info[0]);
        if (mc_bgzf_index(bytes, n, rows.data(), rows.size(), info) != MC_OK) return leave(fn, mc_last_error(nullptr));
        out.resize(std::max<uint64_t>(info[1], 1));
        if (mc_inflate_blocks(ctx, bytes, n, rows.data(), rows.size(), MC_INFLATE_HOST, (uint8_t*)out.data(), info[1], status, nullptr) != MC_OK) return leave(fn, mc_last_error(ctx));
        if (status[0] != MC_INFLATE_OK) return leave(fn, "the device refused block " + std::to_string(status[1]) + " (verdict " + std::to_string(status[0]) + ", reason " + std::to_string(status[2]) + ")");
        size = (size_t)info[1];
        std::lock_guard<std::mutex> g(mtx);
        ++files; blocks += rows.size(); bytesIn += n; bytesOut += info[1];
        return true;
    }
    void report(const Profile& P) const
    {
        if (!P.on) return;
        if (ctx) {
            std::cerr << "mcq profile: gzip input inflated on the device: " << files << " files, " << blocks << " blocks, " << bytesIn << " bytes in, " << bytesOut << " bytes out, "
                      << left.size() << " files left to the host";
            for (size_t i = 0; i < left.size(); ++i) std::cerr << (i ? "; " : " (") << left[i];
            std::cerr << (left.empty() ? "\n" : ")\n");
        } else if (!off.empty()) std::cerr << "mcq: gzip input inflated on the host (" << off << ")\n";
    }
};

// ---- input (mc_input_*): a query file resident on the device, its batches cut there -----------------------------------
// MCQ_INPUT_DEVICE=1.  The producer hands every input file to take(): the file is mapped, the library makes it resident (a plain file is
// uploaded, a BGZF file inflated on the device), cuts it in pieces of at most MCQ_INPUT_DEVICE_PIECE bytes and gives the batches; the
// workers feed them to their slots as device ranges (SlotStep::resident), and a file's buffer is freed when its last batch has been
// cleared.  All resident input alive at once stays below MCQ_INPUT_DEVICE_MB (default 8192): the producer waits for earlier files'
// batches instead.  A file that does not go resident takes the old path unchanged and is named with its reason; one that was inflated
// on the device and then refused (irregular) is copied back once and handed to SeqFile as InflateStep hands its files over.
struct ResidentFile { mc_input* in = nullptr; const char* dev = nullptr; uint64_t bytes = 0; std::atomic<size_t> left{0}; };

struct InputStep : DeviceStep {
    uint64_t files = 0, pieces = 0, batches = 0, bytes = 0, records = 0;
    std::vector<std::string> leftFiles;      // the files left to the host, each with its reason
    uint64_t capBytes = 0, pieceBytes = 0, slotBytes = 0; int flags = 0; uint32_t perBatch = 0;
    std::mutex resMu; std::condition_variable resCv; uint64_t residentBytes = 0;   // (under resMu)
    std::deque<std::unique_ptr<ResidentFile>> residents;                            // (the producer appends; addresses stay)

    static uint64_t env_u64(const char* name, uint64_t dflt) { const char* v = std::getenv(name); return v && *v ? std::strtoull(v, nullptr, 10) : dflt; }
    void open(const Session& S, const Options& o, bool merged, bool covMode, bool aligning)
    {
        const char* sw = std::getenv("MCQ_INPUT_DEVICE");
        if (!sw || std::atoi(sw) == 0) return;
        const bool selects = o.minReadLen > 0 || o.maxReadLen < std::numeric_limits<uint64_t>::max() || o.queryLimit < ((int64_t)1 << 62);
        const char* first = o.pairing == Options::files ? "-pairfiles: a query's two reads lie in two files"
                          : selects ? "length filters and -query-limit select the reads on the host"
                          : aligning ? "-align needs the reads' characters on the host"
                          : S.built ? "build+query" : nullptr;
        off = shared_host_reason(S, merged, covMode, "-cov-percentile keeps the reads' headers beyond their batches", first);
        if (!off.empty()) return;
        ctx = S.ctx;
        flags = o.pairing == Options::sequences ? MC_PARSE_PAIRS : 0;
        perBatch = (uint32_t)(o.batchSize * (flags ? 2 : 1));
        capBytes = env_u64("MCQ_INPUT_DEVICE_MB", 8192) << 20;
        pieceBytes = std::max<uint64_t>(1, std::min<uint64_t>(env_u64("MCQ_INPUT_DEVICE_PIECE", 1ull << 31), 1ull << 31));
        slotBytes = S.cfg.slot_max_chars;
    }
    bool leave(const std::string& fn, const std::string& why) { std::lock_guard<std::mutex> g(mtx); leftFiles.push_back(fn + ": " + why); return false; }

    // true: the file is resident (rf, rows).  false: it takes the old path -- with `plain` filled where the device inflated it already
    bool take(const std::string& fn, const std::atomic<bool>& stopped, ResidentFile*& rf, std::vector<mc_input_batch>& rows, std::vector<char>& plain)
    {
        const int fd = ::open(fn.c_str(), O_RDONLY);
        struct stat st;
        if (fd < 0 || fstat(fd, &st) != 0) { if (fd >= 0) ::close(fd); return false; }          // (SeqFile reports it)
        struct Mapping { int fd; void* m; size_t n; ~Mapping() { if (m != MAP_FAILED) munmap(m, n); ::close(fd); } } map{fd, MAP_FAILED, (size_t)st.st_size};
        if (map.n == 0) return leave(fn, "no bytes");
        map.m = mmap(nullptr, map.n, PROT_READ, MAP_PRIVATE, fd, 0);
        if (map.m == MAP_FAILED) return leave(fn, "cannot be mapped");
        const unsigned char* B = (const unsigned char*)map.m;
        uint64_t need = map.n;
        if (map.n >= 2 && B[0] == 0x1f && B[1] == 0x8b) {
            uint64_t bi[4] = {0, 0, 0, 0};
            if (mc_bgzf_index(B, map.n, nullptr, 0, bi) != MC_OK) return leave(fn, mc_last_error(nullptr));
            if (bi[2] != MC_BGZF_OK) return leave(fn, "plain gzip: not BGZF at byte " + std::to_string(bi[3]));
            need = bi[1];
        }
        if (need > capBytes) return leave(fn, "larger than the cap of " + std::to_string(capBytes >> 20) + " MiB (MCQ_INPUT_DEVICE_MB)");
        {   // the producer waits for earlier files' batches instead of exceeding the cap
            std::unique_lock<std::mutex> l(resMu);
            while (residentBytes && residentBytes + need > capBytes && !stopped) resCv.wait_for(l, std::chrono::milliseconds(20));
            if (stopped) return false;
        }
        uint64_t info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        mc_input* in = nullptr;
        if (mc_input_open(ctx, B, map.n, flags, perBatch, pieceBytes, slotBytes, capBytes, &in, info) != MC_OK) return leave(fn, mc_last_error(ctx));
        if (info[0] != MC_INPUT_OK) {
            if (in) {                                                     // inflated on the device, then refused: copied back once
                plain.resize(info[2]);
                if (mc_input_download(in, plain.data(), plain.size()) != MC_OK) plain.clear();
                mc_input_close(in);
            }
            switch (info[0]) {
            case MC_INPUT_NOT_BGZF: return leave(fn, "plain gzip: not BGZF at byte " + std::to_string(info[1]));
            case MC_INPUT_REFUSED: return leave(fn, "the device refused block " + std::to_string(info[1]) + " (verdict " + std::to_string(info[6]) + ", reason " + std::to_string(info[7]) + ")");
            case MC_INPUT_TOO_LARGE: return leave(fn, "larger than the cap of " + std::to_string(capBytes >> 20) + " MiB (MCQ_INPUT_DEVICE_MB)");
            case MC_INPUT_NO_MEMORY: return leave(fn, "no device memory for " + std::to_string(info[1]) + " bytes");
            case MC_INPUT_IRREGULAR: return leave(fn, "irregular at byte " + std::to_string(info[1]));
            case MC_INPUT_RECORD_TOO_LARGE: return leave(fn, "a record does not fit the largest piece");
            default: return leave(fn, "no bytes");
            }
        }
        rows.resize(info[4]);
        const void* dev = nullptr; uint64_t n = 0;
        if (mc_input_batches(in, rows.data(), rows.size(), &dev, &n) != MC_OK || rows.empty()) { mc_input_close(in); return leave(fn, "no records"); }
        residents.emplace_back(new ResidentFile);
        rf = residents.back().get();
        rf->in = in; rf->dev = (const char*)dev; rf->bytes = n; rf->left = rows.size();
        { std::lock_guard<std::mutex> l(resMu); residentBytes += n; }
        std::lock_guard<std::mutex> g(mtx);
        ++files; pieces += info[3]; batches += rows.size(); bytes += n; records += info[5];
        return true;
    }
    // a batch of rf has been cleared (or will never be submitted): the last one frees the file's buffer
    void done(ResidentFile* rf)
    {
        if (rf->left.fetch_sub(1) != 1) return;
        mc_input_close(rf->in);
        rf->in = nullptr;
        { std::lock_guard<std::mutex> l(resMu); residentBytes -= rf->bytes; }
        resCv.notify_all();
    }
    ~InputStep() { for (auto& r : residents) if (r->in) mc_input_close(r->in); }   // (a job that failed: batches that were never taken)
    void report(const Profile& P) const
    {
        if (!P.on) return;
        if (ctx) {
            std::cerr << "mcq profile: input resident on the device: " << files << " files, " << pieces << " pieces, " << batches << " batches, " << bytes << " bytes, " << records
                      << " records, " << leftFiles.size() << " files left to the host";
            for (size_t i = 0; i < leftFiles.size(); ++i) std::cerr << (i ? "; " : " (") << leftFiles[i];
            std::cerr << (leftFiles.empty() ? "\n" : ")\n");
        } else if (!off.empty()) std::cerr << "mcq: query input read on the host (" << off << ")\n";
    }
};

// ---- merge (mc_merge_results_*): `mcq merge` hands its result files to the library -----------------------------------
// MCQ_MERGE_DEVICE=1.  The host reads a file's leading comment block (results_head: its checks and errors, the column of the top hits),
// the rest goes to mc_merge_results_add in ranges of at most 2^31 bytes cut at line starts; afterwards the lists, the header places and
// the assignments come back and fill MergedInput.  Any verdict other than MC_MERGE_OK (after one reserve + retry for
// MC_MERGE_OVERFLOW) and any library error leave the WHOLE merge to the host path; `why` says which file, verdict and offence.
struct MergeFile { std::string name; const char* data = nullptr; size_t size = 0, body = 0; int tophitsColumn = 0; };   // body: the first byte behind the leading comment block
struct MergeStep {
    bool on = false;
    std::string why;                         // on and not merged by the library: why
    uint64_t files = 0, lines = 0, entries = 0, unknown = 0;
    MergeStep() { const char* sw = std::getenv("MCQ_MERGE_DEVICE"); on = sw && std::atoi(sw) != 0; }

    static uint64_t count_char(const char* p, size_t n, char c)
    {
        uint64_t k = 0;
        for (const char* q = p, *e = p + n; (q = (const char*)memchr(q, c, (size_t)(e - q))) != nullptr; ++q) ++k;
        return k;
    }
    static uint64_t count_result_lines(const char* p, size_t n)   // line starts that hold no '#'
    {
        uint64_t k = 0;
        for (size_t s = 0; s < n;) {
            if (p[s] != '#') ++k;
            const char* nl = (const char*)memchr(p + s, '\n', n - s);
            if (!nl) break;
            s = (size_t)(nl - p) + 1;
        }
        return k;
    }

    bool run(const Options& o, const Taxonomy& tx, const std::vector<MergeFile>& in, size_t maxCand, MergedInput& M)
    {
        mc_config cfg;
        mc_config_default(&cfg);
        cfg.device = o.gpus.empty() ? 0 : o.gpus[0];
        mc_ctx* ctx = nullptr;
        if (mc_create(&cfg, &ctx) != MC_OK) { why = mc_last_error(nullptr); return false; }
        struct Closer { mc_ctx* c; ~Closer() { mc_merge_results_end(c); mc_destroy(c); } } closer{ctx};
        auto failed = [&](const std::string& what) { why = what; return false; };
        auto lib_failed = [&] { return failed(mc_last_error(ctx)); };
        // the taxonomy as arrays: every taxon's ranked lineage, rank, covers, and its taxid
        const size_t nt = tx.taxa.size();
        std::vector<uint32_t> lin(nt * kNumRanks);
        std::vector<uint8_t> rank(nt), covered(nt);
        std::vector<int64_t> ids(nt);
        for (size_t i = 0; i < nt; ++i) {
            const Lineage l = tx.ranks_of((uint32_t)i + 1);
            std::copy(l.begin(), l.end(), lin.begin() + i * kNumRanks);
            rank[i] = (uint8_t)std::min(tx.taxa[i].rank, kNumRanks);
            covered[i] = tx.covers((uint32_t)i + 1) ? 1 : 0;
            ids[i] = tx.taxa[i].id;
        }
        if (mc_set_taxon_table(ctx, lin.data(), rank.data(), covered.data(), nt) != MC_OK || mc_merge_results_set_taxids(ctx, ids.data(), nt) != MC_OK) return lib_failed();
        uint64_t capacity = 1;
        for (const MergeFile& f : in) capacity = std::max<uint64_t>(capacity, count_char(f.data + f.body, f.size - f.body, '\n') + 1);
        if (mc_merge_results_begin(ctx, capacity, (uint32_t)maxCand, o.lowest) != MC_OK) return lib_failed();
        struct Call { size_t file, base; };
        std::vector<Call> calls;                                                // by call number: where the range lies
        constexpr size_t kRange = (size_t)1 << 31;
        for (size_t fi = 0; fi < in.size(); ++fi) {
            const MergeFile& f = in[fi];
            const char* p = f.data + f.body;
            const size_t n = f.size - f.body;
            if (n == 0) return failed(f.name + ": nothing behind the leading comment block");
            const uint64_t fileLines = n <= kRange ? 0 : count_result_lines(p, n);
            for (size_t pos = 0; pos < n;) {
                size_t len = std::min(n - pos, kRange);
                if (pos + len < n) {
                    const void* nl = memrchr(p + pos, '\n', len);
                    if (!nl) return failed(f.name + ": a line of more than 2^31 bytes");
                    len = (size_t)((const char*)nl - (p + pos)) + 1;
                }
                uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                for (int attempt = 0;; ++attempt) {
                    calls.push_back(Call{fi, f.body + pos});
                    if (mc_merge_results_add(ctx, p + pos, len, (uint32_t)f.tophitsColumn, fileLines, MC_MERGE_HOST | (pos ? MC_MERGE_CONTINUE : 0), st, nullptr, 0, nullptr) != MC_OK) return lib_failed();
                    if (st[5] != MC_MERGE_OVERFLOW || attempt == 1) break;
                    if (mc_merge_results_reserve(ctx, st[7]) != MC_OK) return lib_failed();
                    capacity = std::max<uint64_t>(capacity, st[7]);
                }
                if (st[5] != MC_MERGE_OK)
                    return failed(f.name + ": " + (st[5] == MC_MERGE_IRREGULAR ? "irregular line at offset " + std::to_string(f.body + pos + st[6]) : "overflow, " + std::to_string(st[7]) + " lists needed"));
                lines += st[0]; entries += st[3]; unknown += st[4];
                pos += len;
            }
            ++files;
        }
        uint64_t nq = 0;
        if (mc_merge_results_lists(ctx, 0, 0, MC_MERGE_HOST, nullptr, nullptr, &nq, nullptr) != MC_OK) return lib_failed();
        std::vector<mc_taxon_candidate> lists(nq * maxCand);
        std::vector<uint32_t> places(nq * 3);
        std::vector<mc_assignment> assigned(nq);
        mc_classify_options co;
        co.hits_min = (uint32_t)o.hitsMin; co.hits_diff = o.hitsDiff; co.lowest_rank = o.lowest; co.highest_rank = o.highest;
        if (nq && (mc_merge_results_lists(ctx, 0, nq, MC_MERGE_HOST, lists.data(), places.data(), nullptr, nullptr) != MC_OK ||
                   mc_merge_results_classify(ctx, &co, MC_CLASSIFY_HOST, 0, nq, assigned.data(), nullptr) != MC_OK)) return lib_failed();
        M.cands.assign(nq, {}); M.headers.assign(nq, std::string());
        for (uint64_t q = 0; q < nq; ++q) {
            for (size_t j = 0; j < maxCand && lists[q * maxCand + j].hits != 0; ++j)
                M.cands[q].push_back(Cand{0xFFFFFFFFu, lists[q * maxCand + j].hits, 0, 0, lists[q * maxCand + j].taxon});
            const uint32_t* h = &places[3 * q];
            if (h[2]) { const Call& c = calls[h[0]]; M.headers[q].assign(in[c.file].data + c.base + h[1], h[2]); }
        }
        M.assigned = std::move(assigned);
        return true;
    }
    // the device's line under MCQ_PROFILE; the fall-back's line also wherever the info level is not silent: the switch was set
    void report(const Profile& P, bool done, bool info) const
    {
        if (!on || (done ? !P.on : !(P.on || info))) return;
        if (done) std::cerr << "mcq profile: result files merged on the device: " << files << " files, " << lines << " lines, " << entries << " entries, " << unknown
                            << " unknown taxids, 0 files left to the host\n";
        else std::cerr << "mcq: result files merged on the host (" << why << ")\n";
    }
};

#endif  // MCQ_DEVICE_STEPS_H_
