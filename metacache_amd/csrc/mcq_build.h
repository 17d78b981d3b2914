// mcq_build.h -- `metacache build` (and the build half of `build+query`) on MI355X: reference sequences -> database, host C++14 above
// the C ABI's builder (mc_build_*: sketching, sorting and bucketising run on the GPU, builder.hip).  SURVEY.md §8f rank 1.  Mirrors
//   option handling       options.cpp:251-265 (database name), :298-370 (info level, id format, taxonomy), :375-485 (sketching, storage),
//                         :490-520 (augment_taxonomy_options), :535-640 (build mode), :1498-1575 (build+query: -targets / -query / -save-db)
//   taxonomy dumps        taxonomy_io.cpp:55-175 (names.dmp, merged.dmp, nodes.dmp -> non-target taxa), taxonomy.hpp:182-221 (rank names)
//   sequence -> taxon id  taxonomy_io.cpp:180-318 (assembly_summary tables), building.cpp:80-150 (*.accession2taxid after the build),
//                         :196-232 (try_to_rank_unranked_targets), :240-262 (find_taxon_id)
//   adding targets        building.cpp:283-327 (one sequence), :335-455 (all files; here: files and records in the given order = the
//                         reference's single-part build), database.cpp:36-82 (ids, names of duplicates), sequence_io.cpp:470-673 (ids)
//   post-processing       building.cpp:516-534 (-remove-overpopulated-features), :550-566 (-remove-ambig-features)
// Not offered:
// -parts > 1 (the reference spreads targets over parts in thread-schedule order; the multi-GPU modes use key shards instead).
#ifndef MCQ_BUILD_H_
#define MCQ_BUILD_H_
#include "mcq_common.h"

#include <set>

namespace mcq {

enum class IdType { smart, ncbi, genbank, filename, leading_word };

inline std::string trimmed(std::string s)
{
    size_t b = 0, e = s.size();
    while (b < e && std::isspace((unsigned char)s[b])) ++b;
    while (e > b && std::isspace((unsigned char)s[e - 1])) --e;
    return s.substr(b, e - b);
}

inline std::string ncbi_accession_number(const std::string& text)             // sequence_io.cpp:541-573
{
    if (text.empty()) return "";
    std::smatch m;
    std::regex_search(text, m, accession_regex());
    return m[2];
}

inline std::string genbank_identifier(const std::string& text)                // sequence_io.cpp:581-603
{
    if (text.empty()) return "";
    auto i = text.find("gi|");
    if (i == std::string::npos) i = text.find("gi:");
    if (i == std::string::npos) i = text.find("gi=");
    if (i == std::string::npos) return "";
    i += 3;
    auto j = text.find('|', i);
    if (j == std::string::npos) { j = text.find(' ', i); if (j == std::string::npos) j = text.size(); }
    return trimmed(text.substr(i, j - i));
}

inline std::string accession_string(const std::string& text, IdType t)        // extract_accession_string, sequence_io.cpp:608-642
{
    if (text.empty()) return "";
    switch (t) {
        case IdType::ncbi: return ncbi_accession_number(text);
        case IdType::genbank: return genbank_identifier(text);
        case IdType::leading_word: return leading_word(text);
        case IdType::filename: return filename_without_extension(text);
        case IdType::smart: {
            auto s = ncbi_accession_number(text);
            if (!s.empty()) return s;
            s = genbank_identifier(text);
            if (!s.empty()) return s;
            s = filename_without_extension(text);
            if (!s.empty()) return s;
        }
    }
    return text;
}

struct BuildOptions {
    std::string dbfile;
    std::vector<std::string> infiles;
    std::string taxPath;
    std::vector<std::string> mapPost;               // -taxpostmap + the defaults of augment_taxonomy_options
    IdType idType = IdType::smart;
    enum Info { silent, moderate, verbose } info = moderate;
    uint32_t k = 16, s = 16, w = 127, stride = 0;   // options.hpp:102
    bool resetParents = false, removeOverpopulated = false, saveDb = false;
    int maxLocs = -1, parts = 1, targetIdBytes = 4;
    int shards = 0;                                 // key shards of the build (0 = from the input size: one device sort takes 2^32 pairs)
    float maxLoadFac = -1;
    int removeAmbigRank = kNumRanks;
    int maxAmbig = 1;                                        // options.hpp:78
    bool modify = false, maxLocsGiven = false;      // modify mode: the database <dbfile> is read first (mode_build.cpp:74-88)
};

// args: everything after the mode word.  build: <database> <files>... ; build+query: -targets <files>... [-query <files>...] and every
// word this parser does not know goes to the query parser (queryArgs).
inline BuildOptions parse_build(const std::vector<std::string>& args, bool buildQuery, std::vector<std::string>& queryArgs)
{
    BuildOptions o;
    bool haveDb = buildQuery;
    auto need = [&](size_t& i) -> std::string { if (i + 1 >= args.size()) throw std::runtime_error("value missing after '" + args[i] + "'"); return args[++i]; };
    auto values = [&](size_t& i, std::vector<std::string>& dst) { while (i + 1 < args.size() && !args[i + 1].empty() && args[i + 1][0] != '-') dst.push_back(args[++i]); };
    auto set_db = [&](std::string name) {                                      // sanitize_database_name, options.cpp:110-128
        auto pos = name.find(".meta");
        if (pos != std::string::npos) name.erase(pos);
        else { pos = name.find(".cache"); if (pos != std::string::npos) name.erase(pos); }
        o.dbfile = name;
    };
    for (size_t i = 0; i < args.size(); ++i) {
        const std::string& a = args[i];
        if (a.empty()) continue;
        if (a[0] != '-') {
            if (!haveDb) { set_db(a); haveDb = true; }
            else if (!buildQuery) o.infiles.push_back(a);
            else queryArgs.push_back(a);
            continue;
        }
        if (a == "-targets" && buildQuery) values(i, o.infiles);
        else if (a == "-query" && buildQuery) values(i, queryArgs);
        else if (a == "-save-db" && buildQuery) { set_db(need(i)); o.saveDb = true; }
        else if (a == "-taxonomy") o.taxPath = need(i);
        else if (a == "-taxpostmap") values(i, o.mapPost);
        else if (a == "-sequence-id-format") {
            const std::string v = need(i);
            if (v == "smart") o.idType = IdType::smart; else if (v == "ncbi") o.idType = IdType::ncbi;
            else if (v == "gi") o.idType = IdType::genbank; else if (v == "filename") o.idType = IdType::filename;
            else if (v == "leadingword") o.idType = IdType::leading_word;
            else throw std::runtime_error("unknown sequence id format '" + v + "'");
        }
        else if (a == "-silent") o.info = BuildOptions::silent;
        else if (a == "-verbose") o.info = BuildOptions::verbose;
        else if (a == "-kmerlen") o.k = (uint32_t)std::stoul(need(i));
        else if (a == "-sketchlen") o.s = (uint32_t)std::stoul(need(i));
        else if (a == "-winlen") o.w = (uint32_t)std::stoul(need(i));
        else if (a == "-winstride") o.stride = (uint32_t)std::stoul(need(i));
        else if (a == "-reset-taxa" || a == "-reset-parents") o.resetParents = true;
        else if (a == "-max-locations-per-feature") { o.maxLocs = std::stoi(need(i)); o.maxLocsGiven = true; }
        else if (a == "-remove-overpopulated-features") o.removeOverpopulated = true;
        else if (a == "-remove-ambig-features") { o.removeAmbigRank = rank_from_name(need(i)); if (o.removeAmbigRank < 0) throw std::runtime_error("unknown rank"); }
        else if (a == "-max-ambig-per-feature") o.maxAmbig = std::stoi(need(i));
        else if (a == "-max-load-fac" || a == "-max-load-factor") o.maxLoadFac = std::stof(need(i));
        else if (a == "-parts") o.parts = std::stoi(need(i));
        else if (a == "-max-part-size") (void)need(i);
        else if (a == "-target-id-type") {                                    // the reference's compile-time MC_TARGET_ID_TYPE (config.hpp:57-61)
            const std::string v = need(i);
            if (v == "uint16_t" || v == "16") o.targetIdBytes = 2; else if (v == "uint32_t" || v == "32") o.targetIdBytes = 4;
            else throw std::runtime_error("target id type must be uint16_t or uint32_t");
        }
        else if (a == "-build-shards") o.shards = std::stoi(need(i));          // not a reference option: see BuildOptions::shards
        else if (a == "-threads" && !buildQuery) (void)need(i);               // accepted: sketching and sorting run on the GPU
        else if (buildQuery) queryArgs.push_back(a);
        else throw std::runtime_error("unknown option '" + a + "'");
    }
    if (!buildQuery && o.dbfile.empty()) throw std::runtime_error("Database name is missing");
    // process_build_options (options.cpp:614-626)
    {
        std::vector<std::string> expanded;
        for (const auto& name : o.infiles) {
            auto sub = files_in_directory(name);
            if (sub.empty()) expanded.push_back(name); else expanded.insert(expanded.end(), sub.begin(), sub.end());
        }
        o.infiles.swap(expanded);
    }
    if (o.infiles.empty()) throw std::runtime_error("No reference sequence files provided or found");
    if (o.maxLocs < 0) o.maxLocs = 254;                                       // database::max_supported_locations_per_feature()
    if (o.stride == 0) o.stride = o.w - o.k + 1;
    if (o.parts > 1) throw std::runtime_error("-parts > 1 is not available: one part per build (see DESIGN.md, multi-GPU modes)");
    // augment_taxonomy_options (options.cpp:490-520)
    if (!o.taxPath.empty() && o.taxPath.back() != '/') o.taxPath += '/';
    for (const char* f : {"nucl_gb.accession2taxid", "nucl_wgs.accession2taxid", "nucl_est.accession2taxid", "nucl_gss.accession2taxid"})
        o.mapPost.push_back(o.taxPath + f);
    for (const auto& f : files_in_directory(o.taxPath))
        if (f.find(".accession2taxid") != std::string::npos && std::find(o.mapPost.begin(), o.mapPost.end(), f) == o.mapPost.end()) o.mapPost.push_back(f);
    return o;
}

// ---- taxonomy dumps (taxonomy_io.cpp:55-175): taxa above sequence level; the first record of an id wins (unordered_set::emplace) ----
struct TaxTree {
    std::vector<Taxon> taxa;
    std::unordered_map<int64_t, uint32_t> byId;
    bool emplace(int64_t id, int64_t parent, std::string name, int rank)
    {
        if (id == 0 || byId.count(id)) return false;
        Taxon t; t.id = id; t.parent = parent; t.rank = rank; t.name = std::move(name);
        byId.emplace(id, (uint32_t)taxa.size());
        taxa.push_back(std::move(t));
        return true;
    }
};

// fields of one "a\t|\tb\t|\tc\t|" row
inline std::vector<std::string> dump_fields(const std::string& line)
{
    std::vector<std::string> f;
    size_t p = 0;
    while (p <= line.size()) {
        size_t q = line.find('|', p);
        if (q == std::string::npos) q = line.size();
        std::string x = line.substr(p, q - p);
        while (!x.empty() && x.front() == '\t') x.erase(x.begin());
        while (!x.empty() && (x.back() == '\t' || x.back() == '\r')) x.pop_back();
        f.push_back(std::move(x));
        p = q + 1;
    }
    return f;
}

inline TaxTree read_taxonomy_dumps(const BuildOptions& o)
{
    const bool info = o.info != BuildOptions::silent;
    TaxTree tax;
    std::map<int64_t, std::string> names;
    {
        std::ifstream is(o.taxPath + "names.dmp");
        if (is.good()) {
            if (info) std::cout << "Reading taxon names ... " << std::flush;
            int64_t lastId = 0;
            for (std::string line; std::getline(is, line);) {
                auto f = dump_fields(line);
                if (f.size() < 4 || f[0].empty()) continue;
                int64_t id = 0;
                try { id = std::stoll(f[0]); } catch (std::exception&) { continue; }
                if (id == lastId) continue;                                    // a scientific name was already taken for this id
                if (leading_word(f[3]).find("scientific") != std::string::npos) { lastId = id; names.emplace(id, f[1]); }
            }
            if (info) std::cout << "done." << std::endl;
        } else if (info) std::cerr << "Could not read taxon names file " << o.taxPath << "names.dmp; continuing with ids only." << std::endl;
    }
    std::map<int64_t, int64_t> merged;
    {
        std::ifstream is(o.taxPath + "merged.dmp");
        if (is.good()) {
            if (info) std::cout << "Reading taxonomic node mergers ... " << std::flush;
            for (std::string line; std::getline(is, line);) {
                auto f = dump_fields(line);
                if (f.size() < 2 || f[0].empty()) continue;
                try {
                    const int64_t oldId = std::stoll(f[0]), newId = std::stoll(f[1]);
                    merged.emplace(oldId, newId);
                    tax.emplace(oldId, newId, "", kNumRanks);
                } catch (std::exception&) {}
            }
            if (info) std::cout << "done." << std::endl;
        }
    }
    {
        std::ifstream is(o.taxPath + "nodes.dmp");
        if (!is.good()) {
            if (info) std::cerr << "Could not read taxonomic nodes file " << o.taxPath << "nodes.dmp" << std::endl;
            return tax;
        }
        if (info) std::cout << "Reading taxonomic tree ... " << std::flush;
        for (std::string line; std::getline(is, line);) {
            auto f = dump_fields(line);
            if (f.size() < 3 || f[0].empty()) continue;
            int64_t id = 0, parent = 0;
            try { id = std::stoll(f[0]); parent = std::stoll(f[1]); } catch (std::exception&) { continue; }
            auto it = names.find(id);
            std::string name = it != names.end() ? it->second : std::string("--");
            if (name.empty()) name = "<" + std::to_string(id) + ">";
            auto mi = merged.find(id);
            if (mi != merged.end()) id = mi->second;
            mi = merged.find(parent);
            if (mi != merged.end()) parent = mi->second;
            tax.emplace(id, parent, std::move(name), rank_from_dump_name(f[2]));
        }
        if (info) std::cout << tax.taxa.size() << " taxa read." << std::endl;
    }
    auto root = tax.byId.find(1);
    if (root != tax.byId.end()) tax.taxa[root->second].rank = kNumRanks - 1;   // reset_rank(1, root)
    return tax;
}

// ---- sequence id -> taxon id tables (taxonomy_io.cpp:180-318) ----
inline void read_id_table(const std::string& file, std::map<std::string, int64_t>& map, bool info)
{
    std::ifstream is(file);
    if (!is.good()) return;
    if (info) std::cout << "Reading sequence to taxon mappings from " << file << std::endl;
    std::vector<std::string> lines;
    for (std::string l; std::getline(is, l);) lines.push_back(std::move(l));
    // header row = the last of the leading '#' lines (at most 10 are looked at)
    int headerRow = 0;
    for (int i = 0; i < 10; ++i, ++headerRow) { if (i >= (int)lines.size() || lines[i].empty() || lines[i][0] != '#') break; }
    if (headerRow > 0) --headerRow;
    if (headerRow >= (int)lines.size()) return;
    int keycol = 0, taxcol = 0;
    {
        std::istringstream hs(lines[headerRow]);
        int col = 0;
        for (std::string h; hs >> h; ++col) {
            if (h.size() == 1 && h[0] == '#') hs >> h;
            if (h == "taxid") taxcol = col;
            else if (h == "accession.version" || h == "assembly_accession") keycol = col;
        }
    }
    size_t first = (size_t)headerRow + 1;
    if (taxcol < 1) { taxcol = 1; first = 0; }                                // no header: 1st column = key, 2nd = taxon id, from the top
    for (size_t r = first; r < lines.size(); ++r) {
        // the reference moves 'keycol' tabs forward, reads the key, then 'taxcol' MORE tabs forward (taxonomy_io.cpp:271-277)
        const std::string& l = lines[r];
        size_t p = 0;
        bool ok = true;
        for (int i = 0; i < keycol && ok; ++i) { auto t = l.find('\t', p); if (t == std::string::npos) ok = false; else p = t + 1; }
        if (!ok) continue;
        const std::string key = leading_word(l.substr(p));
        size_t q = l.find(key, p) + key.size();
        for (int i = 0; i < taxcol && ok; ++i) { auto t = l.find('\t', q); if (t == std::string::npos) ok = false; else q = t + 1; }
        if (!ok || key.empty()) continue;
        int64_t id = 0;
        try { id = std::stoll(l.substr(q)); } catch (std::exception&) { break; }   // a failed extraction ends the reference's loop
        map.emplace(key, id);
    }
}

inline int64_t find_taxon_id(const std::map<std::string, int64_t>& m, const std::string& name)   // building.cpp:240-262
{
    if (m.empty() || name.empty()) return 0;
    auto i = m.find(name);
    if (i != m.end()) return i->second;
    i = m.upper_bound(name);
    if (i == m.end()) return 0;
    if (i->first.compare(0, name.size(), name) != 0) return 0;
    return i->second;
}

struct BuilderError : std::runtime_error { using std::runtime_error::runtime_error; };   // device / capacity failures: fatal

// ---- the built database: builder handle (device arrays) + taxonomy records (non-target taxa, then one taxon per target) ----
struct BuiltDatabase {
    std::vector<mc_builder*> bs;                    // one builder, or one per key shard (all are given every target)
    BuildOptions opt;
    std::vector<Taxon> nonTarget;
    std::vector<Taxon> targets;                     // id = -(target) - 1, rank sequence
    ~BuiltDatabase() { for (mc_builder* b : bs) mc_build_free(b); }

    void write() const                              // write_database, building.cpp:546-566
    {
        const bool info = opt.info != BuildOptions::silent;
        if (info) std::cout << "------------------------------------------------\nWriting database to file ... " << std::endl;
        std::vector<mc_taxon_rec> recs(nonTarget.size());
        for (size_t i = 0; i < nonTarget.size(); ++i) recs[i] = mc_taxon_rec{nonTarget[i].id, nonTarget[i].parent, (uint32_t)nonTarget[i].rank, nonTarget[i].name.c_str()};
        if (mc_build_write_shards(const_cast<mc_builder**>(bs.data()), (uint32_t)bs.size(), opt.dbfile.c_str(), recs.data(), recs.size()) != MC_OK) {
            if (info) std::cout << "FAIL" << std::endl;
            std::cerr << "Could not write database file!\n";
            return;
        }
        if (info) std::cout << "Completed database writing." << std::endl;
    }
};

// ---- taxmap (mc_taxmap_*): the ranking pass hands its accession2taxid tables to the library ---------------------------
// MCQ_TAXMAP_DEVICE=1 (build, modify, build+query).  Shaped as the hand-offs of mcq_device_steps.h: the switch, run, report.  Every file
// the host loop would open is mapped, its first line dropped, and the rest goes to mc_taxmap_add(MC_TAXMAP_HOST) in pieces cut at line
// ends (MCQ_TAXMAP_PIECE bytes each, 256 MiB by default), until no name is wanted -- where the host loop breaks.  Nothing is applied
// before the last piece is through: any verdict other than MC_TAXMAP_OK and any library error leave the WHOLE pass to the host loop;
// `why` says which file, verdict and offence.
struct TaxmapStep {
    bool on = false;
    std::string why;                         // on and not ranked by the library: why
    uint64_t calls = 0, bytes = 0, rows = 0, files = 0, ranked = 0;
    double validateMs = 0, matchMs = 0;      // under MCQ_PROFILE: the kernels' time (mc_timing_get)
    std::vector<std::string> tried;          // the files the pass opened, in order (the host loop's "Try to map" lines)
    std::vector<int64_t> taxid; std::vector<uint64_t> position;   // per name in the map's order; position all ones: not found
    size_t piece = (size_t)256 << 20;
    TaxmapStep()
    {
        const char* sw = std::getenv("MCQ_TAXMAP_DEVICE"); on = sw && std::atoi(sw) != 0;
        if (const char* p = std::getenv("MCQ_TAXMAP_PIECE")) piece = std::min<size_t>(std::max<long long>(1, std::atoll(p)), (size_t)1 << 31);
    }

    bool run(const std::vector<std::string>& mapFiles, const std::map<std::string, uint32_t>& name2tgt, const std::set<uint32_t>& unranked)
    {
        mc_config cfg;
        mc_config_default(&cfg);
        mc_ctx* ctx = nullptr;
        if (mc_create(&cfg, &ctx) != MC_OK) { why = mc_last_error(nullptr); return false; }
        struct Closer { mc_ctx* c; ~Closer() { mc_taxmap_end(c); mc_destroy(c); } } closer{ctx};
        auto failed = [&](const std::string& what) { why = what; return false; };
        auto lib_failed = [&] { return failed(mc_last_error(ctx)); };
        const bool profile = std::getenv("MCQ_PROFILE") != nullptr;
        if (profile) mc_timing_enable(ctx, 1);
        std::string names;
        std::vector<uint64_t> off(1, 0);
        std::vector<uint8_t> wanted;
        for (const auto& kv : name2tgt) { names += kv.first; off.push_back(names.size()); wanted.push_back(unranked.count(kv.second) ? 1 : 0); }
        if (mc_taxmap_begin(ctx, names.data(), off.data(), wanted.size(), wanted.data()) != MC_OK) return lib_failed();
        uint64_t remaining = unranked.size();
        for (const std::string& file : mapFiles) {
            if (remaining == 0) break;
            const int fd = open(file.c_str(), O_RDONLY);
            if (fd < 0) continue;                                              // (the host loop's `!is.good()`)
            struct FdCloser { int fd; ~FdCloser() { close(fd); } } fdc{fd};
            struct stat sb;
            if (fstat(fd, &sb) != 0 || !S_ISREG(sb.st_mode)) return failed(file + ": not a regular file");
            tried.push_back(file);
            const size_t size = (size_t)sb.st_size;
            if (size == 0) { ++files; continue; }
            void* m = mmap(nullptr, size, PROT_READ, MAP_PRIVATE, fd, 0);
            if (m == MAP_FAILED) return failed(file + ": cannot be mapped");
            struct Unmapper { void* p; size_t n; ~Unmapper() { munmap(p, n); } } um{m, size};
            const char* data = (const char*)m;
            const void* nl0 = memchr(data, '\n', size);
            const size_t body = nl0 ? (size_t)((const char*)nl0 - data) + 1 : size;   // the first line is dropped unread
            for (size_t pos = body; pos < size && remaining != 0;) {
                size_t len = std::min(size - pos, piece);
                if (pos + len < size) {
                    const void* nl = memrchr(data + pos, '\n', len);
                    if (!nl) {                                                 // no line end in a piece: up to the next one, if that is a range
                        const void* nx = memchr(data + pos + len, '\n', size - pos - len);
                        len = nx ? (size_t)((const char*)nx - (data + pos)) + 1 : size - pos;
                        if (len > ((size_t)1 << 31)) return failed(file + ": a line of more than 2^31 bytes");
                    }
                    else len = (size_t)((const char*)nl - (data + pos)) + 1;
                }
                uint64_t st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
                if (mc_taxmap_add(ctx, data + pos, len, MC_TAXMAP_HOST, st, nullptr, 0, nullptr) != MC_OK) return lib_failed();
                if (st[5] != MC_TAXMAP_OK) return failed(file + ": verdict " + std::to_string(st[5]) + " (irregular line) at offset " + std::to_string(pos + st[6]));
                ++calls; bytes += len; rows += st[0]; ranked += st[3];
                remaining = st[4];
                pos += len;
            }
            ++files;
        }
        taxid.assign(wanted.size(), 0); position.assign(wanted.size(), ~0ull);
        if (mc_taxmap_result(ctx, taxid.data(), position.data(), nullptr, MC_TAXMAP_HOST, nullptr) != MC_OK) return lib_failed();
        if (profile) { uint64_t n = 0; mc_timing_get(ctx, "taxmap_validate", &validateMs, &n); mc_timing_get(ctx, "taxmap_match", &matchMs, &n); }
        return true;
    }
    // the device's line under MCQ_PROFILE; the fall-back's line also wherever the info level is not silent: the switch was set
    void report(bool done, bool info) const
    {
        const bool profile = std::getenv("MCQ_PROFILE") != nullptr;
        if (!on || (done ? !profile : !(profile || info))) return;
        if (done) std::cerr << "mcq profile: targets ranked on the device: " << calls << " mc_taxmap_add calls, " << bytes << " bytes, " << rows << " rows, " << ranked
                            << " targets ranked, kernels " << validateMs << " + " << matchMs << " ms, " << files << " files, 0 files left to the host\n";
        else std::cerr << "mcq: targets ranked on the host (" << why << ")\n";
    }
};

// ---- target parse (mc_parse_targets): the file loop hands plain FASTA files to the library ------------------------------
// MCQ_BUILD_PARSE_DEVICE=1 (build, modify, build+query).  Shaped as TaxmapStep: the switch, run, report.  The file loop of build_database
// walks the input files in order; consecutive files the step takes (regular, not empty, no gzip magic, first byte '>') are gathered into one
// PIECE of at most MCQ_BUILD_PARSE_PIECE bytes (256 MiB by default, within [4096, 2^31]): their bytes are copied from their mappings into
// one pinned staging buffer, uploaded once and cut by mc_parse_targets (device form, on a context of the builders' device); status, targets
// and hdr come back after ONE wait.  The headers are read from the staging buffer, which holds the bytes hdr points into -- no
// mc_parse_headers call, nothing more to download.  Every record with len > 0 then goes through the loop's own body with
// mc_build_add_target_device(seq + seq_off), every builder reading the same memory, and mc_build_flush precedes the buffers' reuse.
// A file larger than a piece is cut on the host at record starts (the last "\n>" inside the room; the piece doubles up to 2^31 where there
// is none) and ALL its ranges are judged (a call without room for a record: verdict and counts only) before its first target is added, so
// a file is added entirely here or entirely by the host loop.  MC_PARSE_IRREGULAR leaves the piece's files to the host loop, in order;
// MC_PARSE_OVERFLOW (more records than the tables hold) is answered by one second call with grown tables; a library error leaves the rest
// of the pass to the host loop.
// MCQ_BUILD_INFLATE_DEVICE=1 beside it: a file with the gzip magic is no longer refused outright.  mc_gzip_hint on its
// mapping decides; a file whose header the device takes and whose trailing ISIZE is at most MCQ_BUILD_INFLATE_MAX_MB (and a piece) joins
// the piece as COMPRESSED bytes, counted with its trailing ISIZE.  The piece's gzip files go up in a second pinned buffer and ONE
// mc_inflate_streams call (device form) writes each at its offset of dIn with out_cap = its trailing ISIZE; one wait brings the results
// back.  All rows accepted with produced == out_cap: mc_parse_targets runs on the piece as before, and the headers come from
// mc_parse_headers (the staging buffer does not hold those files' bytes).  The FIRST row that is not ends the piece: the files in front
// of it are parsed and added, it goes through the host loop named "gzip: <reason>", the files behind it are a piece of their own.
struct TargetParseStep {
    struct Mapped {
        int fd = -1; const char* p = nullptr; size_t n = 0;
        bool gz = false; size_t plain = 0;                                        // a gzip file the step inflates: its trailing ISIZE
        size_t size() const { return gz ? plain : n; }                            // the bytes it takes of a piece
        ~Mapped() { if (p) munmap((void*)p, n); if (fd >= 0) close(fd); }
    };
    // a file, or a range of a cut one: n plain bytes of the piece.  gz: data is the file's zn COMPRESSED bytes, n its trailing ISIZE
    struct Segment { size_t fi; const char* data; size_t n; uint64_t recordBase; bool first; bool gz; size_t zn; };
    struct Buf { void* p = nullptr; size_t cap = 0; int kind = 0; };

    bool on = false, dead = false;
    std::string deadWhy;                     // a library error: why the rest of the pass is the host loop's
    size_t piece = (size_t)256 << 20;
    uint64_t calls = 0, bytes = 0, records = 0, targets = 0, files = 0;
    std::vector<std::string> left;           // "file: reason" of every file that went to the host loop
    mc_ctx* ctx = nullptr;
    Buf hIn{nullptr, 0, 1}, hOff{nullptr, 0, 1}, hStatus{nullptr, 0, 1}, hHdr{nullptr, 0, 1}, hTargets{nullptr, 0, 1};
    Buf dIn, dOff, dStatus, dHdr, dTargets, dSeq, dWs;
    // MCQ_BUILD_INFLATE_DEVICE=1: gzip files join a piece as compressed bytes and mc_inflate_streams writes them into dIn
    bool inflateOn = false, inflateAlone = false;
    // MCQ_BUILD_INFLATE_MAX_MB: plain bytes per gzip file.  A row is one wave's serial work and the piece waits for its longest row; 4 is
    // where one row takes the device as long as gzread takes for a whole piece of 256 MiB on one host thread (measured: DESIGN.md 7n)
    size_t inflateMax = (size_t)4 << 20;
    uint64_t zCalls = 0, zFiles = 0, zBytesIn = 0, zBytesOut = 0;
    std::vector<std::string> zLeft;          // "file: gzip: reason" of every gzip file that went to the host loop
    Buf hZ{nullptr, 0, 1}, hRows{nullptr, 0, 1}, hResults{nullptr, 0, 1}, hText{nullptr, 0, 1}, hTextOff{nullptr, 0, 1};
    Buf dZ, dRows, dResults, dZStatus, dText, dTextOff, dTextStatus, dTextWs;
    uint32_t recCap = 1u << 16;
    std::vector<Segment> segs;               // the piece being gathered
    std::vector<std::unique_ptr<Mapped>> maps;
    size_t fill = 0;

    TargetParseStep()
    {
        const char* sw = std::getenv("MCQ_BUILD_PARSE_DEVICE"); on = sw && std::atoi(sw) != 0;
        if (const char* p = std::getenv("MCQ_BUILD_PARSE_PIECE")) piece = (size_t)std::min<long long>(std::max<long long>(4096, std::atoll(p)), 1ll << 31);
        const char* zw = std::getenv("MCQ_BUILD_INFLATE_DEVICE");
        const bool zset = zw && std::atoi(zw) != 0;
        inflateOn = zset && on; inflateAlone = zset && !on;
        if (const char* p = std::getenv("MCQ_BUILD_INFLATE_MAX_MB")) inflateMax = (size_t)std::min<long long>(std::max<long long>(1, std::atoll(p)), 2048) << 20;
    }
    ~TargetParseStep()
    {
        if (!ctx) return;
        for (Buf* b : {&hIn, &hOff, &hStatus, &hHdr, &hTargets, &dIn, &dOff, &dStatus, &dHdr, &dTargets, &dSeq, &dWs}) mc_buffer_free(ctx, b->p, b->kind);
        for (Buf* b : {&hZ, &hRows, &hResults, &hText, &hTextOff, &dZ, &dRows, &dResults, &dZStatus, &dText, &dTextOff, &dTextStatus, &dTextWs}) mc_buffer_free(ctx, b->p, b->kind);
        mc_destroy(ctx);
    }
    TargetParseStep(const TargetParseStep&) = delete;

    bool begin(int device)
    {
        mc_config cfg;
        mc_config_default(&cfg);
        cfg.device = device;
        if (mc_create(&cfg, &ctx) != MC_OK) { ctx = nullptr; return die(mc_last_error(nullptr)); }
        if (std::getenv("MCQ_PROFILE")) mc_timing_enable(ctx, 1);
        return room(hStatus, 64) && room(dStatus, 64);
    }
    bool die(const std::string& why) { dead = true; deadWhy = why; return false; }
    bool room(Buf& b, size_t need)
    {
        if (need <= b.cap) return true;
        mc_buffer_free(ctx, b.p, b.kind); b.p = nullptr; b.cap = 0;
        if (mc_buffer_alloc(ctx, need, b.kind, &b.p) != MC_OK) return die(mc_last_error(ctx));
        b.cap = need;
        return true;
    }
    bool copy(void* dst, const void* src, size_t n, int kind) { return mc_copy_results_on(ctx, dst, src, n, kind, nullptr) == MC_OK || die(mc_last_error(ctx)); }
    bool wait() { return mc_synchronize(ctx) == MC_OK || die(mc_last_error(ctx)); }

    static const char* reason_word(uint32_t r)
    {
        static const char* const words[] = {"accepted", "block type", "stored lengths", "code lengths", "symbol", "distance", "input ends early", "more bytes than its trailing size",
                                            "fewer bytes than its trailing size", "bytes left", "crc", "header", "trailing bytes"};
        return r < sizeof words / sizeof words[0] ? words[r] : "unknown reason";
    }

    // does the step take this file?  why: the reason where it does not
    std::unique_ptr<Mapped> take(const std::string& file, std::string& why) const
    {
        std::unique_ptr<Mapped> m(new Mapped);
        m->fd = open(file.c_str(), O_RDONLY);
        struct stat sb;
        if (m->fd < 0 || fstat(m->fd, &sb) != 0) { why = "unreadable"; return nullptr; }
        if (!S_ISREG(sb.st_mode)) { why = "not a regular file"; return nullptr; }
        if (sb.st_size == 0) { why = "empty"; return nullptr; }
        unsigned char magic[2] = {0, 0};
        if (pread(m->fd, magic, 2, 0) < 1) { why = "unreadable"; return nullptr; }
        if (sb.st_size >= 2 && magic[0] == 0x1f && magic[1] == 0x8b) {
            if (!inflateOn) { why = "gzip"; return nullptr; }
            // the hint on the file's mapping decides: a header the device takes, and a trailing ISIZE within the cap and a piece
            void* z = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, m->fd, 0);
            if (z == MAP_FAILED) { why = "cannot be mapped"; return nullptr; }
            m->p = (const char*)z; m->n = (size_t)sb.st_size;
            uint64_t hint[4] = {0, 0, 0, 0};
            if (mc_gzip_hint((const uint8_t*)m->p, m->n, hint) != MC_OK) { why = "gzip: no hint"; return nullptr; }
            if (hint[0] != MC_GZIP_OK) { why = std::string("gzip: ") + reason_word((uint32_t)hint[3]); return nullptr; }
            if (m->n > ((size_t)1 << 28)) { why = "gzip: more than 2^28 compressed bytes"; return nullptr; }
            if (hint[2] == 0) { why = "gzip: a trailing size of 0"; return nullptr; }
            if (hint[2] > inflateMax) { why = "gzip: larger than MCQ_BUILD_INFLATE_MAX_MB"; return nullptr; }
            if (hint[2] > piece) { why = "gzip: larger than a piece"; return nullptr; }
            m->gz = true; m->plain = (size_t)hint[2];
            return m;
        }
        if (magic[0] == '@') { why = "FASTQ"; return nullptr; }
        if (magic[0] != '>') { why = "does not begin with '>'"; return nullptr; }
        void* p = mmap(nullptr, (size_t)sb.st_size, PROT_READ, MAP_PRIVATE, m->fd, 0);
        if (p == MAP_FAILED) { why = "cannot be mapped"; return nullptr; }
        m->p = (const char*)p; m->n = (size_t)sb.st_size;
        return m;
    }

    // a file cut at record starts into ranges of at most `cap` bytes, cap doubling up to 2^31 where a record does not fit: [begin, end) each
    static bool cut_file(const char* data, size_t size, size_t cap, std::vector<std::pair<size_t, size_t>>& out)
    {
        for (size_t pos = 0; pos < size;) {
            size_t len = std::min(size - pos, cap);
            if (pos + len < size) {
                const char* base = data + pos + 1;                             // (a cut at pos itself would be no cut)
                const char* q = (const char*)memrchr(base, '>', len - 1);
                while (q && q[-1] != '\n') q = (const char*)memrchr(base, '>', (size_t)(q - base));
                if (!q) {
                    if (cap >= ((size_t)1 << 31)) return false;
                    cap = std::min(cap * 2, (size_t)1 << 31);
                    continue;
                }
                len = (size_t)(q - (data + pos));
            }
            out.emplace_back(pos, pos + len);
            pos += len;
        }
        return true;
    }

    void gather(size_t fi, std::unique_ptr<Mapped> m) { segs.push_back(Segment{fi, m->p, m->size(), 0, true, m->gz, m->n}); fill += m->size(); maps.push_back(std::move(m)); }
    void clear() { segs.clear(); maps.clear(); fill = 0; }

    // what a range of n bytes in nf files needs of seq: a sequence's padding exceeds what its record's '>' and line ends give back only
    // for a file's LAST record, whose final '\n' may be missing -- by one byte per file
    static size_t seq_bound(size_t n, uint32_t nf) { return n + nf + 16; }
    // every buffer of a call for n bytes in nf files with tables of maxRecords rows.  false: the step died
    bool rooms(size_t n, uint32_t nf, uint32_t maxRecords)
    {
        const size_t rows = std::max<size_t>(maxRecords, 2);
        return room(hIn, n) && room(hOff, ((size_t)nf + 1) * 8) && room(dIn, (n + 15) / 16 * 16 + 16) && room(dOff, ((size_t)nf + 1) * 8) &&
               room(dWs, mc_parse_targets_scratch_bytes(n, nf, maxRecords)) && room(dSeq, seq_bound(n, nf) + 16) && room(dHdr, rows * 8) && room(dTargets, rows * sizeof(mc_parse_target)) &&
               room(hHdr, rows * 8) && room(hTargets, rows * sizeof(mc_parse_target));
    }

    // the segments' bytes into the staging buffer and up; mc_parse_targets with tables of maxRecords rows; status, and with them hdr and
    // targets at the tables' size, back after ONE wait.  false: the step died
    bool parse(const std::vector<Segment>& ss, uint32_t maxRecords, uint64_t st[8])
    {
        size_t n = 0;
        for (const Segment& s : ss) n += s.n;
        const uint32_t nf = (uint32_t)ss.size();
        const uint64_t wsBytes = mc_parse_targets_scratch_bytes(n, nf, maxRecords);
        if (!rooms(n, nf, maxRecords)) return false;
        uint64_t* off = (uint64_t*)hOff.p;
        size_t at = 0;
        bool anyGz = false;
        for (uint32_t f = 0; f < nf; ++f) { off[f] = at; if (ss[f].gz) anyGz = true; else std::memcpy((char*)hIn.p + at, ss[f].data, ss[f].n); at += ss[f].n; }
        off[nf] = at;
        if (!anyGz) { if (!copy(dIn.p, hIn.p, n, 2)) return false; }
        else                                                                    // (the gzip files' ranges of dIn hold what inflate() wrote: only the runs of plain files go up)
            for (uint32_t f = 0; f < nf;) {
                uint32_t e = f;
                while (e < nf && ss[e].gz == ss[f].gz) ++e;
                if (!ss[f].gz && !copy((char*)dIn.p + off[f], (char*)hIn.p + off[f], off[e] - off[f], 2)) return false;
                f = e;
            }
        if (!copy(dOff.p, hOff.p, ((size_t)nf + 1) * 8, 2)) return false;
        mc_parse_targets_output o{};
        o.hdr = (uint32_t*)dHdr.p; o.targets = (mc_parse_target*)dTargets.p; o.seq = (uint8_t*)dSeq.p; o.seq_capacity = maxRecords ? seq_bound(n, nf) : 0;
        o.status = (uint64_t*)dStatus.p; o.max_records = maxRecords;
        if (mc_parse_targets(ctx, (const char*)dIn.p, n, (const uint64_t*)dOff.p, nf, 0, &o, dWs.p, wsBytes, nullptr) != MC_OK) return die(mc_last_error(ctx));
        ++calls;
        if (!copy(hStatus.p, dStatus.p, 64, 1)) return false;
        if (maxRecords && (!copy(hHdr.p, dHdr.p, (size_t)maxRecords * 8, 1) || !copy(hTargets.p, dTargets.p, (size_t)maxRecords * sizeof(mc_parse_target), 1))) return false;
        if (!wait()) return false;
        std::memcpy(st, hStatus.p, 64);
        return true;
    }

    // the piece's gzip files, uploaded as they are and inflated into dIn at their offsets by ONE mc_inflate_streams call (device form,
    // out_cap = the trailing ISIZE); ONE wait brings the results back.  -1: every row was accepted with produced == out_cap (or there is
    // no gzip file); >= 0: the first segment that was not, `word` says why; -2: the step died.  The bytes of the segments in front of
    // a refused one are in dIn, contiguous from 0
    int inflate(const std::vector<Segment>& ss, std::string& word)
    {
        size_t n = 0, zbytes = 0;
        uint32_t nz = 0;
        for (const Segment& s : ss) { if (s.gz) { zbytes = (zbytes + 15) / 16 * 16 + s.zn; ++nz; } n += s.n; }
        if (!nz) return -1;
        if (!(room(hZ, zbytes) && room(dZ, (zbytes + 15) / 16 * 16 + 16) && room(hRows, nz * sizeof(mc_gzip_stream)) && room(dRows, nz * sizeof(mc_gzip_stream)) &&
              room(hResults, nz * sizeof(mc_gzip_result)) && room(dResults, nz * sizeof(mc_gzip_result)) && room(dZStatus, 32) && room(dIn, (n + 15) / 16 * 16 + 16))) return -2;
        mc_gzip_stream* rows = (mc_gzip_stream*)hRows.p;
        size_t at = 0, z = 0;
        uint32_t k = 0;
        for (const Segment& s : ss) {
            if (s.gz) {
                z = (z + 15) / 16 * 16;
                std::memcpy((char*)hZ.p + z, s.data, s.zn);
                rows[k++] = mc_gzip_stream{z, s.zn, at, s.n};
                z += s.zn;
            }
            at += s.n;
        }
        if (!copy(dZ.p, hZ.p, zbytes, 2) || !copy(dRows.p, hRows.p, nz * sizeof(mc_gzip_stream), 2)) return -2;
        if (mc_inflate_streams(ctx, (const uint8_t*)dZ.p, zbytes, (const mc_gzip_stream*)dRows.p, nz, 0, (uint8_t*)dIn.p, n, (mc_gzip_result*)dResults.p, (uint64_t*)dZStatus.p,
                               nullptr) != MC_OK) { die(mc_last_error(ctx)); return -2; }
        ++zCalls;
        if (!copy(hResults.p, dResults.p, nz * sizeof(mc_gzip_result), 1) || !wait()) return -2;
        const mc_gzip_result* res = (const mc_gzip_result*)hResults.p;
        k = 0;
        for (size_t f = 0; f < ss.size(); ++f) {
            if (!ss[f].gz) continue;
            const mc_gzip_result& r = res[k++];
            if (r.reason) { word = reason_word(r.reason); return (int)f; }
            if (r.produced != ss[f].n) { word = "fewer bytes than its trailing size"; return (int)f; }
            ++zFiles; zBytesIn += ss[f].zn; zBytesOut += r.produced;
        }
        return -1;
    }

    // the headers of a parsed piece that holds gzip files, packed by mc_parse_headers from dIn (the staging buffer does not hold those
    // files' bytes) and downloaded: hText, hTextOff.  false: why says so
    bool headers(size_t n, uint64_t recs, std::string& why)
    {
        const uint32_t* hdr = (const uint32_t*)hHdr.p;
        size_t total = 0;
        for (uint64_t r = 0; r < recs; ++r) total += hdr[2 * r + 1];
        const uint64_t wsBytes = mc_parse_headers_scratch_bytes((uint32_t)recs);
        if (!(room(dText, total + 16) && room(hText, total + 16) && room(dTextOff, (recs + 1) * 8) && room(hTextOff, (recs + 1) * 8) && room(dTextStatus, 32) &&
              room(dTextWs, wsBytes + 16))) { why = deadWhy; return false; }
        if (mc_parse_headers(ctx, (const char*)dIn.p, n, (const uint32_t*)dHdr.p, (const uint64_t*)dStatus.p, (uint32_t)recs, 0, (char*)dText.p, total, (uint64_t*)dTextOff.p,
                             (uint64_t*)dTextStatus.p, dTextWs.p, wsBytes, nullptr) != MC_OK) { die(mc_last_error(ctx)); why = deadWhy; return false; }
        if ((total && !copy(hText.p, dText.p, total, 1)) || !copy(hTextOff.p, dTextOff.p, (recs + 1) * 8, 1) || !copy(hStatus.p, dTextStatus.p, 32, 1) || !wait()) { why = deadWhy; return false; }
        const uint64_t* st = (const uint64_t*)hStatus.p;
        if (st[2] != MC_PARSE_OK || st[0] != recs || st[1] != total) { why = "headers: verdict " + std::to_string(st[2]); return false; }
        return true;
    }

    // one piece: parsed (a second call where the tables were too small), then every record with len > 0 added through add_record(segment,
    // record number in its file, header, length, device address).  false: nothing was added; why says so (the step may have died)
    template <class Prologue, class AddRecord>
    bool run(const std::vector<Segment>& ss, std::string& why, const std::vector<mc_builder*>& bs, Prologue&& prologue, AddRecord&& add_record)
    {
        uint64_t st[8];
        if (!parse(ss, recCap, st)) { why = deadWhy; return false; }
        if (st[4] == MC_PARSE_OVERFLOW && st[0] > recCap) {
            recCap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(st[0], 2ull * recCap), 0xFFFFFFFFull);
            if (!parse(ss, recCap, st)) { why = deadWhy; return false; }
        }
        if (st[4] == MC_PARSE_IRREGULAR) {
            why = "irregular at byte " + std::to_string(st[5] - ((const uint64_t*)hOff.p)[std::min<uint64_t>(st[7], ss.size() - 1)]) + " of file " + std::to_string(st[7]) + " of its piece";
            return false;
        }
        if (st[4] != MC_PARSE_OK) { why = "verdict " + std::to_string(st[4]); return false; }
        const uint64_t recs = st[0];                                            // (<= recCap: rows [0, recs) of hdr and targets came back with status)
        bool anyGz = false;
        size_t pieceBytes = 0;
        for (const Segment& s : ss) { anyGz = anyGz || s.gz; pieceBytes += s.n; }
        if (anyGz && recs && !headers(pieceBytes, recs, why)) return false;
        const uint64_t* textOff = (const uint64_t*)hTextOff.p;
        const uint32_t* hdr = (const uint32_t*)hHdr.p;
        const mc_parse_target* tg = (const mc_parse_target*)hTargets.p;
        uint64_t r = 0;
        for (uint32_t f = 0; f < ss.size(); ++f) {
            const int64_t fileTax = prologue(ss[f]);
            for (; r < recs && tg[r].file == f; ++r) {
                if (tg[r].len == 0) continue;                                   // building.cpp:295
                add_record(ss[f], fileTax, ss[f].recordBase + tg[r].index,
                           anyGz ? std::string((const char*)hText.p + textOff[r], textOff[r + 1] - textOff[r]) : std::string((const char*)hIn.p + hdr[2 * r], hdr[2 * r + 1]), (size_t)tg[r].len,
                           (const char*)dSeq.p + tg[r].seq_off);
                ++targets;
            }
        }
        for (mc_builder* b : bs) if (mc_build_flush(b) != MC_OK) throw std::runtime_error(mc_build_last_error(b));
        size_t n = 0;
        for (const Segment& s : ss) n += s.n;
        bytes += n; records += recs;
        return true;
    }

    // a file larger than a piece: cut, every range judged, the tables and buffers made for the largest range, then every range added.
    // Nothing that can be refused is left for the adding phase: verdicts, record counts and memory are settled before the first target
    // goes in.  What remains is a failing HIP call between two ranges, and that ends the build: the file's first targets cannot be taken back.
    template <class Prologue, class AddRecord>
    bool run_cut_file(size_t fi, const Mapped& m, std::string& why, const std::vector<mc_builder*>& bs, Prologue&& prologue, AddRecord&& add_record)
    {
        std::vector<std::pair<size_t, size_t>> cuts;
        if (!cut_file(m.p, m.n, piece, cuts)) { why = "a record that does not fit the largest piece"; return false; }
        std::vector<Segment> ranges;
        uint64_t base = 0, mostRecords = 0;
        size_t largest = 0;
        for (const auto& c : cuts) {
            std::vector<Segment> one(1, Segment{fi, m.p + c.first, c.second - c.first, base, c.first == 0});
            uint64_t st[8];
            if (!parse(one, 0, st)) { why = deadWhy; return false; }
            if (st[4] == MC_PARSE_IRREGULAR) { why = "irregular at byte " + std::to_string(c.first + st[5]); return false; }
            ranges.push_back(one[0]);
            base += st[0]; mostRecords = std::max(mostRecords, st[0]); largest = std::max(largest, one[0].n);
        }
        recCap = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(mostRecords, recCap), 0xFFFFFFFFull);
        if (!rooms(largest, 1, recCap)) { why = deadWhy; return false; }
        for (const Segment& s : ranges) {
            std::vector<Segment> one(1, s);
            if (!run(one, why, bs, prologue, add_record)) throw std::runtime_error("mcq build: the device parse failed inside a file whose first targets were added (" + why + ")");
        }
        return true;
    }

    // the device's line under MCQ_PROFILE; the fall-back's line also wherever the info level is not silent: the switch was set
    void report(bool info)
    {
        const bool profile = std::getenv("MCQ_PROFILE") != nullptr;
        if (!on) return;
        std::string list;
        for (const auto& l : left) list += (list.empty() ? " (" : "; ") + l;
        if (!list.empty()) list += ")";
        if (profile) {
            double classifyMs = 0, writeMs = 0; uint64_t n = 0;
            if (ctx) { mc_timing_get(ctx, "targets_classify", &classifyMs, &n); mc_timing_get(ctx, "targets_write", &writeMs, &n); }
            std::cerr << "mcq profile: reference sequences parsed on the device: " << calls << " mc_parse_targets calls, " << bytes << " bytes, " << records << " records, "
                      << targets << " targets, kernels " << classifyMs << " + " << writeMs << " ms, " << files << " files, " << left.size() << " files left to the host" << list << "\n";
        }
        if (profile && inflateOn) {
            double ms = 0; uint64_t n = 0;
            if (ctx) mc_timing_get(ctx, "inflate_streams", &ms, &n);
            std::string zlist;
            for (const auto& l : zLeft) zlist += (zlist.empty() ? " (" : "; ") + l;
            if (!zlist.empty()) zlist += ")";
            std::cerr << "mcq profile: gzip references inflated on the device: " << zFiles << " files, " << zBytesIn << " bytes in, " << zBytesOut << " bytes out, " << zCalls
                      << " mc_inflate_streams calls, kernels " << ms << " ms, " << zLeft.size() << " gzip files left to the host" << zlist << "\n";
        }
        if (!left.empty() && (profile || info))
            std::cerr << "mcq: reference sequences of " << left.size() << " files parsed on the host" << list << (dead ? " [the device parse stopped: " + deadWhy + "]" : "") << "\n";
    }
};

inline void build_database(const BuildOptions& o, BuiltDatabase& db)
{
    using clock = std::chrono::steady_clock;
    const auto t0 = clock::now();
    const bool info = o.info != BuildOptions::silent;
    db.opt = o;
    // prepare_database (building.cpp:462-508)
    if (info) std::cout << "Max locations per feature set to " << o.maxLocs << std::endl;
    if (o.maxLoadFac > 0.4f && o.maxLoadFac < 0.99f && info) std::cout << "Using custom hash table load factor of " << o.maxLoadFac << std::endl;
    if (!o.taxPath.empty()) {
        TaxTree t = read_taxonomy_dumps(o);
        db.nonTarget = std::move(t.taxa);
        if (info) std::cout << "Taxonomy applied to database." << std::endl;
    }
    if (db.nonTarget.empty() && info)
        std::cout << "The datbase doesn't contain a taxonomic hierarchy yet.\nYou can add one or update later via:\n"
                     "   metacache modify <database> -taxonomy <directory>" << std::endl;
    if (o.removeAmbigRank != kNumRanks && info) {                                // building.cpp:508-518
        if (db.nonTarget.size() > 1) std::cout << "Ambiguous features on rank " << kRankNames[o.removeAmbigRank] << " will be removed afterwards." << std::endl;
        else std::cout << "Could not determine amiguous features due to missing taxonomic information." << std::endl;
    }

    mc_config c; mc_config_default(&c);
    c.kmerlen = o.k; c.sketchlen = o.s; c.winlen = o.w; c.winstride = o.stride;
    c.target_id_bytes = (uint32_t)o.targetIdBytes;
    c.max_locations_per_feature = (uint32_t)std::max(1, std::min(o.maxLocs, 254));
    c.remove_overpopulated = o.removeOverpopulated ? 1 : 0;
    if (o.maxLoadFac > 0.4f && o.maxLoadFac < 0.99f) c.max_load_factor = o.maxLoadFac;
    // one device sort takes 2^32 (feature, location) pairs: larger inputs are built in key shards (every shard sketches every target
    // and keeps its share of the features; mc_build_finish_shards / mc_build_write_shards put them together)
    uint32_t shards = o.shards > 0 ? (uint32_t)o.shards : 1u;
    if (o.shards <= 0) {
        uint64_t bytes = 0;
        for (const auto& f : o.infiles) { struct stat st; if (stat(f.c_str(), &st) == 0) bytes += (uint64_t)st.st_size * (f.size() > 3 && f.compare(f.size() - 3, 3, ".gz") == 0 ? 4 : 1); }
        uint64_t pairs = bytes / std::max<uint32_t>(o.stride, 1) * o.s;
        if (o.modify) {                                                        // + the locations the database already holds
            std::ifstream is(o.dbfile + ".cache0", std::ios::binary);
            uint64_t hdr[3] = {0, 0, 0};
            if (is.read(reinterpret_cast<char*>(hdr), 24)) pairs += hdr[1];
        }
        shards = (uint32_t)(pairs / 3000000000ull) + 1;
    }
    for (uint32_t i = 0; i < shards; ++i) {
        mc_builder* b = nullptr;
        c.key_shard_index = i; c.key_shard_count = shards;
        if (mc_build_begin(&c, &b) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
        db.bs.push_back(b);
    }
    if (info && shards > 1) std::cout << "Building in " << shards << " key shards." << std::endl;

    // make_sequence_to_taxon_id_map (taxonomy_io.cpp:290-318)
    std::map<std::string, int64_t> seq2tax;
    {
        std::set<std::string> dirs;                                            // unique_directories, filesys_utility.cpp:82-92
        for (const auto& f : o.infiles) dirs.insert(f.substr(0, f.find_last_of("/\\")));
        for (const auto& d : dirs) read_id_table(d + "/assembly_summary.txt", seq2tax, info);
        for (const char* f : {"assembly_summary_refseq.txt", "assembly_summary_refseq_historical.txt", "assembly_summary_genbank.txt",
                              "assembly_summary_genbank_historical.txt"})
            read_id_table(o.taxPath + f, seq2tax, info);
    }
    if (info) {
        const char* idn[] = {"smart", "ncbi", "gi", "filename", "leadingword"};
        std::cout << "Sequence ID extraction method: " << idn[(int)o.idType] << "\nProcessing reference sequences." << std::endl;
    }
    // add_targets_to_database (building.cpp:335-455) with one consumer: files in the given order, records in file order
    std::map<std::string, uint32_t> name2tgt;                                  // taxonomy_cache::name2tax_ (taxonomy.hpp:1135-1160)
    if (o.modify) {
        // make_database(opt.dbfile) (mode_build.cpp:80): targets with their sources, the taxa above them unless -taxonomy replaces them
        // (reset_taxa_above_sequence_level, building.cpp:487-495), and the location lists of the (single) part
        mc_ctx* meta = nullptr;
        if (mc_open_metadata(o.dbfile.c_str(), &meta) != MC_OK) throw std::runtime_error(mc_last_error(nullptr));
        struct Guard { mc_ctx* c; ~Guard() { mc_destroy(c); } } guard{meta};
        uint64_t dbi[8]; mc_db_info(meta, dbi);
        if (dbi[6] != 1) throw std::runtime_error("modify: databases of more than one part are not supported");
        uint64_t nt = 0; mc_db_num_taxa(meta, &nt);
        std::vector<Taxon> old(dbi[5]); std::vector<std::string> oldFile(dbi[5]); std::vector<uint64_t> oldIndex(dbi[5]);
        const bool keepTaxa = o.taxPath.empty();
        for (uint64_t i = 0; i < nt; ++i) {
            Taxon t; uint32_t rk; const char *nm, *fn; uint64_t idx = 0;
            mc_db_taxon(meta, i, &t.id, &t.parent, &rk, &nm);
            t.rank = int(rk); t.name = nm;
            mc_db_taxon_source(meta, i, &fn, &idx, &t.windows);
            if (t.id < 0 && t.rank == 0) {
                const uint64_t tgt = (uint64_t)(-t.id - 1);
                if (tgt >= old.size()) throw std::runtime_error("modify: target id beyond the database's target count");
                oldFile[tgt] = fn; oldIndex[tgt] = idx; old[tgt] = std::move(t);
            }
            else if (keepTaxa) db.nonTarget.push_back(std::move(t));
        }
        for (uint64_t t = 0; t < old.size(); ++t) {
            for (mc_builder* b : db.bs)
                if (mc_build_add_existing_target(b, old[t].name.c_str(), old[t].parent, oldFile[t].c_str(), oldIndex[t], old[t].windows) != MC_OK)
                    throw BuilderError(mc_build_last_error(b));
            name2tgt.emplace(old[t].name, (uint32_t)t);
            db.targets.push_back(std::move(old[t]));
        }
        std::ifstream is(o.dbfile + ".cache0", std::ios::binary);
        uint64_t hdr[3] = {0, 0, 0};
        if (!is.read(reinterpret_cast<char*>(hdr), 24)) throw std::runtime_error("Could not read database file '" + o.dbfile + ".cache0'");
        const size_t vb = 4 + (size_t)o.targetIdBytes;
        std::vector<uint32_t> keys; std::vector<uint8_t> sizes; std::vector<char> vals;
        for (uint64_t done = 0; done < hdr[0];) {
            const uint64_t nb = std::min<uint64_t>(hdr[2], hdr[0] - done);
            keys.resize(nb); sizes.resize(nb);
            is.read(reinterpret_cast<char*>(keys.data()), nb * 4);
            is.read(reinterpret_cast<char*>(sizes.data()), nb);
            uint64_t bv = 0;
            for (uint64_t i = 0; i < nb; ++i) bv += sizes[i];
            vals.resize(bv * vb + 8);
            is.read(vals.data(), bv * vb);
            if (!is) throw std::runtime_error("truncated " + o.dbfile + ".cache0");
            for (mc_builder* b : db.bs)
                if (mc_build_add_locations(b, keys.data(), sizes.data(), vals.data(), nb, (uint32_t)o.targetIdBytes) != MC_OK)
                    throw BuilderError(mc_build_last_error(b));
            done += nb;
        }
        if (info) std::cout << "Database holds " << db.targets.size() << " reference sequences." << std::endl;
    }
    const size_t initTargets = db.targets.size();
    // what both callers -- the host loop below and the device parse (TargetParseStep) -- do for a file and for a record of it
    auto file_taxid = [&](size_t fi, bool say) -> int64_t {
        const std::string& filename = o.infiles[fi];
        std::string fileAcc = accession_string(filename, o.idType);
        int64_t fileTax = find_taxon_id(seq2tax, fileAcc);
        if (fileTax == 0 && o.idType == IdType::smart) { fileAcc = accession_string(filename, IdType::filename); fileTax = find_taxon_id(seq2tax, fileAcc); }
        if (say && o.info == BuildOptions::verbose) std::cerr << "      accession '" << fileAcc << "' -> taxid " << fileTax << std::endl;
        return fileTax;
    };
    // add(builder, name, parent): the mc_build_add_target_* call that hands the sequence over
    auto add_record = [&](const std::string& filename, int64_t fileTax, uint64_t r, const std::string& header, size_t seqLen, const std::function<int(mc_builder*, const char*, int64_t)>& add) {
        std::string seqId = accession_string(header, o.idType);
        if (seqId.empty()) seqId = header;
        int64_t parent = fileTax;
        if (parent == 0) parent = find_taxon_id(seq2tax, seqId);
        if (parent == 0) parent = taxon_id_in_header(header);
        if (parent < 1) parent = 0;                                    // database.cpp:58
        // a name that is already taken gets "!1", "!1!2", ... appended until it is new (taxonomy.hpp:1141-1146)
        std::string sid = seqId;
        int dupl = 0;
        while (name2tgt.find(sid) != name2tgt.end()) { ++dupl; sid += "!" + std::to_string(dupl); }
        const uint32_t tgt = (uint32_t)db.targets.size();
        for (mc_builder* b : db.bs)
            if (add(b, sid.c_str(), parent) != MC_OK)
                throw BuilderError(mc_build_last_error(b));
        if (dupl > 0 && info)
            std::cerr << "Warning: duplicate sequence id! '" << seqId << "' already in database - '" << filename << "/" << r
                      << "' inserted as '" << sid << "'\n";
        name2tgt.emplace(sid, tgt);
        Taxon t; t.id = -(int64_t)tgt - 1; t.parent = parent; t.rank = 0; t.name = sid; t.srcFile = filename; t.srcIndex = r;
        mc_build_target_windows(db.bs[0], tgt, &t.windows);
        db.targets.push_back(std::move(t));
        if (o.info == BuildOptions::verbose) {
            std::cerr << "    P0  [" << seqId;
            if (parent > 0) std::cerr << ":" << parent;
            std::cerr << "]  " << seqLen << " bp" << (dupl > 0 ? "  --  not added to database!\n" : "\n");
        }
    };
    auto announce = [&](size_t fi) { if (o.info == BuildOptions::verbose) std::cerr << "  (" << fi << '/' << o.infiles.size() << ") " << o.infiles[fi] << std::endl; };
    auto host_file = [&](size_t fi) {
        const std::string& filename = o.infiles[fi];
        announce(fi);
        try {
            const int64_t fileTax = file_taxid(fi, true);
            SeqFile file(filename);
            file.index(std::max(1u, std::thread::hardware_concurrency()));
            std::string scratch;
            for (size_t r = 0; r < file.records(); ++r) {
                View h, s;
                file.record(r, h, s, scratch);
                if (s.empty()) continue;                                       // building.cpp:295
                add_record(filename, fileTax, r, std::string(h.p, h.n), s.n,
                           [&](mc_builder* b, const char* sid, int64_t parent) { return mc_build_add_target_src(b, s.p, s.n, sid, parent, filename.c_str(), r); });
            }
        } catch (BuilderError&) {
            throw;
        } catch (std::exception& e) {                                          // unreadable file: the reference reports it only with -verbose
            if (o.info == BuildOptions::verbose) std::cerr << "FAIL: " << e.what() << '\n';
        }
    };
    TargetParseStep parse;                                                     // MCQ_BUILD_PARSE_DEVICE=1: plain FASTA files are cut by the library, piece by piece
    if (parse.on) parse.begin(c.device);
    if (parse.inflateAlone && info) std::cerr << "mcq: MCQ_BUILD_INFLATE_DEVICE=1 has no effect without MCQ_BUILD_PARSE_DEVICE=1\n";
    auto device_prologue = [&](const TargetParseStep::Segment& s) -> int64_t { if (s.first) announce(s.fi); return file_taxid(s.fi, s.first); };   // (a later range of a cut file: its lines are out)
    auto device_record = [&](const TargetParseStep::Segment& s, int64_t fileTax, uint64_t r, const std::string& header, size_t len, const char* dseq) {
        const std::string& filename = o.infiles[s.fi];
        add_record(filename, fileTax, r, header, len,
                   [&](mc_builder* b, const char* sid, int64_t parent) { return mc_build_add_target_device(b, dseq, len, sid, parent, filename.c_str(), r); });
    };
    // the gathered piece goes through the library; where it refuses, the piece's files go through the host loop, in order
    // Its gzip files are inflated first; the first one the device refuses ends the piece: the files in front of it are parsed and added (their
    // bytes lie in the piece from 0), that file goes through the host loop, the files behind it are a piece of their own.  Order stays
    auto drain = [&]() {
        if (parse.segs.empty()) return;
        std::vector<TargetParseStep::Segment> ss = parse.segs;
        while (!ss.empty()) {
            std::string why, word;
            const int bad = parse.dead ? -2 : parse.inflate(ss, word);
            if (bad == -2) {
                for (const auto& s : ss) { parse.left.push_back(o.infiles[s.fi] + ": " + parse.deadWhy); host_file(s.fi); }
                break;
            }
            const std::vector<TargetParseStep::Segment> head(ss.begin(), bad < 0 ? ss.end() : ss.begin() + bad);
            if (!head.empty()) {
                if (parse.run(head, why, db.bs, device_prologue, device_record)) parse.files += head.size();
                else for (const auto& s : head) { parse.left.push_back(o.infiles[s.fi] + ": " + why); host_file(s.fi); }
            }
            if (bad < 0) break;
            parse.left.push_back(o.infiles[ss[bad].fi] + ": gzip: " + word);
            parse.zLeft.push_back(parse.left.back());
            host_file(ss[bad].fi);
            ss.erase(ss.begin(), ss.begin() + bad + 1);
        }
        parse.clear();
    };
    for (size_t fi = 0; fi < o.infiles.size(); ++fi) {
        if (!parse.on) { host_file(fi); continue; }
        std::string why = parse.deadWhy;
        std::unique_ptr<TargetParseStep::Mapped> m = parse.dead ? nullptr : parse.take(o.infiles[fi], why);
        if (m && m->size() > parse.piece) {                                    // a file of several pieces: on its own (never a gzip file: take leaves those to the host)
            drain();
            if (!parse.dead && parse.run_cut_file(fi, *m, why, db.bs, device_prologue, device_record)) { ++parse.files; continue; }
            if (parse.dead) why = parse.deadWhy;
            m.reset();
        }
        if (!m) { drain(); parse.left.push_back(o.infiles[fi] + ": " + why); if (why.compare(0, 5, "gzip:") == 0) parse.zLeft.push_back(parse.left.back()); host_file(fi); continue; }
        if (parse.fill + m->size() > parse.piece) drain();
        if (parse.dead) { parse.left.push_back(o.infiles[fi] + ": " + parse.deadWhy); host_file(fi); continue; }
        parse.gather(fi, std::move(m));
    }
    drain();
    parse.report(info);
    for (mc_builder* b : db.bs) if (mc_build_finish(b, nullptr) != MC_OK) throw std::runtime_error(mc_build_last_error(b));
    if (info)
        std::cout << "Added " << db.targets.size() - initTargets << " reference sequences in "
                  << std::chrono::duration<double>(clock::now() - t0).count() << " s" << std::endl;

    // try_to_rank_unranked_targets (building.cpp:196-232)
    {
        std::set<uint32_t> unranked;
        for (uint32_t t = 0; t < db.targets.size(); ++t) if (o.resetParents || db.targets[t].parent == 0) unranked.insert(t);
        if (!unranked.empty()) {
            if (info) std::cout << unranked.size() << " targets are unranked (no taxon was assigned)." << std::endl;
            // MCQ_TAXMAP_DEVICE=1: the library finds every name's first row; what it found is applied as the loop below applies it
            TaxmapStep step;
            const auto r0 = clock::now();
            const bool onDevice = step.on && step.run(o.mapPost, name2tgt, unranked);
            step.report(onDevice, info);
            if (onDevice) {
                if (info) for (const auto& file : step.tried) std::cout << "Try to map sequences to taxa using '" << file << "'" << std::endl;
                size_t i = 0;
                for (const auto& kv : name2tgt) {
                    const uint32_t t = kv.second;
                    if (step.position[i] != ~0ull && unranked.count(t)) {
                        db.targets[t].parent = step.taxid[i];
                        for (mc_builder* b : db.bs) mc_build_set_parent(b, (uint64_t)t, step.taxid[i]);
                    }
                    ++i;
                }
            }
            else for (const auto& file : o.mapPost) {
                // rank_targets_with_mapping_file (building.cpp:80-150): rows "accession accession.version taxid gi" after one header line
                std::ifstream is(file);
                if (!is.good()) continue;
                if (info) std::cout << "Try to map sequences to taxa using '" << file << "'" << std::endl;
                std::string acc, accver, gi; uint64_t taxid = 0;
                std::getline(is, acc); acc.clear();
                auto with_name = [&](const std::string& n) -> int64_t { if (n.empty()) return -1; auto i = name2tgt.find(n); return i == name2tgt.end() ? -1 : (int64_t)i->second; };
                auto with_similar = [&](const std::string& n) -> int64_t {
                    if (n.empty()) return -1;
                    auto i = name2tgt.upper_bound(n);
                    if (i == name2tgt.end() || i->first.compare(0, n.size(), n) != 0) return -1;
                    return (int64_t)i->second; };
                while (is >> acc >> accver >> taxid >> gi) {
                    int64_t t = with_name(accver);
                    if (t < 0) { t = with_similar(acc); if (t < 0) t = with_name(gi); }
                    if (t >= 0) {
                        auto u = unranked.find((uint32_t)t);
                        if (u != unranked.end()) {
                            db.targets[t].parent = (int64_t)taxid;
                            for (mc_builder* b : db.bs) mc_build_set_parent(b, (uint64_t)t, (int64_t)taxid);
                            unranked.erase(u);
                            if (unranked.empty()) break;
                        }
                    }
                }
                if (unranked.empty()) break;
            }
            if (std::getenv("MCQ_PROFILE"))
                std::cerr << "mcq profile: ranking pass " << std::chrono::duration<double>(clock::now() - r0).count() << " s on the " << (onDevice ? "device" : "host") << "\n";
        }
        size_t still = 0;
        for (const auto& t : db.targets) if (t.parent == 0) ++still;
        if (info) {
            if (!still) std::cout << "All targets are ranked (have a taxon assigned)." << std::endl;
            else std::cout << still << " targets remain unranked (no taxon was assigned)." << std::endl;
        }
    }
    // post_process_features (building.cpp:550-566): -remove-ambig-features, after the targets got their final parents
    if (o.removeAmbigRank != kNumRanks && db.nonTarget.size() > 1) {
        if (info) std::cout << "\nRemoving ambiguous features on rank " << kRankNames[o.removeAmbigRank] << "... " << std::flush;
        std::unordered_map<int64_t, uint32_t> byId;
        for (uint32_t i = 0; i < db.nonTarget.size(); ++i) byId.emplace(db.nonTarget[i].id, i);
        // the target's entry of that rank in its ranked lineage (taxonomy::make_ranks, taxonomy.hpp:576-597): the last taxon of the
        // rank on the way to the root; 0 = none
        std::vector<uint32_t> anc(db.targets.size(), 0);
        for (uint32_t t = 0; t < db.targets.size(); ++t) {
            if (o.removeAmbigRank == 0) { anc[t] = t + 1; continue; }
            int64_t id = db.targets[t].parent;
            while (id != 0) {
                auto it = byId.find(id);
                if (it == byId.end()) break;
                const Taxon& p = db.nonTarget[it->second];
                if (p.rank == o.removeAmbigRank) anc[t] = it->second + 1;
                if (p.parent == id) break;
                id = p.parent;
            }
        }
        uint64_t old = 0, rem = 0;
        for (mc_builder* b : db.bs) {
            uint64_t k = 0, v = 0, r = 0;
            mc_build_counts(b, &k, &v); old += k;
            if (mc_build_remove_ambiguous(b, anc.data(), anc.size(), (uint32_t)std::max(0, o.maxAmbig), &r) != MC_OK) throw std::runtime_error(mc_build_last_error(b));
            rem += r;
        }
        if (info) std::cout << rem << " of " << old << "." << std::endl;
    }
}

}  // namespace mcq
#endif
