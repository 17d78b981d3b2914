/* metacache_amd.h -- C ABI of the MI355X-native MetaCache query hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no C++ / torch types.
 * Every entry point names the reference interface (file:line under muellan/metacache src/) it
 * replaces.  The library behind it is hand-written HIP for gfx950; there is NO CPU fallback: every
 * call that needs the GPU fails with MC_ERR_HIP if no device is usable.
 *
 * Pipeline per batch of queries (a query = one read or one read pair), details in DESIGN.md §3:
 *   plan / scan          : windows per query -> offsets
 *   sketch_lane          : one lane per short read: rolling canonical k-mers -> min-hash sketches
 *   chunk_sketch / probe : long single reads, one lane per window
 *   probe_cands          : one lane per query: bucket lookups, location list, sort, window-range candidates, top-K
 *   mid_cands            : lists of 33..256 locations, 4 / 8 / 16 lanes per query, register sort
 *   hash_cands           : lists of 65..256 locations, one wave per query, (target, window) counts in an LDS table
 *   big_filter / big_count : lists above 128 (RefSeq-scale tables): filtered by target, then counted
 *   query_wave / sort_candidates : one wave per query for everything else (and for -allhits)
 *   (semantics = reference CPU classifier, bit for bit)
 *
 * Threading: one mc_ctx per (process, device).  mc_batch_* calls are thread-safe for DISTINCT slots (one slot per host
 * thread, like one query_handler / query_host_data per thread in the reference, database_query.hpp:204-205,
 * query_batch.cuh:369-371).  Between mc_batch_submit and mc_batch_wait a slot borrows one of a few device pipes (stream +
 * workspace), so the copies and kernels of different slots overlap on the device.  mc_query_device and
 * mc_candidates_from_hits use the context's own pipe: one caller at a time.
 */
#ifndef METACACHE_AMD_H_
#define METACACHE_AMD_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* status codes: 0 ok, >0 recoverable, <0 fatal; nothing throws or exits across this ABI
 * (reference: C++ exceptions main.cpp:65-77, CUERR exit(1) cuda_helpers.cuh:18-26) */
#define MC_OK               0
#define MC_BATCH_FULL       1   /* mc_batch_add: query does not fit, submit first (query_batch.cuh:126-132) */
#define MC_ERR_INVALID     -1
#define MC_ERR_HIP         -2
#define MC_ERR_NOMEM       -3
#define MC_ERR_IO          -4
#define MC_ERR_UNSUPPORTED -5
#define MC_ERR_STATE       -6

#define MC_NUM_RANKS 21          /* taxonomy.hpp:103 */
#define MC_MAX_SKETCH 32         /* features per window handled on device */
#define MC_MAX_WINLEN 1024       /* characters per window handled on device */

typedef struct mc_ctx mc_ctx;

/* One top candidate = match_candidate minus the host pointer (candidate_structs.hpp:80-104).
 * Unused trailing entries of a query have hits == 0 (consumers stop at hits > 0, printing.cpp:291). */
typedef struct {
    uint32_t tgt;   /* target id                         */
    uint32_t hits;  /* number of location hits in range  */
    uint32_t beg;   /* first window of the range         */
    uint32_t end;   /* last window of the range (incl.)  */
} mc_candidate;

/* One location = database::location (database.hpp:136-166), always widened to 2 x u32 on device;
 * as a little-endian u64 it reads (tgt << 32) | win, i.e. location::operator< is integer <. */
typedef struct {
    uint32_t win;
    uint32_t tgt;
} mc_location;

typedef struct {
    int32_t  device;                 /* HIP device ordinal */
    /* query sketching (sketching_options, hash_dna.hpp:99-163); kmerlen must equal the DB's */
    uint32_t kmerlen;                /* <= 16 */
    uint32_t sketchlen;              /* <= MC_MAX_SKETCH */
    uint32_t winlen;                 /* <= MC_MAX_WINLEN */
    uint32_t winstride;
    /* candidate generation (candidate_structs.hpp:113-125) */
    uint32_t max_candidates;         /* K: output stride per query; '-maxcand 0' => caller passes a cap */
    /* table loading */
    uint32_t target_id_bytes;        /* 2 or 4: width of target_id in mc_load_batch values (config.hpp:56-62) */
    uint32_t num_parts;              /* database parts to be loaded (1..255; > 1: every part must be announced with
                                        mc_load_begin before the first mc_load_batch; target ids < 2^24) */
    uint32_t max_locations_per_feature; /* load-time truncation to the first n values (host_hashmap.hpp:454-466); 0 = keep */
    uint32_t remove_overpopulated;   /* load-time: empty buckets with more than n values (host_hashmap.hpp:480-495); 0 = off;
                                        mc_open_database clamps n to the DB's own bucket cap - 1 (mode_query.cpp:69-76) */
    float    max_load_factor;        /* hash table load factor (-max-load-fac, mode_query.cpp:49-55); 0 = default 0.3 */
    /* host batch slots (query_batch ctor, database_query.hpp:192-202) */
    uint32_t num_slots;
    uint32_t slot_max_queries;
    uint32_t slot_max_chars;
    uint32_t copy_allhits;           /* 1: sorted location lists are copied back too (-allhits) */
    int32_t  single_part;            /* mc_open_database: -1 = load every part; p >= 0 = only <name>.cache<p>, as one part
                                        (database::read singlePartId, database.cpp:196-205) -- one part per GPU */
    /* key sharding of ONE part over several GPUs ("Mode K"): only the features f with mc_key_owner(f, count) == index are
     * kept while loading; count <= 1 keeps everything.  A sharded context answers mc_query_device(MC_WANT_ALLHITS) with
     * the PARTIAL location lists of its keys; the union of all shards goes through mc_candidates_from_hits. */
    uint32_t key_shard_index;
    uint32_t key_shard_count;
    /* target-range sharding of ONE part over several GPUs ("Mode T"): mc_open_database keeps only the locations whose target lies in
     * range `index` of `count` CONTIGUOUS target-id ranges (cut where the targets' window counts -- the metadata's -- split into
     * equal shares: target t belongs to range floor(windows_before(t) * count / windows_total)); count <= 1 keeps everything.  The
     * load-time rules above are applied to the file's full bucket first, as on the whole table.  Every range keeps the full target
     * numbering and answers mc_query_* with the unchanged single-table path; the candidates of a read are disjoint between ranges,
     * so mc_merge_part_candidates over the ranges' top lists IN RANGE ORDER equals the whole table's list (mc_partset_open does
     * that when this count is > 1).  Not combinable with key shards or with several parts in one context. */
    uint32_t target_shard_index;
    uint32_t target_shard_count;
} mc_config;

void mc_config_default(mc_config* cfg);

/* lifetime ---------------------------------------------------------------------------------- */
int  mc_create(const mc_config* cfg, mc_ctx** out);
void mc_destroy(mc_ctx* ctx);
const char* mc_last_error(const mc_ctx* ctx);   /* ctx may be NULL: error of the last failed mc_create */

/* table loading: mirrors read_binary(is, featureStore_, partId, progress) (database.cpp:167-179)
 * = hash_multimap::deserialize (hash_multimap.hpp:970-1030), batch structure as in the file
 * (:1037-1082): per batch keys[n] (u32), sizes[n] (u8), values[sum sizes] packed
 * {window_id win (u32); target_id tgt (u16|u32)}. */
int mc_load_begin(mc_ctx* ctx, uint32_t part, uint64_t nkeys, uint64_t nvalues);
/* Optional, before the first mc_load_begin: the number of windows of every target (the reference knows them from its target metadata:
 * database.hpp target_count(), every target's source().windows, taxonomy.hpp:264-280).  When all windows of the database -- plus a gap
 * of 1024 numbers per target -- can be numbered in 32 bits (up to ~480 Gbp at the default window stride, whatever the single targets
 * look like) and the database is a single part, the table stores a location as ONE global window number
 *     gw = first_number(target) + window
 * in 4 bytes instead of the reference's 8-byte {win, tgt} (config.hpp:56-62 / candidate_structs.hpp:44-62): same order, same results,
 * half the bytes per location list in HBM and on the fabric -- a 2 x 10^10-location table takes 86 GB instead of 172.  A location
 * outside its target's announced windows makes mc_load_end fail (MC_ERR_INVALID).  mc_open_database and the builder's tables call
 * this themselves; mc_set_tuning(ctx, "compact_locations", 0) / MC_COMPACT_LOCATIONS=0 keep the 8-byte store. */
int mc_load_target_windows(mc_ctx* ctx, const uint32_t* windows_per_target, uint64_t num_targets);
/* the same announcement from bounds alone: targets 0 .. max_target_id with max_window_id + 1 windows each */
int mc_load_location_range(mc_ctx* ctx, uint32_t max_target_id, uint32_t max_window_id);
/* how the loaded table lies in HBM: layout[0] low 32 bits = bytes per stored location (8, or 4 with the compact store), bit 32 = 1 if the
 * table has its DIRECT-ADDRESS INDEX (2^32 entries of 8 bytes beside the buckets -- the feature is the index: one independent 8-byte
 * load per lookup of the lane path; built at mc_load_end for single-part tables whose buckets take 8 GiB and more where
 * 34 GB + head-room are free; mc_set_tuning "direct_index" 0 / 1 / -1, MC_DIRECT_INDEX), [1] low 32 bits = the gap
 * between two targets' window numbers in the compact form (0 otherwise), high 32 bits = the list alignment in entries (1, or 32 = every
 * list of the compact store begins on a 128-byte line: the loaders switch it on where the padded store stays below 1.5 x the plain one
 * and fits the device; mc_set_tuning "list_align" 0 / 1 / -1, MC_LIST_ALIGN), [2] = number of 64-byte buckets, [3] = entries of the list
 * store (lists of >= 2 with their padding; single locations live in their bucket) */
int mc_table_layout(const mc_ctx* ctx, uint64_t layout[4]);
/* the targets whose locations this context holds: range[0] <= target < range[1] (everything: 0 .. number of targets; a target-range
 * shard, mc_config.target_shard_*: its contiguous range, possibly empty); range[2] = features stored in the table, range[3] = locations */
int mc_target_range(const mc_ctx* ctx, uint64_t range[4]);
int mc_load_batch(mc_ctx* ctx, uint32_t part, const uint32_t* keys, const uint8_t* sizes,
                  const void* values, uint64_t nkeys_in_batch);
int mc_load_end(mc_ctx* ctx, uint32_t part);

/* convenience: database::read (database.cpp:183-242) -- reads <name>.meta (header, sketching,
 * taxonomy -> lineages) and every <name>.cache<p>, creates the context and loads all parts.  Query
 * sketching as adapt_options_to_database (querying.cpp:225-251): kmerlen always the DB's; sketchlen /
 * winlen == 0 => the DB's; winstride == 0 => winlen - kmerlen + 1 (not the DB's stride). */
int mc_open_database(const char* name, const mc_config* cfg, mc_ctx** out);
/* database::read with scope::metadata_only (database.cpp:183-242), what `info` mode needs (mode_info.cpp:55-230): taxa, sources,
 * lineages and the header fields for the mc_db_* calls -- no table, no device; query calls on it fail with MC_ERR_STATE. */
int mc_open_metadata(const char* name, mc_ctx** out);
/* how mc_open_database read the files of a single-part context (reader threads -> pinned slabs -> copy stream -> table kernels; the
 * reference reads every part in its own thread, database.cpp:203-226): stats[0..3] = bytes read, nanoseconds of the load in all, of its
 * index pass (the batches' places in the file), nanoseconds the device feeder waited for the reader threads.  MC_LOAD_THREADS: reader
 * threads (default 8); MC_LOAD_PIPELINE=0: the sequential loader. */
int mc_load_stats(const mc_ctx* ctx, uint64_t stats[4]);

/* target lineage table (ranked_lineages_of_targets, taxonomy.hpp:919-1030; uploaded like
 * copy_target_lineages_to_gpus gpu_hashmap.cu:1383-1396): lin[tgt*21 + rank] = taxon index + 1,
 * 0 = none.  Needed only for lowest_rank > 0 (taxon merging, candidate_generation.hpp:203-228). */
int mc_set_lineages(mc_ctx* ctx, const uint32_t* lin, uint64_t num_targets);

/* database facts after loading: info[0..7] = k, s, w, stride (target sketching), maxLocsPerFeature,
 * targetCount, partCount, locationCount (as stored on device) */
int mc_db_info(const mc_ctx* ctx, uint64_t info[8]);

/* taxonomy block of the .meta file as read by mc_open_database (taxonomy.hpp:702-728): taxa in file
 * order; 'taxon index' everywhere in this ABI = position in this list.  Targets are the taxa with
 * negative ids, id = -(target)-1 (taxonomy.hpp:930). */
int mc_db_num_taxa(const mc_ctx* ctx, uint64_t* n);
int mc_db_taxon(const mc_ctx* ctx, uint64_t index, int64_t* id, int64_t* parent, uint32_t* rank, const char** name);
/* file_source of a taxon (taxonomy.hpp:264-280; meaningful for targets): file name, sequence index in that file, window count */
int mc_db_taxon_source(const mc_ctx* ctx, uint64_t index, const char** filename, uint64_t* file_index, uint64_t* windows);
int mc_db_lineages(const mc_ctx* ctx, const uint32_t** lin, uint64_t* num_targets);

/* lineage table of EVERY taxon (taxonLineages_[taxon], taxonomy.hpp:1315-1322 = make_ranks of any taxon, :576-597): what
 * mc_evaluate_assignments compares two arbitrary taxa by.  Row x - 1 describes the taxon whose lineage entry is x (taxon index + 1).
 *   lin[(x-1) * MC_NUM_RANKS + r] = the ancestor-or-self of rank r as index + 1, 0 = none: the taxon itself in its own rank's slot if it
 *     has a rank, then the parent chain; a later (higher) ancestor of the same rank overwrites an earlier one; the walk ends at an
 *     unknown id or a self-parent.
 *   rank[x-1] = the taxon's rank, MC_NUM_RANKS = none (a larger value is read as none).  rank == NULL derives it from the rows: the slot
 *     that names the taxon itself, none if there is no such slot.
 *   covered[x-1] != 0: the taxon is a target or lies on the FULL parent chain, ranked or not, of at least one target
 *     (taxonomy_cache::covers, taxonomy.hpp:1355-1366, which walks make_lineage, not make_ranks).  covered may be NULL; then
 *     MC_EVALUATE_COVERAGE is MC_ERR_STATE.
 * mc_open_database and mc_open_metadata fill the table from the .meta taxonomy block (the targets' rows are the rows of mc_db_lineages).
 * mc_db_taxon_table hands the host copy out (rank and covered may be NULL; *covered = NULL where the table has none) and works on a
 * metadata-only context.  Setting a table DROPS the evaluation tallies; no evaluation may be in flight.
 * MC_ERR_INVALID: an entry above num_taxa, NULL lin with num_taxa > 0, more than 2^32 - 2 taxa. */
int mc_set_taxon_table(mc_ctx* ctx, const uint32_t* lin, const uint8_t* rank, const uint8_t* covered, uint64_t num_taxa);
int mc_db_taxon_table(const mc_ctx* ctx, const uint32_t** lin, const uint8_t** rank, const uint8_t** covered, uint64_t* num_taxa);

/* host batch slots: query_batch::add_paired_read (query_batch.cuh:85-186), database::query_gpu_async
 * (database.hpp:386-397), host_data.wait_for_results / allhits(i) / top_candidates(i) / clear
 * (query_batch.cuh:212-259); caller code database_query.hpp:87-124 */
int mc_batch_add(mc_ctx* ctx, uint32_t slot, const char* seq1, uint32_t len1, const char* seq2, uint32_t len2,
                 uint32_t max_windows_in_range);
/* many single-end queries at once: read i = seqs[offsets[i] .. offsets[i+1]); maxWindowsInRange is derived per read
 * from the database's window stride (candidate_structs.hpp:143-145) and insert_size_max.  Returns the number of reads
 * added (< n when the slot is full: submit, wait, clear, continue with the rest) or a negative error. */
int64_t mc_batch_add_bulk(mc_ctx* ctx, uint32_t slot, const char* seqs, const uint64_t* offsets, uint64_t n, uint64_t insert_size_max);
/* How the slots reach the device.  With two or more slots of up to 8 192 reads (and top candidates only: copy_allhits = 0) submissions
 * are QUEUED: a slot that finds a pipe free and nothing waiting goes out at once, everything else is taken by dispatcher threads of the
 * library -- whatever is waiting when a pipe comes free goes to the device as ONE batch (slots of the reference's size -- 4 096 reads,
 * options.hpp:229-232 -- are a chain of ~25 dependent steps and two host round trips for 0.1 ms of device work each; database_query.hpp:110-113
 * orders the submissions with a mutex instead; up to five dispatchers: the runtime's four hardware queues); larger slots and MC_SLOT_COALESCE=0: every slot its own batch (MC_SLOT_COALESCE=1: united whatever their size).  stats[0] = 1 if slots are united,
 * [1] = united batches sent so far, [2] = slots they carried, [3] = dispatcher threads. */
int mc_slot_stats(mc_ctx* ctx, uint64_t stats[4]);
/* "" or what the library has noticed about the HIP runtime in this process: the slot paths time their enqueue-only calls, and when these
 * take milliseconds apiece (the runtime's direct dispatch under many submitting threads: 3-4 x slower query phases at 150 Gbp)
 * the text names the remedy -- AMD_DIRECT_DISPATCH=0 in the process' environment before it starts.  Also printed once to stderr. */
const char* mc_runtime_warning(void);
int mc_batch_submit(mc_ctx* ctx, uint32_t slot, int lowest_rank);

typedef struct {
    uint32_t num_queries;
    uint32_t max_candidates;          /* stride of cands */
    const mc_candidate* cands;        /* [num_queries * max_candidates], slot-owned pinned memory */
    const uint64_t* hit_offsets;      /* [num_queries + 1] (NULL unless copy_allhits) */
    const mc_location* hits;          /* sorted (tgt,win) lists, query i = [hit_offsets[i], hit_offsets[i+1]) */
    const uint32_t* hit_counts;       /* [num_queries] number of location hits per query */
} mc_results;

int mc_batch_wait(mc_ctx* ctx, uint32_t slot, mc_results* out);  /* valid until mc_batch_clear(slot) */
int mc_batch_clear(mc_ctx* ctx, uint32_t slot);

/* device-resident entry point (what the slots call after their H2D copy; also used when reads are
 * already in HBM).  All pointers are DEVICE pointers.
 *   seq     : characters; every sequence starts 4-byte aligned; 16 readable slack bytes at the end
 *   qinfo   : [n][4] = {offset1, len1, offset2, len2} (offsets into seq; len2 = 0 for single reads)
 *   max_win : [n] maxWindowsInRange per query (candidate_structs.hpp:143-145), or NULL with
 *             max_win_uniform > 0
 * Results stay on device inside ctx-owned buffers (valid until the next call on this ctx):
 *   cands [n * max_candidates], hit_counts [n] (stride 4 words: {hits, features, found, probe steps}), and -- per
 *   flags -- hit_offsets [n+1] / hits, features.
 * 'stream' is a hipStream_t (NULL = the context's own stream); the call is asynchronous. */
typedef struct {
    const uint8_t*  seq;
    const uint32_t* qinfo;
    const uint32_t* max_win;
    uint32_t        max_win_uniform;
    uint32_t        num_queries;
    uint64_t        num_chars;        /* bytes in seq actually used (for checks) */
} mc_device_batch;

typedef struct {
    const mc_candidate* cands;
    const uint32_t*     hit_counts;
    const uint64_t*     hit_offsets;
    const mc_location*  hits;
    const uint32_t*     features;     /* [total_windows * sketchlen] window sketches, 0xFFFFFFFF padded */
    const uint32_t*     win_offsets;  /* [n+1] first window index of each query */
} mc_device_results;

#define MC_WANT_ALLHITS  1   /* keep the sorted location lists (hit_offsets / hits) */
#define MC_WANT_FEATURES 2   /* keep the window sketches (features) */
#define MC_WANT_PARTIAL_HITS 4 /* keep the location lists (hit_offsets / hits) in ANY order inside a list: what a key-sharded context hands to
                                 the exchange of Mode K (the owner sorts the union); unlike MC_WANT_ALLHITS this keeps the fast lane path */
#define MC_WANT_PARTIAL_NUMBERS 16 /* as MC_WANT_PARTIAL_HITS on a table with the compact location store, the lists left as the 4-byte global
                                 window numbers they are stored as: hit_offsets is filled, hits only for the reads the wave kernels took --
                                 mc_partial_numbers hands the numbers out (no decoding to (target, window) and back: 5.5 -> 0.6 ms per 10^6 reads) */
#define MC_SECOND_PIPE 8     /* run on the context's SECOND pipe (own stream, workspace and result buffers): one more caller thread may have a
                                 call in flight there while another runs on the first pipe, so the kernels of two batches overlap on the
                                 device the way several query_batch objects do in the reference (query_batch.cuh:369-371).  The
                                 results of a pipe stay valid until the next call on the SAME pipe. */
#define MC_DEFER_TAIL 32     /* TWO BATCHES IN FLIGHT FROM ONE CALLER THREAD: the call enqueues the batch's main kernels and returns without any
                                 synchronisation; what the host has to read device counters for (the sorted class of the filtered path, the
                                 segments of the exact wave kernels' leftovers: a few reads per million) is left to mc_query_finish on the
                                 same pipe, which the caller issues AFTER it has enqueued the next batch on the other pipe -- the device
                                 never waits for the host.  out->cands is complete once mc_query_finish has returned (in stream order).
                                 Honoured on the lane path without MC_WANT_* (small batches then skip their look at the work-list counters
                                 too and launch every kernel); otherwise the call does everything at once as without the flag
                                 (mc_query_finish is then a no-op).  A new mc_query_device -- and every other call that uses the first
                                 pipe's workspace: mc_candidates_from_*, mc_partial_numbers, mc_last_batch_stats -- runs a pending tail
                                 first; mc_destroy drops it.  INPUT LIFETIME: the tail reads the batch again (in->seq, in->qinfo,
                                 in->max_win): the caller's device buffers must stay valid and unchanged until mc_query_finish (or the
                                 call that runs the tail in its place) has returned. */
int mc_query_device(mc_ctx* ctx, const mc_device_batch* in, int lowest_rank, int flags,
                    mc_device_results* out, void* stream);
/* the tail of the last mc_query_device(MC_DEFER_TAIL) call on the first (flags = 0) or second (flags = MC_SECOND_PIPE) pipe: waits for
 * that batch's main kernels, then runs its rare classes on the same stream.  The reference gets the same overlap from several
 * query_batch objects, one stream each (query_batch.cuh:369-371, database_query.hpp:110-113). */
int mc_query_finish(mc_ctx* ctx, int flags);
/* waits for ONE pipe's stream (flags = 0: the first, MC_SECOND_PIPE: the second) -- what a two-pipe caller uses instead of mc_synchronize
 * (which waits for both) before it hands a finished batch's results to somebody else while the other pipe's batch is still running */
int mc_query_wait(mc_ctx* ctx, int flags);
int mc_synchronize(mc_ctx* ctx);

/* Mode P (one database part per GPU) and part groups.  Per-part candidate lists of the same reads (DEVICE pointers, [n][max_candidates]
 * each, in part order; target ids as mc_open_database with cfg.single_part leaves them: the database's own) -> one list per read, as if
 * the parts had been queried one after the other with one candidate list: host_hashmap.hpp:695-723 concatenates the parts' sorted
 * location lists, candidate_generation.hpp:172-231 inserts their candidates in that order (ties keep arrival order; lowest_rank > 0: one
 * entry per taxon, this context's lineages).  max_candidates <= 4.  out may be lists[0].  Asynchronous on 'stream'.
 * Replaces what the reference does across its GPUs for a partitioned database (gpu_hashmap.cu:1255-1290, query_batch.cu:464-527) and
 * `metacache merge` of per-part result files (mode_merge.cpp:247-296). */
int mc_merge_part_candidates(mc_ctx* ctx, const mc_candidate* const* lists, uint32_t num_lists, uint32_t num_queries, int lowest_rank,
                             mc_candidate* out, void* stream);

/* A partitioned database queried part group by part group (docs/partitioning.md:116-153, for databases beyond the node's HBM), the
 * parts of a group spread over GPUs (options.cpp:1155-1163 lists the reference's multi-GPU switches): `resident_parts` parts are in
 * HBM at a time -- one context each, part i of a group on devices[i % num_devices] -- and the NEXT group is loaded by a background
 * thread while the reads run against this one.  Per batch the reads are dealt out to the devices as owners; every device sends every
 * owner its parts' top lists of that owner's reads (one grouped ncclSend / ncclRecv round: RCCL, one communicator rank per device,
 * ncclCommInitAll) and every owner merges its reads' lists in part order (mc_merge_part_candidates), together with the list the earlier
 * groups left, and copies its share to the host (the reference forwards running top candidates GPU -> GPU, query_batch.cu:638-652).  Two
 * batches are in flight; mc_partset_classify_resident may be called from several threads at once.  devices == NULL: cfg->device alone.  cfg: as for mc_open_database (slot_max_queries / slot_max_chars = batch size).
 * cfg->target_shard_count > 1: the "parts" are the contiguous target ranges of ONE part file (cfg->single_part, or part 0), cut at load
 * (mc_config.target_shard_*); everything else -- groups, gather, merge in range order -- is the same. */
typedef struct mc_partset mc_partset;
int  mc_partset_open(const char* name, const mc_config* cfg, uint32_t resident_parts, const int32_t* devices, uint32_t num_devices, mc_partset** out);
void mc_partset_close(mc_partset* ps);
/* info[0..5] = parts, resident parts, groups, devices, nanoseconds the loader thread spent loading, nanoseconds the queries waited for it */
int  mc_partset_info(const mc_partset* ps, uint64_t info[6]);
/* all n reads (read i = seqs + offs[i] .. offs[i + 1]; seqs2 / offs2: the mates, NULL for single reads) against every part;
 * out[n][max_candidates] in HOST memory; insert_max as -insertsize (maxWindowsInRange, candidate_structs.hpp:143-145) */
int  mc_partset_classify(mc_partset* ps, const char* seqs, const uint64_t* offs, const char* seqs2, const uint64_t* offs2, uint64_t n,
                         int lowest_rank, uint64_t insert_max, mc_candidate* out);
/* The same in the caller's hands, for reads that STREAM (mcq -resident-parts): mc_partset_select_group makes part group g resident (groups in
 * order 0, 1, ...: group g + 1 loads behind group g's queries, every part by its own reader threads, one loading thread per device --
 * database.cpp:203-226 reads every part in a thread of its own); mc_partset_classify_resident takes a batch of reads through the parts of
 * the resident group only and merges their lists behind the list the earlier groups left in inout (has_prior != 0) -- the caller keeps
 * 16 bytes x max_candidates per read between the groups, nothing else.  mc_partset_load_bytes: bytes of .cache files the group loads read. */
int  mc_partset_select_group(mc_partset* ps, uint32_t group);
int  mc_partset_classify_resident(mc_partset* ps, const char* seqs, const uint64_t* offs, const char* seqs2, const uint64_t* offs2, uint64_t n,
                                  int lowest_rank, uint64_t insert_max, int has_prior, mc_candidate* inout);
int  mc_partset_load_bytes(const mc_partset* ps, uint64_t* bytes);
const char* mc_partset_last_error(const mc_partset* ps);

/* Mode K.  Owner shard of a feature (independent of the table's own bucket hash). */
uint32_t mc_key_owner(uint32_t feature, uint32_t shard_count);
/* rows 8-10 on location lists that are already gathered (DEVICE pointers; query i = hits[hit_offsets[i] .. hit_offsets[i+1]),
 * any order inside a list, e.g. the concatenated partial lists of all key shards): sort by (tgt, win), best window range per
 * target, top candidates -- query_handler.hpp:75-101 + candidate_generation.hpp:47-231 on a single-part list.
 * Results as mc_query_device (out->cands; out->hits / hit_offsets = the sorted lists).  Asynchronous on 'stream'. */
typedef struct {
    const mc_location* hits;
    const uint64_t*    hit_offsets;   /* [n + 1] */
    const uint32_t*    max_win;       /* [n] or NULL with max_win_uniform > 0 */
    uint32_t           max_win_uniform;
    uint32_t           num_queries;
} mc_device_hits;
int mc_candidates_from_hits(mc_ctx* ctx, const mc_device_hits* in, int lowest_rank, mc_device_results* out, void* stream);
/* Mode K owner side in ONE call, everything on the device: the partial lists of num_sources key shards for this rank's num_queries
 * reads -- counts[s * num_queries + i] locations of read i from source s; each source's locations back to back in read order, the
 * sources' blocks back to back in hits (exactly what an all-to-all-v of the shards' sorted partial lists delivers; total_hits = its
 * receive size, known to the host from the split sizes) -- are concatenated per read and go through rows 8-10: united lists of more
 * than 256 locations through the target filter and the (target, window) counting of the replicated mode (the union buffer standing
 * in for the table's location store), the others through the sort of mc_candidates_from_hits.  out->hits / hit_offsets = the united
 * lists (sorted only where the sort ran).  Replaces the reference's per-part forwarding chain (query_batch.cu:464-527, :638-652). */
typedef struct {
    const uint32_t*    counts;        /* [num_sources * num_queries] */
    const mc_location* hits;          /* [total_hits] */
    uint64_t           total_hits;
    const uint32_t*    max_win;       /* [num_queries] or NULL with max_win_uniform > 0 */
    uint32_t           max_win_uniform;
    uint32_t           num_queries;
    uint32_t           num_sources;
} mc_device_partial_hits;
int mc_candidates_from_partial_hits(mc_ctx* ctx, const mc_device_partial_hits* in, int lowest_rank, mc_device_results* out, void* stream);
/* Mode K with 4-BYTE locations on the wire.  What travels between the key shards is the compact location store's own form of a
 * location, the global window number gw = gwBase[target] + window (every context of one database numbers the windows of ALL targets the
 * same way: the numbering comes from the targets' window counts in the metadata).  Needs a single-part database whose windows can be
 * numbered in 32 bits (mc_load_target_windows; MC_ERR_UNSUPPORTED otherwise: use the 8-byte calls above).
 *
 * Shard side, after mc_query_device(MC_WANT_PARTIAL_HITS) on a key-sharded context (such a call looks up only the features the shard
 * owns): res's partial lists as numbers, back to back in read order, and the per-read counts -- the piece for the owner of reads
 * [lo, hi) is the contiguous range numbers[cut(lo) .. cut(hi)).  cut_offsets[i] (HOST) = first number of read cut_queries[i]
 * (cut_queries[i] <= num_queries): the split sizes of the all-to-all-v, the one host round trip of the exchange.  out's pointers
 * are ctx-owned device memory, valid until the next mc_partial_numbers call; filled asynchronously on 'stream'.
 * Replaces query_batch.cu:464-527 (the reference forwards the sketches from GPU to GPU and accumulates per-part results). */
typedef struct {
    const uint32_t* counts;       /* device [num_queries] */
    const uint32_t* numbers;      /* device [total] */
    uint64_t        total;
} mc_device_partial_numbers;
int mc_partial_numbers(mc_ctx* ctx, const mc_device_results* res, uint32_t num_queries, const uint32_t* cut_queries, uint32_t num_cuts,
                       uint64_t* cut_offsets, mc_device_partial_numbers* out, void* stream);
/* Owner side in ONE call: rows 8-10 on the pieces num_sources (<= 64) key shards sent for this rank's num_queries reads --
 * counts[s * num_queries + i] numbers of read i from source s, each source's numbers back to back in read order, source s' block
 * at numbers[source_offsets[s] .. source_offsets[s + 1]) (source_offsets on the HOST: the receive displacements).  No union copy:
 * the receive buffer stands in for the table's location store, every source's piece is one list of the read; lists of more than
 * 64 locations take the filtered path of the replicated mode (gw_filter / gw_count / sorted lists), the rest and what that path
 * hands back are decoded to (target, window) and sorted.  'numbers' must stay untouched until the results have been copied out and
 * must be readable 16 bytes past its end.  Results as mc_query_device (out->cands).
 * Replaces query_batch.cu:638-652 + the candidate generation of gpu_hashmap.cu:1255-1290 across the reference's GPUs. */
typedef struct {
    const uint32_t* counts;          /* device [num_sources * num_queries] */
    const uint32_t* numbers;         /* device */
    const uint64_t* source_offsets;  /* HOST [num_sources + 1] */
    const uint32_t* max_win;         /* device [num_queries] or NULL with max_win_uniform > 0 */
    uint32_t        max_win_uniform;
    uint32_t        num_queries;
    uint32_t        num_sources;
} mc_device_partial_numbers_in;
int mc_candidates_from_partial_numbers(mc_ctx* ctx, const mc_device_partial_numbers_in* in, int lowest_rank, mc_device_results* out, void* stream);
/* the same on the context's first (flags = 0) or second (flags = MC_SECOND_PIPE) pipe: a caller that keeps two batches in flight (keyset.cpp's
 * lanes) runs a batch's shard side -- mc_query_device(MC_WANT_PARTIAL_NUMBERS | pipe), mc_partial_numbers -- and its owner side on the same pipe */
int mc_candidates_from_partial_numbers_on(mc_ctx* ctx, const mc_device_partial_numbers_in* in, int lowest_rank, int flags, mc_device_results* out, void* stream);
/* what mc_candidates_from_partial_numbers has done on this context so far: stats[0..3] = reads, reads whose pieces took the filtered path,
 * numbers received, locations decoded for the sort (short lists + what the filtered path handed back) */
int mc_owner_stats(const mc_ctx* ctx, uint64_t stats[4]);

/* ONE database key-sharded over the GPUs of the node, driven from C++ (what `mcq query -shard keys -gpus a,b,...` runs): shard s of
 * num_shards on devices[s % num_devices], one context each (mc_open_database with key_shard_index / key_shard_count).  Per batch
 * every shard looks its own features up for ALL reads (mc_query_device(MC_WANT_PARTIAL_HITS)), the partial lists travel as 4-byte
 * numbers to the shard that owns the read (contiguous read shards; grouped ncclSend / ncclRecv = all-to-all-v over RCCL/xGMI between
 * devices, device-to-device copies between shards of one device), and the owner runs rows 8-10 (mc_candidates_from_partial_numbers).
 * RCCL is used when num_shards == num_devices > 1 (or MC_KEYSET_RCCL=1 with one shard: the same calls with a single rank);
 * several shards on one device are what a single-GPU box can test.  num_shards == 0: one per device.
 * Reference: gpu_hashmap.cu:1255-1290, query_batch.cu:464-527 (its parts-over-GPUs query), options.cpp:1155-1163. */
typedef struct mc_keyset mc_keyset;
int  mc_keyset_open(const char* name, const mc_config* cfg, uint32_t num_shards, const int32_t* devices, uint32_t num_devices, mc_keyset** out);
void mc_keyset_close(mc_keyset* ks);
/* info[0..7] = shards, devices, 1 if the exchange runs over RCCL, locations of all shards, numbers sent through the exchange so far, batches,
 * reads whose pieces took the filtered path on their owner, locations decoded for the sort (mc_owner_stats summed over the shards) */
int  mc_keyset_info(const mc_keyset* ks, uint64_t info[8]);
/* as mc_partset_classify: out[n][max_candidates] in HOST memory */
int  mc_keyset_classify(mc_keyset* ks, const char* seqs, const uint64_t* offs, const char* seqs2, const uint64_t* offs2, uint64_t n,
                        int lowest_rank, uint64_t insert_max, mc_candidate* out);
const char* mc_keyset_last_error(const mc_keyset* ks);

/* copies out of the ctx-owned result buffers, asynchronous on the context's stream
 * (kind: 0 = device -> device, 1 = device -> host); mc_synchronize waits for both pipes' streams */
int mc_copy_results(mc_ctx* ctx, void* dst, const void* src, uint64_t bytes, int kind);
/* the same on the caller's stream (the one its mc_query_device call ran on; NULL = the context's, or with kind | MC_SECOND_PIPE the
 * second pipe's own stream: results of a mc_query_device(MC_SECOND_PIPE) call that was given no stream).
 * kind 2 = host -> device: a caller whose reads lie in pinned host memory uploads batch i + 1 on the pipe it will run on while batch i's
 * kernels run on the other pipe (cudaMemcpyAsync of query_batch's host buffers, query_batch.cu:330-360) */
int mc_copy_results_on(mc_ctx* ctx, void* dst, const void* src, uint64_t bytes, int kind, void* stream);
/* device memory (kind 0) and pinned host memory (kind 1) on the context's device, for callers that do not link the HIP runtime themselves
 * (mcq's build step): with mc_copy_results_on and mc_synchronize they fill and read the arrays of the device forms.  The
 * memory is the caller's until mc_buffer_free (same kind; NULL, another kind or a context without a device: nothing happens); the context
 * keeps no list of it, so the kind is the caller's word.  Device memory is 256-byte aligned.
 * MC_ERR_INVALID: NULL ctx or out, bytes == 0, another kind; MC_ERR_STATE: a context without a device; MC_ERR_NOMEM. */
int  mc_buffer_alloc(mc_ctx* ctx, uint64_t bytes, int kind, void** out);
void mc_buffer_free(mc_ctx* ctx, void* p, int kind);

/* tuning / test hook (not needed for normal use): the switches the MC_BIG_MIN / MC_QUAD_LOOKUP / MC_NO_LANE_PATH environment variables
 * set at mc_create, on a live context with no batch in flight.  names: "big_min" (location lists longer than this are filtered by
 * target before they are counted, big_filter_kernel), "quad_lookup" (-1 by table size, 0 / 1), "lane_path" (0 / 1), "compact_locations" (0 / 1, before mc_load_begin),
 * "filter_bpc" / "count_bpc" (blocks per CU of the filter kernels' / the first counting instance's persistent grids, 0 = default; this context only),
 * "gw_fuse" (counting inside the filter kernel: 1 = default, 0 = the two kernels apart, 5 / 6 = the fused kernel's five- / six-waves-per-SIMD instances; the default runs at seven),
 * "gw_big_h" (reads beyond this many locations take the fine-block instance of the stream filter; default 32 768, 0 = none),
 * "lane_fusion" (sketching + lookups of the lane path in one kernel: -1 = on tables beyond 1 GiB (default), 0 / 1 = never / always),
 * "direct_index" (-1 by table size, 0 / 1; on a loaded table the index is built or dropped at once: mc_table_layout),
 * "filter_lookup" (the lane path's direct-index lookups inside the filter kernel, the lane kernel only sketches: -1 (default) = on tables
 *   with the compact store whose direct index the size rule built (bucket table of 8 GiB or more), for calls that launch every kernel
 *   without a host look at the work-list counters (MC_DEFER_TAIL or more than 2^20 reads), ask for top candidates only and give ONE window
 *   range of at most 3 for all reads (max_win NULL: single reads of up to two windows -- the batches it was measured faster on; batches
 *   with a range per read were measured slower with it, read pairs not at all);
 *   0 = never; 1 = wherever a direct index exists, whatever the batch size -- tests and A/B runs),
 * "list_align" (before the table is loaded: the compact store's lists on 128-byte lines of their own, mc_table_layout).
 * Every value of every switch gives the same results (tests/test_gpu_variants.py and the variant loops of test_gpu_scale.py /
 * test_gpu_reference_midscale.py run them against the goldens, the oracle and the reference). */
int mc_set_tuning(mc_ctx* ctx, const char* name, int64_t value);

/* semi-global alignment of reads to subjects on the device, as `metacache query -align` computes it on the host (alignment.hpp:177-276,
 * make_semi_global_alignment classification.cpp:76-100): match +2, mismatch -1, gap -1 on the characters as they are; free end gaps; ties
 * fall to diag, then above, then left; the end cell is the corner unless a cell of the last column, then of the last row, is strictly
 * greater.  Problem i is read i = reads[read_off[i] .. read_off[i+1]), its mate (mates may be NULL: no mates; an empty mate counts as
 * none) and subject i.  Read 1 is aligned forward and reverse-complemented (case kept, U -> A); the mate's two scores are added to
 * them as unsigned 64-bit numbers (a negative score wraps, as in the reference), forward is shown when its sum is strictly greater:
 * reversed[i] = 0, else 1.  score_fwd / score_rev are read 1's own scores, mate_fwd / mate_rev the mate's (0 without one).
 * The shown alignment's two strings (gaps are '_', equal lengths, at least one column) go to aligned[aligned_off[i] .. aligned_off[i+1]):
 * first half the aligned read, second half the aligned subject; aligned_off (n + 1 numbers) is FILLED by the call, aligned_cap must be
 * at least the sum of 2 * max(1, len_read + len_subject).  Works on any context, with or without a loaded table, from several threads at
 * once.  A call goes to the device in sub-batches whose output and scratch stay under mc_set_tuning "align_scratch_mb" (default 512;
 * one problem alone always goes): reads up to 256 against subjects up to 512 characters keep their trace in LDS, longer ones in device
 * scratch, 2 bits per cell. */
int mc_align_semiglobal(mc_ctx* ctx, const char* reads, const uint64_t* read_off, const char* mates, const uint64_t* mate_off,
                        const char* subjects, const uint64_t* subj_off, uint64_t n, int32_t* score_fwd, int32_t* score_rev,
                        int32_t* mate_fwd, int32_t* mate_rev, uint8_t* reversed, char* aligned, uint64_t aligned_cap, uint64_t* aligned_off);
/* stats[0..3] = problems aligned on this context, matrix cells of read 1 (len_read * len_subject summed), nanoseconds of the alignment
 * kernels (HIP events around each sub-batch's launches), sub-batches */
int mc_align_stats(const mc_ctx* ctx, uint64_t stats[4]);

/* ---- classification: one taxon per read from its top candidates ---------------------------------
 * The reference's ranked-LCA vote (classification.cpp:146-189; -hitmin, -hitdiff, -lowest, -highest) on the device, for candidate
 * lists of any producer: mc_query_device (either pipe), mc_candidates_from_*, mc_merge_part_candidates, or -- with MC_CLASSIFY_HOST --
 * the host arrays of mc_batch_wait, mc_partset_* and mc_keyset_*.  Needs the lineage table (mc_open_database reads it from the .meta
 * file; mc_set_lineages otherwise); a slot's index in a lineage is the taxon's rank.
 *   A read's list is cands[i * stride .. i * stride + stride) up to the first entry with hits == 0; an empty list is unclassified.
 *   tax(c) = lineage slot 0 of c.tgt for lowest_rank 0, else its first non-zero slot at lowest_rank or above; a tgt beyond the
 *   lineage table has a lineage of zeros.  No tax(cand[0]), or cand[0].hits < hits_min: unclassified.
 *   threshold = cand[0].hits > hits_min ? (float)(cand[0].hits - hits_min) * hits_diff : 0.0f  (unsigned difference, one float
 *   multiply); candidates 1, 2, ... vote as long as (float)hits > threshold, the first one that is not ends the vote.  hits_diff is the
 *   FACTOR: the command line's rule "a value above 1 is a percentage" (options.cpp:1312) is the caller's.
 *   Every voter moves the result up the top candidate's lineage: from the current rank r (at first the slot tax(cand[0]) came from) to the
 *   first r' >= r where the top candidate's lineage is non-zero and equal to the voter's.  None, or r' > highest_rank: unclassified.
 *   At the end r > highest_rank is unclassified as well; otherwise the read is assigned the top candidate's lineage slot r. */
typedef struct {
    uint32_t hits_min;               /* -hitmin */
    float    hits_diff;              /* -hitdiff as a factor; finite, >= 0 */
    int32_t  lowest_rank;            /* -lowest,  0 .. MC_NUM_RANKS - 1 */
    int32_t  highest_rank;           /* -highest, lowest_rank .. MC_NUM_RANKS - 1 */
} mc_classify_options;
void mc_classify_options_default(mc_classify_options* opt);      /* {0, 1.0f, 0, MC_NUM_RANKS - 1} */

typedef struct {
    uint32_t taxon;                  /* taxon index + 1 as in the lineage table; 0 = unclassified */
    uint32_t info;                   /* bits 0-7: rank (MC_NUM_RANKS = unclassified); bits 8-15: voters = candidates that entered the vote,
                                        the top one included (0 if unclassified; 255 stands for 255 and more) */
} mc_assignment;

#define MC_CLASSIFY_HOST  1          /* cands / out are HOST arrays: staged through device buffers of the context, the call returns when out is filled */
#define MC_CLASSIFY_TALLY 2          /* add this call's reads to the context's tallies (mc_classify_tally) */
/* out[i] = the assignment of read i.  Without MC_CLASSIFY_HOST cands and out are DEVICE pointers (8-byte aligned) and the call is
 * asynchronous on 'stream' (a hipStream_t; NULL = the context's own): enqueued behind the call that made the candidates it needs no
 * synchronisation in between.  out must not overlap cands.  Calls on different streams may run -- and tally -- at the same time.
 * The lineage table goes to the device with the first call and again after a later mc_set_lineages (which also clears the tallies;
 * no classification may be in flight then).
 * MC_ERR_INVALID (checked first): NULL ctx or options, NULL arrays with num_queries > 0, stride == 0, a rank outside
 * 0 .. MC_NUM_RANKS - 1, lowest_rank > highest_rank, hits_diff negative or not finite, unknown flags, out overlapping cands.
 * num_queries == 0: MC_OK, nothing is done.  MC_ERR_STATE: a context without lineages, or without a device (mc_open_metadata). */
int mc_classify_candidates(mc_ctx* ctx, const mc_classify_options* opt, const mc_candidate* cands, uint32_t num_queries,
                           uint32_t stride, int flags, mc_assignment* out, void* stream);
/* the tallies of all MC_CLASSIFY_TALLY calls since the last reset, exact 64-bit sums: assigned[r] = reads whose result has rank r
 * (assigned[MC_NUM_RANKS] = unclassified reads); taxon_counts[x] = reads assigned to the taxon with lineage entry x (= taxon index + 1;
 * what -abundances counts per taxon), of which the first min(capacity, *num_counts) are copied; *num_counts = 1 + the largest entry of
 * the lineage table.  assigned, taxon_counts (with capacity 0) and num_counts may be NULL.  Waits for the context's own streams; a caller
 * that classified on streams of its own synchronises them first.  reset != 0 clears the counters after they have been read. */
int mc_classify_tally(mc_ctx* ctx, uint64_t assigned[MC_NUM_RANKS + 1], uint64_t* taxon_counts, uint64_t capacity,
                      uint64_t* num_counts, int reset);

/* ---- evaluation against a ground truth: -precision / -taxon-coverage ---------------------------------
 * The last block of the reference's query summary (classification.cpp:237-295 update_coverage_statistics / evaluate_classification,
 * classification_statistics.hpp:87-107 assign_known_correct, printed by printing.cpp:537-592) on the device: given what each read was
 * assigned and what it really is, how many reads were classified correctly and wrongly on every rank, and how many hits fell on taxa
 * the database does not cover.  Needs the taxon table (mc_set_taxon_table; rank[], lin[][] and covered[] below are its arrays, a rank of
 * MC_NUM_RANKS = 21 is "none").  Per read i, with a = assigned[i].taxon and t = truth[i] (taxon index + 1, 0 = none / unknown):
 *   1. an entry greater than the table's num_taxa is treated as 0 and counted once in out_of_table.
 *   2. ar = a ? rank[a-1] : 21.  The TABLE's rank: assigned[i].info is not read, so assignment arrays of any producer work.
 *   3. kr = t ? rank[t-1] : 21.  A truth without a rank counts as unknown (mcq's ground truth hands over the next ranked ancestor,
 *      classification.cpp:109-137; resolving read headers stays the caller's).
 *   4. cr = 21; if a and t: the first slot r = 0 .. 20 with lin[a-1][r] != 0 && lin[a-1][r] == lin[t-1][r] gives
 *      cr = rank[that taxon - 1]  (ranked_lca, taxonomy.hpp:1291-1301, then ->rank()).
 *   5. assign_known_correct: cr = max(cr, ar, kr); assigned[ar]++; known[kr]++; if kr != 21: correct[cr]++, and if cr > kr && cr > ar:
 *      wrong[cr-1]++ ("counted wrong").
 *   6. verdicts[i] = {kr, cr, counted wrong ? 1 : 0, 0} where verdicts is given.
 *   7. with MC_EVALUATE_COVERAGE and t != 0: for every slot with x = lin[t-1][r] != 0, rr = rank[x-1] and on = (a != 0 && rr >= ar);
 *      coverage[rr] counts a true_pos (covered[x-1], on), false_neg (covered, not on), false_pos (not covered, on) or true_neg
 *      (update_coverage_statistics, classification.cpp:237-263).
 * Without MC_EVALUATE_HOST the arrays are DEVICE pointers (assigned 8-byte, truth and verdicts 4-byte aligned) and the call is
 * asynchronous on 'stream' (NULL = the context's own): enqueued behind mc_classify_candidates it needs no synchronisation in between.
 * Calls on different streams may tally at the same time; the counters are exact 64-bit sums and order-free.  With MC_EVALUATE_HOST the
 * arrays are staged in pieces through buffers of the context, one caller at a time (mc_set_tuning "evaluate_stage_rows": reads per
 * piece, 0 = default), and the call returns when done; one that fails on the device after its first piece has counted the pieces
 * before it.  The table goes to the device with the first call and again after a later mc_set_taxon_table.
 * MC_ERR_INVALID (checked first): NULL ctx, NULL assigned or truth with num_queries > 0, neither verdicts nor MC_EVALUATE_TALLY,
 * MC_EVALUATE_COVERAGE without MC_EVALUATE_TALLY, unknown flags, misaligned device arrays, verdicts overlapping an input.
 * num_queries == 0: MC_OK.  MC_ERR_STATE: no taxon table, MC_EVALUATE_COVERAGE without covered[], a context without a device. */
typedef struct { uint8_t known, correct, flags, reserved; } mc_verdict;     /* kr, cr, bit 0 of flags = counted wrong */
#define MC_EVALUATE_HOST     1       /* the arrays are HOST arrays, the call returns when done */
#define MC_EVALUATE_TALLY    2       /* add this call's reads to the context's evaluation tallies (mc_evaluate_tally) */
#define MC_EVALUATE_COVERAGE 4       /* with MC_EVALUATE_TALLY: also the confusion counters of -taxon-coverage (rule 7) */
int mc_evaluate_assignments(mc_ctx* ctx, const mc_assignment* assigned, const uint32_t* truth, uint32_t num_queries,
                            int flags, mc_verdict* verdicts, void* stream);
/* the tallies of all MC_EVALUATE_TALLY calls since the last reset (or the last mc_set_taxon_table): the per-rank bins as the rule above
 * fills them -- the cumulative figures of the summary (classification_statistics.hpp:135-227) are sums over them --, reads = reads
 * evaluated, out_of_table = entries of rule 1.  Waits for the context's own streams as mc_classify_tally does; reset != 0 clears the
 * counters after they have been read.  These counters are the evaluation's own: mc_classify_tally's are not touched. */
typedef struct {
    uint64_t assigned[MC_NUM_RANKS + 1], known[MC_NUM_RANKS + 1], correct[MC_NUM_RANKS + 1], wrong[MC_NUM_RANKS + 1];
    uint64_t coverage[MC_NUM_RANKS + 1][4];      /* true_pos, false_pos, true_neg, false_neg */
    uint64_t reads, out_of_table;
} mc_evaluation;
int mc_evaluate_tally(mc_ctx* ctx, mc_evaluation* out, int reset);

/* ---- target coverage: the two-pass classification of -cov-percentile ------------------------------
 * The reference (map_queries_to_targets_default, classification.cpp:747-838) keeps every read's candidates, collects per target the
 * windows that qualifying candidates cover (matches_per_target::insert, matches_per_target.hpp:100-127), removes the targets at the
 * low end of the coverage distribution (filter_targets_by_coverage, classification.cpp:591-634) and classifies every read again from
 * the candidates that are left (update_candidates, :660-671).  Here the covered windows of ALL targets are one bitmap in the context:
 * target t owns ceil(windows(t) / 32) 32-bit words of it.  Needs the targets' window counts (mc_open_database and the builder's tables
 * announce them; mc_load_target_windows otherwise) and the lineage table; MC_ERR_STATE without either, or without a device.
 * Announcing other window counts (mc_load_target_windows, mc_load_location_range) or other lineages (mc_set_lineages) DROPS the
 * accumulated coverage, its statistics and the keep mask; no coverage call may be in flight then.  (The calls that lay the bitmap out
 * again or replace the mask wait for the device and hold one mutex with the launches of mc_coverage_add / mc_coverage_drop, so a
 * host thread that marks or drops meanwhile launches on the old or on the new state, never on freed memory; what it marked is lost.)
 *   A read's list is cands[i * stride .. i * stride + stride) up to the first entry with hits == 0.  An entry QUALIFIES when
 *   hits >= hits_min and tax(c) != 0, tax(c) as for mc_classify_candidates above (lineage slot lowest_rank itself for rank 0, else the
 *   first non-zero slot from lowest_rank up; a tgt beyond the lineage table has none).  An entry that does not qualify is skipped and
 *   the walk goes on.  A qualifying entry marks the windows beg .. min(end, windows(tgt) - 1) of its target.  Entries with
 *   tgt >= the number of announced targets, with beg > end, or with windows at or beyond windows(tgt) mark only their in-range part (if
 *   any) and add one each to the out-of-range statistic.
 * Without MC_COVERAGE_HOST the arrays are DEVICE pointers (16-byte aligned) and the call is asynchronous on 'stream' (a hipStream_t;
 * NULL = the context's own): enqueued behind the call that made the candidates it needs no synchronisation in between, on either pipe.
 * Calls on different streams may mark at the same time.  (mc_set_tuning "coverage_load_first" 0: the marking kernel sends every mask out
 * as an atomic instead of loading the word first -- the same bitmap, kept for measurements)
 * MC_ERR_INVALID (checked first): NULL ctx, NULL arrays with num_queries > 0, stride == 0, lowest_rank outside 0 .. MC_NUM_RANKS - 1,
 * unknown flags.  num_queries == 0: MC_OK. */
#define MC_COVERAGE_HOST 1           /* cands (and out) are HOST arrays, staged in pieces as MC_CLASSIFY_HOST does; the call returns when done */
int mc_coverage_add(mc_ctx* ctx, const mc_candidate* cands, uint32_t num_queries, uint32_t stride, uint32_t hits_min,
                    int32_t lowest_rank, int flags, void* stream);
/* covered[t] = marked windows of target t, windows[t] = its announced window count (the denominators of classification.cpp:606-611):
 * the first min(capacity, *num_targets) of each are copied; either pointer, num_targets and stats may be NULL.  stats[0..3] =
 * qualifying entries that marked windows, out-of-range entries, bits set in the bitmap, mc_coverage_add calls -- since the last reset.
 * Waits for the context's own streams; a caller that marked on streams of its own synchronises them first.  reset != 0 clears the
 * bitmap and the statistics after they have been read (the keep mask stays). */
int mc_coverage_counts(mc_ctx* ctx, uint32_t* covered, uint32_t* windows, uint64_t capacity, uint64_t* num_targets,
                       uint64_t stats[4], int reset);
/* filter_targets_by_coverage (classification.cpp:591-634) on the host, no context: the targets are visited in 'order' (num_order ids;
 * NULL = ascending target id, all num_targets of them); those with covered == 0 are skipped and not kept; covP = (float)covered /
 * (float)windows, summed in float in visiting order; a STABLE sort ascending by covP; then, from the low end,
 * part += covP; if (part > percentile * sum) stop; else the target is dropped.  keep[t] = 1 exactly for visited targets that were not
 * dropped (keep has num_targets bytes).  MC_ERR_INVALID: percentile not finite or outside [0, 1] (the command line's rule "a value
 * above 1 is a percentage", options.cpp:1313, is the caller's), NULL arrays with num_targets > 0, an id >= num_targets or repeated.
 * The reference's own result additionally depends on the iteration order of its std::unordered_map (the visiting order, and with it
 * the rounding of the float sum) and on std::sort's order of equal values: that is why 'order' is a parameter, and why a caller that
 * must drop exactly the reference's targets (mcq) keeps this one step in the reference's containers. */
int mc_coverage_keep(const uint32_t* covered, const uint32_t* windows, uint64_t num_targets, const uint32_t* order,
                     uint64_t num_order, float percentile, uint8_t* keep);
/* the targets whose candidates mc_coverage_drop keeps: keep[t] != 0 for t < num_targets (copied to the device); NULL = no mask.
 * No mc_coverage_drop may be in flight. */
int mc_coverage_set_keep(mc_ctx* ctx, const uint8_t* keep, uint64_t num_targets);
/* update_candidates (classification.cpp:660-671): out row i = the entries of in row i (up to its first hits == 0) whose tgt is kept,
 * in their order, then zeros; a tgt beyond the mask is not kept.  out may be 'in' itself; any other overlap is MC_ERR_INVALID, as are
 * NULL ctx, NULL arrays with num_queries > 0, stride == 0 and unknown flags (MC_COVERAGE_HOST: host arrays).  MC_ERR_STATE when no
 * mask is set.  Device arrays are 16-byte aligned; asynchronous on 'stream' as mc_coverage_add. */
int mc_coverage_drop(mc_ctx* ctx, const mc_candidate* in, uint32_t num_queries, uint32_t stride, int flags, mc_candidate* out,
                     void* stream);

/* ---- per-target hit lists: -hits-per-ref -----------------------------------------------------------
 * The reference (matches_per_target::insert / sort, matches_per_target.hpp:104-136; printed by show_matches_per_targets,
 * printing.cpp:385-420) keeps, for every target, the (query id, window range, hits) of all qualifying candidates, sorted by window
 * range and then query id.  Here every qualifying candidate becomes one mc_target_hit in a LOG in device memory, and
 * mc_target_hits_collect sorts the log on the device and cuts it into one slice per target.  Needs the lineage table and a device;
 * MC_ERR_STATE without either.  A later mc_set_lineages DROPS what was accumulated and its statistics (the log keeps its size).
 *   Which entries are recorded is the rule of mc_coverage_add, to the letter: a read's list is cands[i * stride ..) up to the first
 *   entry with hits == 0; an entry QUALIFIES when hits >= hits_min and tax(c) != 0 (lineage slot lowest_rank itself for rank 0, else
 *   the first non-zero slot from lowest_rank up; a tgt beyond the lineage table has none); an entry that does not qualify is skipped
 *   and the walk goes on.  A qualifying entry becomes the record {tgt, beg, end, hits, query} with beg and end as they are (no window
 *   table is needed) and query = query_ids[i] if query_ids is given, else first_query_id + i.
 * mc_target_hits_reserve sizes the log to capacity_records (what it holds stays; MC_ERR_INVALID if that is more than the new size);
 * 0 frees the log and drops what was accumulated.  It waits for the device; no add may be in flight.
 * mc_target_hits_add without a flag: cands (16-byte aligned) and query_ids (8-byte aligned, or NULL) are DEVICE pointers and the call
 * is asynchronous on 'stream' (a hipStream_t; NULL = the context's own): enqueued behind the call that made the candidates it needs
 * no synchronisation in between.  It never allocates: records that find no room are NOT stored and are counted (stats[1]); without
 * a reserved log it returns MC_ERR_STATE.  Calls on different streams may append at the same time.
 * With MC_TARGET_HITS_HOST the arrays are HOST arrays, the call returns when done and one caller runs at a time (no device-mode add
 * may be in flight on another stream meanwhile).  Before anything is launched it makes room for num_queries * stride more records:
 * the log grows by doubling (a new allocation and a device-to-device copy), bounded by mc_set_tuning "target_hits_max_mb" (the log's
 * largest size in MiB, default 8192: 3.5 x 10^8 records; the sort's second buffer at collect time is not counted).  If room cannot
 * be made the call returns MC_ERR_NOMEM and has added NOTHING, so that the caller can keep that batch elsewhere; MC_ERR_STATE if the
 * log has dropped records before.
 * MC_ERR_INVALID (checked first): NULL ctx, NULL cands with num_queries > 0, stride == 0, lowest_rank outside 0 .. MC_NUM_RANKS - 1,
 * unknown flags, misaligned device arrays.  num_queries == 0: MC_OK. */
typedef struct { uint32_t tgt, beg, end, hits; uint64_t query; } mc_target_hit;   /* 24 bytes */
#define MC_TARGET_HITS_HOST 1        /* cands / query_ids are HOST arrays, staged in pieces as MC_COVERAGE_HOST does */
extern const uint32_t mc_target_hits_tile;   /* records one block sorts in LDS: the sort's pass count is ceil(log2(ceil(n / tile))) (for tests and tools) */
int mc_target_hits_reserve(mc_ctx* ctx, uint64_t capacity_records);
int mc_target_hits_add(mc_ctx* ctx, const mc_candidate* cands, const uint64_t* query_ids, uint64_t first_query_id,
                       uint32_t num_queries, uint32_t stride, uint32_t hits_min, int32_t lowest_rank, int flags, void* stream);
/* Waits for the context's stream and its second pipe's (the streams that NULL and MC_SECOND_PIPE callers enqueue on; a caller that
 * appended on any other stream -- its own, or a batch slot's -- synchronises that one first), sorts the log on the
 * device ascending by (tgt, beg, end, query, hits) -- compared lexicographically, query as a 64-bit number: a total order over the
 * fields, so the result is a pure function of the SET of records, whatever call order, streams and atomics did -- and returns
 * records[offsets[t] .. offsets[t + 1]) = target t's list; offsets[t + 1] - offsets[t] is the target's record count.
 * *num_targets = the lineage table's target count; offsets has *num_targets + 1 entries and capacity_targets says how many TARGETS it
 * has room for (capacity_targets + 1 entries); records has room for capacity_records.  A capacity smaller than the size is
 * MC_ERR_INVALID.  A SIZE QUERY is any call with both arrays NULL: it fills *num_targets, *num_records and stats (each may be NULL).
 * stats[0..3] = records stored, records dropped for lack of room, mc_target_hits_add calls, targets with at least one record --
 * since the last reset.  With stats[1] > 0 a call that asks for an array returns MC_ERR_STATE (after the sizes and stats have been
 * filled): a partial list must not pass for a whole one; the size query still answers, and resets.
 * reset != 0 clears the log and the statistics after they have been read (the log keeps its size).  A call that asks for neither an
 * array nor stats does not sort: with reset it is the cheap way to empty the log. */
int mc_target_hits_collect(mc_ctx* ctx, uint64_t* offsets, uint64_t capacity_targets, uint64_t* num_targets,
                           mc_target_hit* records, uint64_t capacity_records, uint64_t* num_records, uint64_t stats[4], int reset);

/* ---- mapping lines: the per-read output of `metacache query` ----------------------------------------
 * The reference prints one line per read (show_query_mapping, classification.cpp:432-523; show_candidates and show_candidate_ranges,
 * printing.cpp:283-380).  Here the lines of a whole batch are rendered on the device, behind the query and the vote.  Every text of a
 * line that depends on the taxonomy or on the output options (-taxids, -taxids-only, -omit-ranks, -lineage, -separate-cols, -separator,
 * -lowest, -highest) depends on the taxon or on the target alone, so the library needs neither: it needs three TABLES OF STRINGS and a
 * handful of flags.  Line i, with `column` the column separator:
 *     [id column] name column [truth column] [tophits column] [locations column] result '\n'
 *   id        (MC_FORMAT_QUERY_IDS) query_ids[i] if query_ids is given, else first_query_id + i (modulo 2^64), as a decimal number.
 *   name      names[name_off[i] .. name_off[i + 1]): the bytes as they are (the caller cuts the header at its first blank).
 *   truth     (MC_FORMAT_TRUTH) the MC_TEXT_RESULT entry of truth[i].
 *   tophits   (MC_FORMAT_TOPHITS) the read's candidates cands[i * stride ..) up to the first with hits == 0, joined by ','; each is
 *             text ':' hits with text = the MC_TEXT_CANDIDATE entry of its tgt.  A candidate whose text is empty -- or whose tgt lies
 *             beyond the table -- prints nothing, neither the ':' nor the hits, but its comma stays (show_candidates for a target
 *             without a taxon).
 *   locations (MC_FORMAT_LOCATIONS) per candidate of the same walk '[' win_stride * beg ',' win_stride * end + win_len "] ", in 64 bits.
 *   result    the MC_TEXT_RESULT entry of assigned[i].taxon (entry 0: the unclassified text).  Where the MC_TEXT_TARGET_RESULT table is
 *             set, an assignment with taxon != 0 and rank 0 (bits 0-7 of info: a sequence-level result) prints that table's entry of
 *             the read's FIRST candidate's tgt instead.
 *   A result index (taxon, truth, or that tgt) beyond its table prints entry 0 of MC_TEXT_RESULT and is counted once in
 *   mc_format_stats.  With MC_FORMAT_MAPPED_ONLY a read with assigned[i].taxon == 0 has no line at all (line_off[i + 1] == line_off[i]).
 * mc_format_set_text: `count` strings, string k = bytes[offsets[k] .. offsets[k + 1]), offsets[0] == 0 and not decreasing; copied.  The
 * table goes to the device with the first mc_format_mappings and again after a later set; no format call may be in flight while a
 * table is replaced.  Needs no device (an mc_open_metadata context takes the tables, and checks arguments).  MC_ERR_INVALID: NULL ctx
 * or offsets, an unknown table, MC_TEXT_RESULT with count == 0, offsets that do not begin at 0 or decrease.
 * mc_format_mappings: line i = out[line_off[i] .. line_off[i + 1]); line_off[n] = the bytes all lines need.  If that exceeds
 * out_capacity NO BYTE OF out IS WRITTEN and line_off is still complete, so that the caller can size a buffer and call again.
 *   Without MC_FORMAT_HOST all arrays are DEVICE pointers (out and cands 16-byte, assigned and the u64 arrays 8-byte, truth 4-byte
 *   aligned) and the call is asynchronous on 'stream' (a hipStream_t; NULL = the context's own): enqueued behind mc_query_device ->
 *   mc_classify_candidates it needs no synchronisation in between.  The overflow verdict is then line_off[n] > out_capacity, for the
 *   caller to read; the call returns MC_OK.  line_off has room for num_queries + 1 + MC_FORMAT_SCRATCH entries: the tail is the
 *   workspace of the scan, so the call keeps no per-call state in the context and calls on different streams may run at the same time.
 *   With MC_FORMAT_HOST the arrays are HOST arrays (line_off: num_queries + 1 entries), staged in pieces through buffers of the context
 *   as MC_CLASSIFY_HOST does (mc_set_tuning "format_stage_rows": reads per piece, 0 = default), one caller at a time; the call returns
 *   when out is filled, or MC_ERR_NOMEM (line_off complete, out untouched) when the lines do not fit.
 * MC_ERR_INVALID (checked first, before any device call): NULL ctx, options or line_off, NULL cands, assigned or name_off with
 * num_queries > 0, NULL out with out_capacity > 0, stride == 0, column_len > 16, unknown flags, MC_FORMAT_TRUTH without truth,
 * misaligned device arrays, out overlapping an input or line_off.  MC_ERR_STATE: no MC_TEXT_RESULT table, MC_FORMAT_TOPHITS without
 * the MC_TEXT_CANDIDATE table, a context without a device (mc_open_metadata).  num_queries == 0: MC_OK and line_off[0] = 0 (a DEVICE line_off
 * is written on the stream, so that form needs the device even then).
 * mc_format_stats: stats[0..4] = mc_format_mappings calls that had reads, reads handed over, lines written, bytes written, result indices beyond
 * their table -- the last three counted by the calls whose lines fitted.  Waits for the context's own streams. */
#define MC_TEXT_RESULT        0      /* indexed by mc_assignment.taxon (and truth); entry 0 = the unclassified text */
#define MC_TEXT_TARGET_RESULT 1      /* indexed by target, optional: the result text of sequence-level assignments */
#define MC_TEXT_CANDIDATE     2      /* indexed by target: the text in front of ":hits" */
int mc_format_set_text(mc_ctx* ctx, int which, const char* bytes, const uint64_t* offsets, uint64_t count);
typedef struct {
    char     column[16];             /* the column separator (-separator) ... */
    uint32_t column_len;             /* ... and its length, 0 .. 16 */
    uint32_t win_stride, win_len;    /* the database's window stride and window length: the locations column */
} mc_format_options;
#define MC_FORMAT_HOST        1      /* the arrays are HOST arrays, the call returns when out is filled */
#define MC_FORMAT_QUERY_IDS   2      /* -queryids */
#define MC_FORMAT_TRUTH       4      /* -ground-truth */
#define MC_FORMAT_TOPHITS     8      /* -tophits */
#define MC_FORMAT_LOCATIONS   16     /* -locations */
#define MC_FORMAT_MAPPED_ONLY 32     /* -mapped-only */
#define MC_FORMAT_SCRATCH     2048   /* entries of workspace behind a DEVICE line_off */
int mc_format_mappings(mc_ctx* ctx, const mc_format_options* opt, const mc_candidate* cands, uint32_t stride, const mc_assignment* assigned,
                       const uint32_t* truth, const uint64_t* query_ids, uint64_t first_query_id, const char* names, const uint64_t* name_off,
                       uint32_t num_queries, int flags, char* out, uint64_t out_capacity, uint64_t* line_off, void* stream);
int mc_format_stats(mc_ctx* ctx, uint64_t stats[5]);

/* ---- the all-hits column (-allhits): a read's whole location list, run-length encoded ----------------
 * show_matches (printing.cpp:315-365).  Read i's list is hits[hit_off[i] .. hit_off[i + 1]).  A RUN is a maximal stretch of consecutive
 * entries with equal tgt and equal win (nothing assumes a sorted list; the lists of mc_query_device(MC_WANT_ALLHITS) are).  Runs print in
 * list order with nothing between them, an empty list gives an empty piece; the trailing ',' stays.  With text = entry tgt of the table
 * of mc_format_matches_set_text, C = the run's length in decimal (as the reference's int for lengths below 2^31):
 *   MC_MATCHES_WINDOWS (-lowest sequence):  text '/' W ':' C ','   W = win as the signed 32-bit number int(win) (win >= 2^31 prints negative);
 *                                           a run whose entry is empty, or whose tgt lies beyond the table, prints NOTHING.
 *   otherwise (a lowest rank above it):     text ':' C ','         an empty entry still prints ":C,"; a tgt beyond the table prints nothing.
 *   A tgt beyond the table is counted once per run in mc_format_matches_stats, in both forms.
 * mc_format_matches_set_text: the table, indexed by target; the rules of mc_format_set_text (count == 0 is allowed, a string has less
 *   than 16 MiB; needs no device); copied, and sent to the device again after a later set -- no format call may be in flight meanwhile.
 * mc_format_matches: piece i = out[piece_off[i] .. piece_off[i + 1]); piece_off[n] = the bytes all pieces need.  If that exceeds
 *   out_capacity NO BYTE OF out IS WRITTEN and piece_off is still complete (the contract of mc_format_mappings).
 *   Without MC_FORMAT_HOST all arrays are DEVICE pointers (out 16-byte, hits, hit_off and piece_off 8-byte aligned) and the call is
 *   asynchronous on 'stream' (NULL = the context's own): behind mc_query_device(MC_WANT_ALLHITS) -- hits / hit_offsets of its
 *   mc_device_results -- it needs no synchronisation.  piece_off has room for num_queries + 1 + MC_FORMAT_SCRATCH entries (the scan's
 *   workspace: no per-call state in the context, calls on different streams may run at the same time); returns MC_OK, the overflow
 *   verdict is piece_off[n] > out_capacity.
 *   With MC_FORMAT_HOST the arrays are HOST arrays (piece_off: num_queries + 1 entries), staged through buffers of the context in pieces
 *   of whole reads with at most mc_set_tuning "format_stage_hits" locations (0 = default: 4 Mi) -- a read whose list alone is longer
 *   goes alone --, one caller at a time; returns when out is filled, or MC_ERR_NOMEM (piece_off complete, out untouched).
 *   MC_ERR_INVALID (checked first, before any device call): NULL ctx or piece_off, NULL hit_off with num_queries > 0, NULL out with
 *   out_capacity > 0, unknown flags, misaligned device arrays, a host hit_off that decreases, out overlapping an input or piece_off.
 *   MC_ERR_STATE: no table, a context without a device (mc_open_metadata).  num_queries == 0: MC_OK and piece_off[0] = 0 (a DEVICE
 *   piece_off is written on the stream, so that form needs the device even then).
 * mc_format_mappings_with: mc_format_mappings with ONE MORE COLUMN between the truth column and the tophits column (where the reference
 *   prints -allhits): the bytes extra[extra_off[i] .. extra_off[i + 1]) followed by the column separator.  With MC_FORMAT_MAPPED_ONLY a
 *   read without a line skips its piece.  extra == NULL: exactly mc_format_mappings.  extra / extra_off are device or host arrays as the
 *   others are (extra_off: num_queries + 1 entries, 8-byte aligned on the device, not decreasing); `extra` may be the `out` of
 *   mc_format_matches and extra_off its piece_off, enqueued on the same stream with no synchronisation in between.  The same flags,
 *   errors and statistics as mc_format_mappings; MC_ERR_INVALID also for extra without extra_off and for out overlapping either.
 * mc_format_matches_stats: stats[0..4] = mc_format_matches calls that had reads, reads handed over, runs printed, bytes written, runs whose
 *   tgt lay beyond the table -- the last three counted by the calls whose pieces fitted.  Waits for the context's own streams.
 * mc_timing_get names: "matches_lengths" (matches_kernel<false> + tile_scan_kernel), "matches_write" (matches_kernel<true>). */
#define MC_MATCHES_WINDOWS    2      /* the window form: text '/' window ':' length ',' */
int mc_format_matches_set_text(mc_ctx* ctx, const char* bytes, const uint64_t* offsets, uint64_t count);
int mc_format_matches(mc_ctx* ctx, const mc_location* hits, const uint64_t* hit_off, uint32_t num_queries, int flags, char* out, uint64_t out_capacity,
                      uint64_t* piece_off, void* stream);
int mc_format_mappings_with(mc_ctx* ctx, const mc_format_options* opt, const mc_candidate* cands, uint32_t stride, const mc_assignment* assigned,
                            const uint32_t* truth, const uint64_t* query_ids, uint64_t first_query_id, const char* names, const uint64_t* name_off,
                            uint32_t num_queries, int flags, char* out, uint64_t out_capacity, uint64_t* line_off, void* stream,
                            const char* extra, const uint64_t* extra_off);
int mc_format_matches_stats(mc_ctx* ctx, uint64_t stats[5]);

/* ---- reads out of a FASTA / FASTQ byte range: the input side of a query on the device ------
 * THE RECORD RULE (sequence_reader::read_next, sequence_io.cpp:160-236, for regular input).  The range is bytes[0, nbytes); bytes[0] is
 * '>' (FASTA) or '@' (FASTQ) and selects the kind; the range holds whole records, the last one ends at nbytes.  A line start is position
 * 0 or the byte after a '\n'; "trimmed" means without the trailing run of '\r' / '\n'.
 *   FASTA: a record starts at every line start that holds '>'; the header is the rest of that line, trimmed; the sequence is the record's
 *          other lines in order, each trimmed (empty lines add nothing).  A line start that holds '+' makes the range IRREGULAR.
 *   FASTQ: lines count from 0.  Line 4k starts with '@' and is the header (without the marker, trimmed); line 4k + 1 is the sequence,
 *          trimmed, and does not start with '+', '>', '\n' or '\r'; line 4k + 2 starts with '+'; line 4k + 3 is dropped.  Any violation,
 *          or a number of lines that is no multiple of 4, makes the range IRREGULAR.
 *   The name is the header up to its first ' '.  MC_PARSE_PAIRS: query q is records 2q and 2q + 1 under the first one's name; an odd
 *   count leaves a last query with len2 = 0 (status[7] = 1).
 *   The device refuses MORE than the rule does -- a '\r' that is not followed by '\n' or by the end of the range is IRREGULAR -- and never
 *   cuts an accepted range differently from the rule.  The offence (status[5]) is the offset of the first line start, or '\r', that broke
 *   the rule; nbytes for an incomplete last FASTQ group.
 * mc_parse_records fills, in file order: hdr[records][2] = offset and length of each header in bytes; qinfo[queries][4] as
 *   mc_device_batch takes it (offsets into seq; every sequence begins at a multiple of 4, the padding bytes and the 16 bytes behind the
 *   last sequence are 0; a query without a second mate has qinfo[2] = the end of the first, padded, and qinfo[3] = 0, as mc_batch_add
 *   leaves it); names + name_off[queries + 1] as mc_format_mappings takes them; max_win[queries] = 2 + max(len1 + len2,
 *   insert_size_max) / the database's window stride; status[8] = records, queries, bytes of seq needed (with the 16 behind), bytes of
 *   names needed, verdict, offence, the longest len1 + len2, half pair.  With a verdict other than MC_PARSE_OK NOTHING but status is
 *   written; with MC_PARSE_OVERFLOW (more than max_records records, or a capacity too small) status holds what a second call needs; with
 *   MC_PARSE_IRREGULAR only verdict and offence mean anything.  The arrays have room for max_records records (name_off: one more).
 *   Without MC_PARSE_HOST all arrays are DEVICE pointers (bytes, seq and workspace 16-byte, name_off and status 8-byte, the others 4-byte
 *   aligned) and the call is enqueued on `stream` (NULL: the context's) without any synchronisation: in front of mc_query_device, whose
 *   mc_device_batch it fills.  The caller owns the workspace (mc_parse_scratch_bytes(nbytes) bytes); the context keeps nothing per call,
 *   so calls on different streams may run at once.  The same bytes give the same outputs, byte for byte.  bytes[0] is part of the verdict.
 *   With MC_PARSE_HOST all arrays are HOST arrays (workspace may be NULL), staged through buffers of the context, one caller at a time;
 *   the call returns when they are filled.
 * MC_ERR_INVALID (checked first, before any device call): NULL ctx, out, bytes or status, nbytes == 0 or > 2^31, unknown flags, NULL
 *   arrays with max_records > 0, a capacity without its array or beyond 2^32 - 1, MC_PARSE_HOST: bytes[0] that is no marker; device form:
 *   a workspace that is too small, misaligned arrays.  MC_ERR_STATE: a context without a device (mc_open_metadata).
 * mc_parse_stats: stats[0..3] = calls, bytes handed over, records of the accepted ranges, ranges refused (irregular or overflow); waits
 *   for the device.  mc_timing_get names: "parse_classify" (the three tile passes and their scans), "parse_write". */
#define MC_PARSE_HOST       1
#define MC_PARSE_PAIRS      2
#define MC_PARSE_OK         0
#define MC_PARSE_IRREGULAR  1
#define MC_PARSE_OVERFLOW   2
typedef struct {
    uint32_t* hdr;            /* [max_records][2] */
    uint32_t* qinfo;          /* [max_records][4] */
    uint8_t*  seq;
    uint64_t  seq_capacity;
    char*     names;
    uint64_t  names_capacity;
    uint64_t* name_off;       /* [max_records + 1] */
    uint32_t* max_win;        /* [max_records] */
    uint64_t* status;         /* [8]; mc_parse_mates: [10] */
    uint32_t  max_records;
} mc_parse_output;
extern const uint32_t mc_parse_tile;   /* bytes one block classifies: what lies in front of a tile comes from a scan over the tiles (for tests and tools) */
uint64_t mc_parse_scratch_bytes(uint64_t nbytes);
int mc_parse_records(mc_ctx* ctx, const char* bytes, uint64_t nbytes, int flags, uint64_t insert_size_max, const mc_parse_output* out,
                     void* workspace, uint64_t workspace_bytes, void* stream);
int mc_parse_stats(mc_ctx* ctx, uint64_t stats[4]);

/* ---- mates in two ranges: the two files of `-pairfiles` ("mates") ------
 * THE MATES RULE (sequence_pair_reader::next for pairing_mode::files).  There are two ranges, B1[0, n1) and B2[0, n2).  Each is judged by
 * the record rule above on its own and selects its own kind by its first byte (FASTA beside FASTQ is allowed: the reference's two
 * readers are independent).  Query q is record q of B1 -- the first mate, and the query's name -- and record q of B2, the second mate.
 * For accepted ranges qinfo, seq, names, name_off and max_win are, field by field and byte by byte, what mc_parse_records(...,
 * MC_PARSE_PAIRS, ...) gives for a file in which the records of the two ranges alternate; hdr[2 * queries][2] holds in row 2q the header
 * of query q's first mate as offset and length IN B1, in row 2q + 1 that of its second mate IN B2.  The ranges hold the same number of
 * records, or the call refuses with MC_PARSE_UNEQUAL (the reference stops silently at the shorter file; this library never cuts an
 * accepted input differently from what it was handed).
 * status has 10 words: [0..6] as for mc_parse_records with [0] = the records of both ranges together, [1] = queries; [7] = the range
 *   (0 or 1) in which the offence [5] lies with MC_PARSE_IRREGULAR, else 0 -- when both ranges are irregular, range 0's offence is the
 *   one reported; [8], [9] = the records of B1 and of B2, meaningful with MC_PARSE_OK, MC_PARSE_OVERFLOW and MC_PARSE_UNEQUAL (so the
 *   caller can cut the longer range).  MC_PARSE_OVERFLOW is as for mc_parse_records, max_records counted over both ranges; [0], [2] and
 *   [3] then hold what a second call needs, and [6] is filled only where the records fit max_records (else 0).  With MC_PARSE_UNEQUAL
 *   only [0], [4], [8] and [9] mean anything.  With a verdict other than MC_PARSE_OK NOTHING but status is written.
 * mc_parse_mates: flags is 0 (DEVICE pointers; bytes1, bytes2, seq and workspace 16-byte aligned, the others as for mc_parse_records;
 *   enqueued on `stream` without any synchronisation; the caller owns the workspace of mc_parse_mates_scratch_bytes(n1, n2,
 *   out->max_records) bytes and the context keeps nothing per call, so calls on different streams may run at once; the same bytes give
 *   the same outputs) or MC_PARSE_HOST (HOST arrays, staged through the context as mc_parse_records does).  MC_ERR_INVALID (checked
 *   first, before any device call) as for mc_parse_records for either range, and: MC_PARSE_PAIRS or another flag, n1 + n2 > 2^31.
 *   mc_parse_stats counts these calls too (bytes: n1 + n2). */
#define MC_PARSE_UNEQUAL    3
uint64_t mc_parse_mates_scratch_bytes(uint64_t n1, uint64_t n2, uint32_t max_records);
int mc_parse_mates(mc_ctx* ctx, const char* bytes1, uint64_t n1, const char* bytes2, uint64_t n2, int flags, uint64_t insert_size_max,
                   const mc_parse_output* out, void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- batch borders of a FASTA / FASTQ range: what the host index did ------
 * THE CUT RULE.  The range is B[0, n), n = nbytes, R = records_per_batch; B[0] selects the kind.  Line starts, record starts (FASTA: a
 * line start that holds '>'; FASTQ: the start of every line 4k) and offences are those of THE RECORD RULE above.  What this call adds is
 * where the range is taken to END:
 *   closed (no MC_CUT_OPEN): consumed = n, whole = the number of record starts; verdict and offence are exactly those of
 *          mc_parse_records for B[0, n) -- a first byte that is no marker (offence 0) and an incomplete last FASTQ group (offence n) included.
 *   open (MC_CUT_OPEN): the last record may be cut short, and the next call starts at consumed.
 *          FASTA: whole = the record starts - 1, consumed = the line start of the last record (one record: whole = 0, consumed = 0).
 *          FASTQ: a group is whole when all four of its lines end in a '\n' inside the range: whole = (number of '\n') / 4, consumed = the
 *          byte behind the (4 * whole)-th '\n'.
 *          MC_PARSE_PAIRS: whole is rounded down to an even number and consumed moves back with it.
 *          The verdict covers B[0, consumed) only -- an offence at or behind consumed is none, the next call judges it -- and for
 *          consumed > 0 verdict and offence are those of mc_parse_records for B[0, consumed).  consumed = 0 is MC_PARSE_OK with no batch,
 *          unless B[0] is no marker.
 *   batches: nb = ceil(whole / R); cuts[i] = the line start of record i * R for i < nb, cuts[nb] = consumed.  Every B[cuts[i], cuts[i + 1])
 *          is a range of whole records that mc_parse_records accepts: R records, the last batch the rest.  MC_PARSE_PAIRS wants an even R.
 * status[8] = whole, nb, consumed, the record starts seen in the range, verdict, offence, the largest cuts[i + 1] - cuts[i] (what a slot
 *   must hold; filled with MC_PARSE_OK only, else 0), 1 when the last batch ends in a half pair (closed, pairs, odd whole).
 *   MC_PARSE_OVERFLOW: nb + 1 > capacity (the entries of cuts); status holds what a second call needs.  With a verdict other than
 *   MC_PARSE_OK NOTHING but status is written; with MC_PARSE_IRREGULAR only verdict and offence mean anything.
 * mc_parse_cut: as mc_parse_records -- without MC_PARSE_HOST bytes, cuts, status and workspace are DEVICE pointers (cuts and status
 *   8-byte, workspace 16-byte aligned) and the call is enqueued on `stream` (NULL: the context's) without any synchronisation; the caller
 *   owns the workspace (mc_parse_cut_scratch_bytes(nbytes) bytes), the context keeps nothing per call, the same bytes give the same
 *   outputs.  Unlike mc_parse_records it accepts bytes at ANY address: a piece starts where the last one ended.  With MC_PARSE_HOST all
 *   arrays are HOST arrays (workspace may be NULL), staged through the context, one caller at a time.
 * MC_ERR_INVALID (checked first, before any device call): NULL ctx, bytes, cuts or status, nbytes == 0 or > 2^31, records_per_batch == 0
 *   (or odd with MC_PARSE_PAIRS), unknown flags; device form: a workspace that is too small, misaligned cuts, status or workspace.
 *   MC_ERR_STATE: a context without a device.  mc_parse_stats does not count these calls.  mc_timing_get name: "parse_cut".
 * mc_parse_headers packs the headers of a range that mc_parse_records has cut: hdr and parse_status are what that call left for bytes
 *   (device arrays, or host arrays with MC_PARSE_HOST).  The record count is read ON THE DEVICE from parse_status[0], so the call sits
 *   behind the parse on one stream without any synchronisation.  out_off[r] = the sum of the header lengths in front of record r
 *   (out_off[records] = all of them), out = the trimmed headers back to back.  status[4] = records, bytes of out needed, verdict, 0; the
 *   verdict is MC_PARSE_OK, MC_PARSE_OVERFLOW (out_capacity too small; or more records than max_records, then the bytes needed are not
 *   known and [1] = 0), or the parse's own verdict passed through ([0] = [1] = 0).  With a verdict other than MC_PARSE_OK NOTHING but
 *   status is written.  Device form: hdr 4-byte, parse_status, out_off and status 8-byte, workspace 16-byte aligned
 *   (mc_parse_headers_scratch_bytes(max_records) bytes); bytes and out at any address.  MC_ERR_INVALID as above; flags other than
 *   MC_PARSE_HOST.  mc_timing_get name: "parse_headers". */
#define MC_CUT_OPEN         4      /* beside MC_PARSE_HOST (1) and MC_PARSE_PAIRS (2) */
uint64_t mc_parse_cut_scratch_bytes(uint64_t nbytes);
int mc_parse_cut(mc_ctx* ctx, const char* bytes, uint64_t nbytes, uint32_t records_per_batch, int flags,
                 uint64_t* cuts, uint64_t capacity, uint64_t status[8],
                 void* workspace, uint64_t workspace_bytes, void* stream);
uint64_t mc_parse_headers_scratch_bytes(uint32_t max_records);
int mc_parse_headers(mc_ctx* ctx, const char* bytes, uint64_t nbytes, const uint32_t* hdr, const uint64_t* parse_status,
                     uint32_t max_records, int flags, char* out, uint64_t out_capacity, uint64_t* out_off /* [max_records + 1] */,
                     uint64_t status[4], void* workspace, uint64_t workspace_bytes, void* stream);

/* ---- targets out of MANY FASTA files in one byte range: the input side of a build on the device ------
 * THE TARGET RULE.  The range is bytes[0, nbytes).  File f is bytes[file_off[f], file_off[f + 1]); file_off[0] = 0, the table ascends
 * strictly and file_off[num_files] = nbytes.  Each file is judged by the FASTA part of THE RECORD RULE above ON ITS OWN:
 *   a line start is the file's first byte, or the byte after a '\n' of the same file (a file need not end in '\n');
 *   a file's first byte that is not '>' is IRREGULAR, the offence is that byte (FASTQ is not taken);
 *   a line start that holds '+' is IRREGULAR; a '\r' that is not followed by '\n' or by the file's end is IRREGULAR.
 *   A record starts at every line start that holds '>'; header and sequence are those of the record rule (the header ends with its line
 *   or with the file).  So the files, each with a '\n' put behind it where it lacks one, give exactly the records of mc_parse_records.
 *   The lowest offence of the range is reported and status[7] names its file.  A file table that breaks its own rule is found on the
 *   device (one thread per row): MC_PARSE_IRREGULAR with offence nbytes and status[7] = the first bad row (row r > 0 is bad when it is
 *   not above row r - 1, row 0 when it is not 0, row num_files also when it is not nbytes).  MC_PARSE_HOST refuses such a table with
 *   MC_ERR_INVALID before any device call.
 * mc_parse_targets fills, in range order and for ALL records, empty ones included: hdr[records][2] as mc_parse_records lays it out
 *   (offset of the header in the range, without the marker; its trimmed length); targets[r] = seq_off (an offset into seq, a multiple
 *   of 4), len (sequence bytes: all lines but the header, trimmed, empty lines add nothing), file, index (the record's number inside its
 *   file, from 0, empty records counted), reserved = 0; seq = the sequences back to back, each at a multiple of 4, the padding bytes and
 *   the 16 bytes behind the last sequence 0, a record with len == 0 takes no room (seq_off is then where the next sequence begins) --
 *   what mc_build_add_target_device asks of its source.  status[8] = records, records with len > 0, bytes of seq needed (with the 16
 *   behind), 0, verdict, offence, the longest len, the file of the offence.  status[0] and status[4] are the words mc_parse_headers
 *   reads of a parse's status (the record count and the verdict; of hdr it reads rows [0, records)), so it packs the headers of a range
 *   parsed here unchanged.  With MC_PARSE_OVERFLOW (more than max_records records, or seq_capacity too small) status[0..2] and [6] hold
 *   what a second call needs; with MC_PARSE_IRREGULAR only [4], [5] and [7] mean anything (the others are 0).  With a verdict other than
 *   MC_PARSE_OK NOTHING but status is written.
 *   Without MC_PARSE_HOST all arrays, file_off included, are DEVICE pointers (bytes, seq and workspace 16-byte, targets, status and
 *   file_off 8-byte, hdr 4-byte aligned) and the call is enqueued on `stream` (NULL: the context's) without any synchronisation.  The
 *   caller owns the workspace (mc_parse_targets_scratch_bytes(nbytes, num_files, max_records) bytes); the context keeps nothing per call,
 *   so calls on different streams may run at once.  The same bytes give the same outputs, byte for byte.
 *   With MC_PARSE_HOST all arrays are HOST arrays (workspace may be NULL), staged through buffers of the context, one caller at a time;
 *   the call returns when they are filled.
 * MC_ERR_INVALID (checked first, before any device call): NULL ctx, out, bytes, file_off or status, nbytes == 0 or > 2^31, num_files == 0,
 *   flags other than MC_PARSE_HOST, NULL arrays with max_records > 0, a capacity without its array; device form: a workspace that is too
 *   small, misaligned arrays.  MC_ERR_STATE: a context without a device (mc_open_metadata).  mc_parse_stats counts these calls.
 *   mc_timing_get names: "targets_classify" (the table pass, three byte passes, the record sums and the scans), "targets_write". */
typedef struct { uint64_t seq_off; uint32_t len, file, index, reserved; } mc_parse_target;   /* 24 bytes */
typedef struct {
    uint32_t*        hdr;          /* [max_records][2]: offset and length of each header, as mc_parse_records leaves them */
    mc_parse_target* targets;      /* [max_records] */
    uint8_t*         seq;
    uint64_t         seq_capacity;
    uint64_t*        status;       /* [8] */
    uint32_t         max_records;
} mc_parse_targets_output;
uint64_t mc_parse_targets_scratch_bytes(uint64_t nbytes, uint32_t num_files, uint32_t max_records);
int mc_parse_targets(mc_ctx* ctx, const char* bytes, uint64_t nbytes, const uint64_t* file_off /* [num_files + 1] */, uint32_t num_files,
                     int flags, const mc_parse_targets_output* out, void* workspace, uint64_t workspace_bytes, void* stream);

/* raw bytes into a batch slot: the slot's reads are cut on the device
 * mc_batch_add_file_bytes fills an EMPTY slot with a byte range of a FASTA / FASTQ file (whole records; flags: 0 or MC_PARSE_PAIRS): one
 *   copy into the slot's pinned input.  MC_BATCH_FULL, and nothing added, when nbytes exceeds the slot's character capacity; MC_ERR_STATE
 *   when the slot holds reads already or is in flight; mc_batch_add on a slot that holds a raw range is MC_ERR_STATE as well.
 *   mc_batch_submit uploads the bytes, has mc_parse_records cut them into the slot's device input and runs the unchanged query on that;
 *   it waits once for the device, for the number of reads.  A raw slot is never united with other slots: where the context unites its
 *   slots (small slots, no all-hits lists) it goes alone and mc_batch_submit returns when it is through.  mc_batch_wait and
 *   mc_batch_clear work as before.
 * mc_batch_records, after mc_batch_wait: the verdict of mc_parse_records and its offence, the numbers of records and queries, the half
 *   pair, and host views of hdr [records][2] and qinfo [queries][4] (valid until mc_batch_clear; NULL with another verdict than
 *   MC_PARSE_OK).  With such a verdict mc_results.num_queries is 0 and the caller takes the batch the old way: MC_PARSE_IRREGULAR, or
 *   MC_PARSE_OVERFLOW for more queries than slot_max_queries, more characters than the slot's capacity, or a read (pair) of len + 8 >
 *   slot_max_chars.  MC_ERR_STATE: a slot without a submitted raw range. */
typedef struct {
    uint32_t        verdict;
    uint32_t        records, queries, half_pair;
    uint64_t        offence;
    const uint32_t* hdr;
    const uint32_t* qinfo;
} mc_batch_record_info;
int mc_batch_add_file_bytes(mc_ctx* ctx, uint32_t slot, const char* bytes, uint64_t nbytes, int flags, uint64_t insert_size_max);
int mc_batch_records(mc_ctx* ctx, uint32_t slot, mc_batch_record_info* out);
/* mc_batch_add_file_mates fills an EMPTY slot with the two ranges of the mates rule: MC_BATCH_FULL, and nothing added, when n1 + n2
 *   exceeds the slot's character capacity; otherwise as mc_batch_add_file_bytes.  mc_batch_submit uploads both ranges and runs
 *   mc_parse_mates, then the unchanged query; it waits once for the device between the two, for the number of reads.  mc_batch_records
 *   works unchanged: records = 2 * queries, half_pair = 0, hdr as mc_parse_mates leaves it (row 2q in bytes1, row 2q + 1 in bytes2);
 *   a verdict other than MC_PARSE_OK (MC_PARSE_UNEQUAL among them) leaves mc_results.num_queries at 0. */
int mc_batch_add_file_mates(mc_ctx* ctx, uint32_t slot, const char* bytes1, uint64_t n1, const char* bytes2, uint64_t n2, uint64_t insert_size_max);
/* mc_batch_add_device_bytes is mc_batch_add_file_bytes for a range that lies in DEVICE memory already (a batch of mc_parse_cut, DESIGN.md
 *   7l): any alignment; the memory stays untouched until mc_batch_wait returns; the same MC_BATCH_FULL / MC_ERR_STATE answers; never
 *   united with other slots.  mc_batch_submit copies the range once on the device instead of uploading it, and has mc_parse_headers pack
 *   the headers behind the parse; they travel back with the results.  mc_batch_records works unchanged.
 * mc_batch_headers, after mc_batch_wait: host views of the headers back to back and of off[records + 1] (header r is bytes[off[r],
 *   off[r + 1])), valid until mc_batch_clear; NULL views and 0 records with a verdict other than MC_PARSE_OK.  MC_ERR_STATE: a slot that
 *   was not filled by mc_batch_add_device_bytes and submitted. */
int mc_batch_add_device_bytes(mc_ctx* ctx, uint32_t slot, const void* dbytes, uint64_t nbytes, int flags, uint64_t insert_size_max);
int mc_batch_headers(mc_ctx* ctx, uint32_t slot, const char** bytes, const uint64_t** off, uint64_t* records);

/* ---- a query file resident on the device: for callers that own no device memory (`mcq query`, MCQ_INPUT_DEVICE) ------
 * mc_input_open takes a file's bytes as they lie on the HOST (its mapping) and makes them resident: a plain file is uploaded; a file that
 *   begins with the gzip magic goes through mc_bgzf_index and the DEVICE form of mc_inflate_blocks into a buffer sized from the index, so
 *   the plain bytes never exist on the host.  The resident bytes are then cut with mc_parse_cut in pieces of at most piece_bytes (<= 2^31):
 *   every piece but the last with MC_CUT_OPEN, the next one starting at `consumed`; an open piece with consumed = 0 is doubled up to 2^31.
 *   A batch of records_per_batch records (flags: 0 or MC_PARSE_PAIRS, then an even number) whose bytes exceed slot_bytes is cut again with
 *   half the records (kept even for pairs), down to one query; one query that still does not fit is kept with too_big = 1.  The call waits
 *   for the device; it uses the context's own stream.
 *   info[8] = verdict, detail, plain bytes, pieces, batches, records, 1 where the bytes were inflated on the device, second detail.
 *   MC_INPUT_OK: *out is the handle.  MC_INPUT_NOT_BGZF (gzip that is no BGZF; detail: the offending member's offset), MC_INPUT_REFUSED
 *   (a member the device refused; detail: the row, second detail: its MC_INFLATE_R_* reason), MC_INPUT_TOO_LARGE (plain bytes >
 *   max_resident_bytes), MC_INPUT_NO_MEMORY, MC_INPUT_EMPTY: nothing is resident, *out is NULL.  MC_INPUT_IRREGULAR (detail: the offence,
 *   an offset into the plain bytes) and MC_INPUT_RECORD_TOO_LARGE (a record that does not fit the largest piece): no batches; *out is
 *   NULL for a plain file and a handle WITHOUT batches for an inflated one, so that mc_input_download can copy the plain bytes back once.
 *   MC_ERR_INVALID: NULL arguments, nbytes == 0, unknown flags, records_per_batch == 0 or odd with pairs, piece_bytes == 0 or > 2^31,
 *   slot_bytes == 0.  MC_ERR_STATE: a context without a device.
 * mc_input_batches: the batches in file order ({offset into the plain bytes, bytes, records, queries, half_pair: the file's last query has
 *   no second mate, too_big}; the first `capacity` of them), the device address of the plain bytes -- batch i goes to a slot as
 *   mc_batch_add_device_bytes(ctx, slot, device_bytes + offset, nbytes, flags, ...) -- and their number.  mc_input_download copies the plain
 *   bytes to the host.  mc_input_close frees the handle and its device memory; no batch of it may be in flight. */
typedef struct mc_input mc_input;
typedef struct { uint64_t offset, nbytes; uint32_t records, queries, half_pair, too_big; } mc_input_batch;
#define MC_INPUT_OK                0
#define MC_INPUT_NOT_BGZF          1
#define MC_INPUT_REFUSED           2
#define MC_INPUT_TOO_LARGE         3
#define MC_INPUT_NO_MEMORY         4
#define MC_INPUT_EMPTY             5
#define MC_INPUT_IRREGULAR         6
#define MC_INPUT_RECORD_TOO_LARGE  7
int mc_input_open(mc_ctx* ctx, const void* file_bytes, uint64_t nbytes, int flags, uint32_t records_per_batch, uint64_t piece_bytes, uint64_t slot_bytes,
                  uint64_t max_resident_bytes, mc_input** out, uint64_t info[8]);
int mc_input_batches(const mc_input* in, mc_input_batch* batches, uint64_t capacity, const void** device_bytes, uint64_t* nbytes);
int mc_input_download(const mc_input* in, void* host_bytes, uint64_t capacity);
void mc_input_close(mc_input* in);

/* ---- BGZF input inflated on the device ---------------------------------------------
 * BGZF (what bgzip and htslib write) is a sequence of independent gzip members of at most 64 KiB in and out.  gzread joins the members
 * of such a file, so the specification of everything below is "the bytes zlib gives".
 * A BGZF MEMBER at offset p of bytes[0, nbytes):
 *   bytes[p .. p + 3] = 1f 8b 08 04 (deflate, FEXTRA and no other flag); MTIME, XFL and OS are anything; XLEN is the u16 at p + 10 (all
 *   numbers little endian); the extra field is XLEN bytes of subfields {SI1, SI2, SLEN u16, SLEN bytes} that tile it exactly; exactly
 *   one subfield has SI1 = 'B', SI2 = 'C', SLEN = 2: its u16 is BSIZE and the member is BSIZE + 1 bytes; the payload is
 *   bytes[p + 12 + XLEN, p + BSIZE + 1 - 8); the trailer is CRC32 u32 and ISIZE u32 with ISIZE <= 65536; the member is at least
 *   12 + XLEN + 8 bytes and ends at or before nbytes.
 * A RANGE IS BGZF when members chain from offset 0 to exactly nbytes (an empty range is not).  Every other range is MC_BGZF_FOREIGN --
 *   plain gzip, another FLG, a missing or doubled BC subfield, trailing bytes, a member cut short -- and the offence is the offset of
 *   the member that broke the rule.  This refuses more than zlib does (zlib takes FNAME and ignores trailing garbage); it never accepts
 *   a range and reads it differently.  The 28-byte end-of-file block (ISIZE 0) is an ordinary member.
 * A BLOCK INFLATES CORRECTLY when its payload is a deflate stream (RFC 1951: stored, fixed and dynamic blocks, any number of them) that,
 *   after its final block and the bits up to the next byte, ends exactly at the trailer; that produces exactly ISIZE bytes; in which no
 *   match reaches in front of the block's own first output byte (a BGZF block has no history); and whose bytes have the trailer's
 *   CRC-32.  Anything else is MC_INFLATE_CORRUPT.  Code sets are accepted as zlib accepts them: over-subscribed sets never, incomplete
 *   sets only as a single 1-bit literal/length or distance code or no distance code at all, a dynamic block only with a code for 256.
 *   Nothing that zlib's raw inflate refuses is accepted, and no other bytes are ever produced.
 * mc_bgzf_index: HOST only -- no context, no device, no zlib.  info = members, out bytes (the sum of ISIZE), verdict, offence.  Row i is
 *   member i: bytes[in_off, + in_len) -> out[out_off, + out_len), out_off the sum of the ISIZE in front.  With capacity too small (or
 *   blocks == NULL) info is still complete and the first `capacity` rows are filled: size, then call again.  With MC_BGZF_FOREIGN
 *   members and out bytes count the members in front of the offence.  MC_ERR_INVALID: info == NULL, bytes == NULL with nbytes > 0.
 * mc_inflate_blocks inflates the members the rows name.  status = verdict, the lowest bad row, its reason (MC_INFLATE_R_*, 0 with
 *   MC_INFLATE_OVERFLOW), the bytes of out the call covers (the largest out_off + out_len).  The lowest bad row decides the verdict:
 *   MC_INFLATE_OVERFLOW where its out_off + out_len > out_capacity (such a row writes nothing), else MC_INFLATE_CORRUPT.  It is a
 *   minimum over the rows, so the order in which the device takes them does not matter; the same input gives the same out and status.
 *   With a verdict other than MC_INFLATE_OK out[0, out_capacity) is unspecified; nothing outside it is touched.  Each row stores only
 *   inside its own [out_off, out_off + out_len) and uses only bytes of its own member; out_len bounds its stores, and a trailer whose
 *   ISIZE differs from out_len is MC_INFLATE_R_SHORT or MC_INFLATE_R_OVER.
 *   Without MC_INFLATE_HOST bytes, blocks, out and status are DEVICE pointers (bytes and out 16-byte, blocks and status 8-byte aligned;
 *   bytes readable up to nbytes rounded up to 16); the call is enqueued on `stream` (NULL: the context's own) with no synchronisation
 *   and no per-call state in the context, so calls on different streams may run at once, and mc_parse_records can take out behind it
 *   on the same stream.
 *   With MC_INFLATE_HOST they are HOST arrays, staged through buffers of the context in pieces of whole members (mc_set_tuning
 *   "inflate_stage_bytes": compressed bytes per piece, 0 = 64 MiB), one caller at a time; the call returns when out is filled or the
 *   verdict is known.  The rows are checked on the host first: in_off and out_off non-decreasing and the slices non-overlapping, inside
 *   nbytes, out_len <= 65536 -- else MC_ERR_INVALID.
 *   MC_ERR_INVALID (checked first, before any device call): NULL ctx or status; NULL bytes or blocks with num_blocks > 0; NULL out with
 *   out_capacity > 0; unknown flags; misaligned device arrays; out overlapping bytes.  MC_ERR_STATE: a context without a device
 *   (mc_open_metadata).  num_blocks == 0: MC_OK and an OK status.
 * mc_inflate_stats: calls, bytes in (nbytes), bytes out of the accepted calls, calls refused; waits for the device.  mc_timing_get name:
 *   "inflate_blocks" (the three launches of one enqueue; the host form enqueues once per staged piece). */
typedef struct { uint64_t in_off, out_off; uint32_t in_len, out_len; } mc_bgzf_block;
#define MC_BGZF_OK       0
#define MC_BGZF_FOREIGN  1
int mc_bgzf_index(const uint8_t* bytes, uint64_t nbytes, mc_bgzf_block* blocks, uint64_t capacity, uint64_t info[4]);

#define MC_INFLATE_HOST      1
#define MC_INFLATE_OK        0
#define MC_INFLATE_CORRUPT   1
#define MC_INFLATE_OVERFLOW  2
#define MC_INFLATE_R_BTYPE     1   /* block type 3 */
#define MC_INFLATE_R_STORED    2   /* LEN and NLEN of a stored block disagree */
#define MC_INFLATE_R_LENGTHS   3   /* a dynamic block's code lengths: counts beyond 286 / 30, a bad code-length code, a repeat without a
                                      predecessor or past HLIT + HDIST, no code for 256, an over-subscribed or incomplete set */
#define MC_INFLATE_R_SYMBOL    4   /* a literal/length code that is no symbol, or symbol 286 / 287 */
#define MC_INFLATE_R_DISTANCE  5   /* a distance code that is no symbol, code 30 / 31, or a distance beyond the block's output so far */
#define MC_INFLATE_R_INPUT     6   /* the stream needs bits beyond its payload (or the row's member does not hold a payload) */
#define MC_INFLATE_R_OVER      7   /* more than out_len / ISIZE bytes */
#define MC_INFLATE_R_SHORT     8   /* fewer than ISIZE bytes */
#define MC_INFLATE_R_LEFT      9   /* whole bytes left between the end of the stream and the trailer */
#define MC_INFLATE_R_CRC      10
int mc_inflate_blocks(mc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, const mc_bgzf_block* blocks, uint64_t num_blocks, int flags,
                      uint8_t* out, uint64_t out_capacity, uint64_t status[4], void* stream);
int mc_inflate_stats(mc_ctx* ctx, uint64_t stats[4]);

/* ---- whole gzip files inflated on the device ------------------------------------------
 * Reference genomes are ordinary gzip files: one long member each, no BSIZE, no 64 KiB bound.  One such stream is a chain and gains
 * nothing from a GPU; a build reads thousands of them, and there the FILE is the unit of parallelism as the member is above.
 * THE STREAM RULE.  A ROW is one file's bytes[in_off, in_off + in_len) and a slice out[out_off, out_off + out_cap).  The row's bytes are
 *   a CHAIN of one or more gzip members from in_off to exactly in_off + in_len.
 * A MEMBER: 1f 8b 08 FLG, MTIME (4), XFL, OS; then, as FLG says and in this order, FEXTRA (bit 2: a u16 length and its bytes), FNAME
 *   (bit 3: bytes up to and with a zero), FCOMMENT (bit 4: the same).  FTEXT (bit 0) is ignored.  FHCRC (bit 1) or a reserved bit (5, 6, 7)
 *   is refused -- more than zlib refuses; as above, never an accepted range read differently.  Behind the header a raw deflate stream
 *   whose length nothing states: the stream says where it ends, and what bounds its input is the row's end minus the 8 trailer bytes.
 *   Behind the byte-aligned end of the stream the trailer: CRC-32, then ISIZE.  The member is correct when its output has that CRC-32,
 *   its length mod 2^32 is ISIZE, and no match reaches in front of THIS member's first output byte: a second member starts with an
 *   empty history, as zlib's reset between members gives it.  Deflate blocks and code sets are accepted exactly as by the block rule.
 * Behind a trailer the row ends or the next member begins; bytes there that do not start with 1f 8b are MC_INFLATE_R_TRAILING (gzread
 *   would ignore them; the caller's host path reads such a file as it always did).  A row is ACCEPTED when its chain ends exactly at the
 *   row's end and the total output fits out_cap; `produced` is that total and may be less than out_cap.  A refused row reports
 *   produced 0, the members it finished and the reason.
 * LIMITS of a row: 18 <= in_len <= 2^28 and out_cap <= 2^31.  The decoder counts a member's unread input in bits and its output in
 *   bytes, both in 32-bit registers; these limits keep the counters valid.  The host form checks them before any device call
 *   (MC_ERR_INVALID), the kernel refuses such a row with MC_INFLATE_R_INPUT.
 * REASONS: the MC_INFLATE_R_* above with their numbers (MC_INFLATE_R_LEFT has no meaning here), and MC_INFLATE_R_HEADER (bad magic in the
 *   first member, CM != 8, FHCRC or a reserved flag, a header field that runs past the row), MC_INFLATE_R_TRAILING.  MC_INFLATE_R_INPUT
 *   also covers a stream or a trailer that runs past the row, MC_INFLATE_R_OVER more than out_cap and a slice outside out_capacity,
 *   MC_INFLATE_R_SHORT / _OVER an ISIZE that differs from the member's own count.
 * mc_gzip_hint: HOST only -- no context, no device, no zlib; every access checked against nbytes.  info = verdict (MC_GZIP_OK: the first
 *   member's header is one the device takes, and a trailer fits behind it), the offset of the first member's deflate stream, the
 *   trailing ISIZE (the last four bytes; 0 below 4 bytes), the offence (the MC_INFLATE_R_* reason, 0 with MC_GZIP_OK).  The trailing
 *   ISIZE is the size of a single-member file below 4 GiB.  For a chain it is too small: a row sized by it ends in MC_INFLATE_R_OVER and
 *   the caller falls back.  MC_ERR_INVALID: info == NULL, bytes == NULL with nbytes > 0.
 * mc_inflate_streams inflates the rows.  It follows mc_inflate_blocks in form -- flags, pointers, alignment (rows, results and status
 *   8-byte), stream, staging ("inflate_stage_bytes", the same buffers and mutex), the argument checks and their order -- and differs
 *   where it says so here:
 *   A ROW'S VERDICT IS ITS OWN.  results[i] is written for every row.  An accepted row's out[out_off, out_off + produced) holds zlib's
 *   bytes whatever the other rows are.  A refused row may write anywhere inside its OWN slice and nowhere else; a row whose slice does
 *   not lie inside out_capacity writes nothing.  The host form checks that the slices are pairwise disjoint (MC_ERR_INVALID); in the
 *   device form disjoint slices are the CALLER'S CONTRACT -- the kernel cannot see the other rows.
 *   status = verdict, the lowest refused row, its reason, the number of accepted rows.  MC_INFLATE_OK only if every row is accepted;
 *   else the lowest refused row decides: MC_INFLATE_OVERFLOW where its reason is MC_INFLATE_R_OVER (a matter of room), else
 *   MC_INFLATE_CORRUPT.  The lowest row is an atomic minimum: the same input gives the same status.  No synchronisation between the
 *   launches, no host step before the verdict.  num_rows <= 2^30.
 * mc_inflate_streams_stats: calls, bytes in (nbytes), bytes out of the accepted rows, rows refused; waits for the device.  mc_inflate_stats
 *   does not count these calls.  mc_timing_get name: "inflate_streams". */
typedef struct { uint64_t in_off, in_len, out_off, out_cap; } mc_gzip_stream;
typedef struct { uint64_t produced; uint32_t members, reason; } mc_gzip_result;   /* reason 0 = accepted */
#define MC_GZIP_OK       0
#define MC_GZIP_FOREIGN  1
#define MC_INFLATE_R_HEADER   11
#define MC_INFLATE_R_TRAILING 12
int mc_gzip_hint(const uint8_t* bytes, uint64_t nbytes, uint64_t info[4]);
int mc_inflate_streams(mc_ctx* ctx, const uint8_t* bytes, uint64_t nbytes, const mc_gzip_stream* rows, uint64_t num_rows, int flags,
                       uint8_t* out, uint64_t out_capacity, mc_gzip_result* results, uint64_t status[4], void* stream);
int mc_inflate_streams_stats(mc_ctx* ctx, uint64_t stats[4]);

/* ---- per-part result files merged on the device: what `metacache merge` reads ------
 * The result files of queries against single database parts (docs/partitioning.md of the reference) are cut into one candidate list
 * per query, and the vote runs over those lists.  (mc_merge_part_candidates above is something else: it merges candidate ARRAYS.)
 * Terms: a RESULT LINE is a line that does not start with '#'; lines that start with '#' are comment lines.  A TAXON ENTRY x is taxon
 * index + 1: row x - 1 of the taxon table (mc_set_taxon_table), 0 = none.  The LIST of query q is max_candidates pairs {taxon entry,
 * hits}, hits descending, ending at the first pair with hits == 0.
 * THE LINE RULE (read_results, mode_merge.cpp:158-238) -- narrower than what the reference's stream code tolerates: the device refuses
 * more and never reads an accepted range differently.  A range is bytes[0, n), n <= 2^31; it begins at a line start and its last line
 * may lack the '\n'.  A regular result line is, in order:
 *   1. one or more decimal digits at the line's first byte, value id <= 2^32 - 1; the query is q = id > 0 ? id - 1 : 0;
 *   2. any bytes up to the first '|';
 *   3. blanks (' ' or '\t'), then the header token: a non-empty run of non-blank bytes that holds no '|';
 *   4. from there tophits_column - 1 further '|', then the next '\t';
 *   5. the list: empty when the next byte is '\t' or the line ends; else entry (',' entry)* followed by '\t' or the end of the line,
 *      entry = an optional '-', 1-18 digits (the taxid), ':', 1-10 digits (hits, 1 .. 2^32 - 1).
 *   An empty line, a '\r', '\v', '\f' or NUL byte anywhere in a result line, or any other deviation makes the range IRREGULAR; the offence is the
 *   smallest line start of an offending line.  A second result line for the same q inside one file is an offending line too (found
 *   for q below the store's capacity: beyond it the verdict is MC_MERGE_OVERFLOW first).
 * TAXIDS: a taxid becomes a taxon entry through mc_merge_results_set_taxids; an entry whose taxid is not in the table is skipped and
 *   counted (the reference's "Skipping hit").
 * THE FILE RULE (the reference's resize, mode_merge.cpp:171-186): at the start of each file the number of lists is set to that file's
 *   number of result lines, which empties the lists and header places of higher queries collected from earlier files; a line whose
 *   q + 1 exceeds it grows it again.  Files are folded in the order of the calls, the entries of a line in their order.
 * THE INSERT RULE is insert_taxon_candidate (candidate_generation.hpp:172-231) with max_candidates and merge_below: a full list whose
 *   last entry has at least as many hits refuses the entry; with merge_below != 0 an entry whose taxon is in the list replaces that
 *   one only with strictly more hits and moves up past entries with strictly fewer; otherwise it goes behind every entry with as
 *   many hits (ties keep the earlier one in front) and the entry pushed out at the end is dropped.
 * THE HEADER RULE: a query keeps the header token of the first line folded for it while it had none, as a place {call, offset,
 *   length}: call = the number of the mc_merge_results_add call since mc_merge_results_begin (from 0, refused calls counted), offset
 *   into that call's range.  length 0: no header.
 * THE VOTE RULE is that of mc_classify_candidates for candidates that carry a taxon (classification.cpp:146-189): the lineage of a
 *   candidate is its taxon's row of the taxon table, the walk starts at the top candidate's own taxon and at that taxon's rank (a taxon
 *   without a rank starts at MC_NUM_RANKS and ends unclassified); threshold, voters, highest_rank, the final check and mc_assignment
 *   are as there.  lowest_rank is checked and not used.
 * mc_merge_results_set_taxids: id_of_row[x - 1] = the taxid of taxon entry x.  Needs mc_set_taxon_table first, with as many rows, and
 *   again after a later mc_set_taxon_table; duplicate ids are MC_ERR_INVALID.  Waits for the device.
 * mc_merge_results_begin: an empty store of capacity_queries lists (8 * max_candidates + 20 bytes per query); max_candidates beyond
 *   mc_merge_results_max_candidates (32) is MC_ERR_UNSUPPORTED.  mc_merge_results_reserve grows the store and keeps its content; both
 *   wait for the device.  mc_merge_results_end frees the store.
 * mc_merge_results_add folds one range.  file_lines is ignored with MC_MERGE_CONTINUE (the range continues the file of the previous
 *   call: no cut, duplicates are checked across the pieces); otherwise it is the file's number of result lines, 0 = "this range is the
 *   whole file: count them".  status[8] = result lines, comment lines, lists after the call, entries folded, unknown taxids, verdict,
 *   offence, capacity needed.  With a verdict other than MC_MERGE_OK NOTHING but status changes, and [3], [4] are 0; [7] is 0 with
 *   MC_MERGE_IRREGULAR.  MC_MERGE_OVERFLOW: some q, or file_lines, is beyond the capacity; [7] says what to reserve.
 *   Without MC_MERGE_HOST bytes, status and workspace are DEVICE pointers (bytes and workspace 16-byte, status 8-byte aligned; workspace
 *   of mc_merge_results_scratch_bytes(nbytes) bytes) and the call is enqueued on `stream` (NULL: the context's) without any
 *   synchronisation, neither between its passes nor between calls.  The calls on one context's store are ordered by the caller (one
 *   stream, or events).  The same calls give the same bytes.  With MC_MERGE_HOST bytes and status are HOST arrays (workspace may be
 *   NULL), staged through the context; the call returns when status is filled.
 * mc_merge_results_lists copies lists [first, first + count) (count * max_candidates pairs) and their header places ([count][3]);
 *   either array may be NULL; *num_queries (may be NULL) = the number of lists.  Lists beyond that number are empty.  flags: 0 (DEVICE
 *   pointers, enqueued) or MC_MERGE_HOST (returns when filled).
 * mc_merge_results_classify: out[i] = the assignment of query first + i.  flags as for mc_classify_candidates; MC_CLASSIFY_TALLY adds to
 *   the counters mc_classify_tally reads.  Those are sized by the lineage table; a context WITHOUT lineages sizes them by the taxon table
 *   (*num_counts = 1 + its rows, and mc_classify_tally then works without lineages), a context with lineages whose table names fewer
 *   taxa than the taxon table has rows gets MC_ERR_UNSUPPORTED for the flag.
 * mc_merge_results_stats: calls, bytes, result lines of accepted ranges, entries folded, unknown taxids, ranges refused; waits.
 * MC_ERR_INVALID (checked first, before any device call): NULL ctx, bytes, status or options, nbytes == 0 or > 2^31,
 *   tophits_column == 0, unknown flags, max_candidates == 0, misaligned device arrays, a workspace that is too small, NULL out with
 *   count > 0; with a store: first + count beyond its capacity.  MC_ERR_STATE: no taxon table, no taxid table, no begin,
 *   MC_MERGE_CONTINUE as the first call, or a context without a device (mc_open_metadata).  The calls work on a context without a
 *   loaded table (mc_create).  mc_timing_get names: "merge_results_validate", "merge_results_fold", "merge_results_vote". */
typedef struct { uint32_t taxon, hits; } mc_taxon_candidate;
#define MC_MERGE_HOST      1         /* bytes is a HOST array, staged through the context; the call returns when done */
#define MC_MERGE_CONTINUE  2         /* this range continues the file of the previous call */
#define MC_MERGE_OK        0
#define MC_MERGE_IRREGULAR 1
#define MC_MERGE_OVERFLOW  2
extern const uint32_t mc_merge_results_tile;             /* bytes one block owns the line starts of (for tests and tools) */
extern const uint32_t mc_merge_results_max_candidates;
int mc_merge_results_set_taxids(mc_ctx* ctx, const int64_t* id_of_row, uint64_t num_taxa);
int mc_merge_results_begin(mc_ctx* ctx, uint64_t capacity_queries, uint32_t max_candidates, int32_t merge_below);
int mc_merge_results_reserve(mc_ctx* ctx, uint64_t capacity_queries);
uint64_t mc_merge_results_scratch_bytes(uint64_t nbytes);
int mc_merge_results_add(mc_ctx* ctx, const char* bytes, uint64_t nbytes, uint32_t tophits_column, uint64_t file_lines, int flags,
                         uint64_t status[8], void* workspace, uint64_t workspace_bytes, void* stream);
int mc_merge_results_lists(mc_ctx* ctx, uint64_t first, uint64_t count, int flags, mc_taxon_candidate* lists, uint32_t* header_place,
                           uint64_t* num_queries, void* stream);
int mc_merge_results_classify(mc_ctx* ctx, const mc_classify_options* opt, int flags, uint64_t first, uint64_t count, mc_assignment* out,
                              void* stream);
int mc_merge_results_stats(mc_ctx* ctx, uint64_t stats[6]);
void mc_merge_results_end(mc_ctx* ctx);

/* ---- targets ranked from accession2taxid tables on the device: the ranking pass of build / modify ------
 * try_to_rank_unranked_targets (building.cpp:85-149, :196-229): every row "accession accession.version taxid gi" of a table names at
 * most one target, and a target that still has no parent takes the taxid of the FIRST row that names it.
 * THE NAMES are the target names (taxonomy_cache::name2tax_): `count` byte strings, name i = names[name_off[i] .. name_off[i + 1]),
 *   strictly ascending in unsigned byte order, a shorter prefix first (std::string::compare).  wanted[i] != 0: the name takes a taxid
 *   (an unranked target; under -reset-taxa every target).
 * THE TARGET OF A ROW `acc accver taxid gi` (building.cpp:122-130, taxonomy.hpp:1108-1127) is
 *   1. the name equal to accver;
 *   2. else the smallest name strictly greater than acc, if acc is a prefix of it (a name EQUAL to acc is thus skipped for the next
 *      longer one, or for none: the reference's upper_bound, kept);
 *   3. else the name equal to gi;
 *   4. else none.
 *   A row whose target is not wanted does nothing: it does not fall through to another name.
 * THE WINNER: each wanted name takes the taxid of the first row, in the order of the calls and then of the bytes, whose target it is.
 *   A taxid of 0 counts as found.  The position of the winner is call * 2^32 + line start, call = the number of the mc_taxmap_add call
 *   since mc_taxmap_begin (from 0, refused calls counted), line start = the offset into that call's range.
 * THE LINE RULE -- narrower than the reference's token stream `is >> acc >> accver >> taxid >> gi`: the device refuses more and never
 *   reads an accepted range differently.  A range is bytes[0, n), n <= 2^31; it begins at a line start, holds whole lines, and its last
 *   line may lack the '\n'.  The file's first line is not part of it (the reference drops it unread; so does the caller).  A regular
 *   line is: optional blanks (' ' or '\t'), four non-empty tokens of non-blank bytes separated by runs of blanks, optional blanks; its
 *   third token is 1-18 decimal digits; it has at most mc_taxmap_max_line (1 024) bytes, the '\n' not counted.  An empty or blank-only
 *   line, a '\r', '\v', '\f' or NUL byte, a line that is too long or any other deviation (fewer or more tokens, a third token that is
 *   not all digits or has 19 and more) makes the range MC_TAXMAP_IRREGULAR; the offence is the smallest line start of an offending
 *   line.  With any verdict but MC_TAXMAP_OK NOTHING but status changes.
 * mc_taxmap_begin: the names and their flags (HOST arrays, copied); every name is unfound afterwards.  Names that do not ascend
 *   strictly, descending offsets, count >= 2^31 or more than 2^32 - 1 bytes of names are MC_ERR_INVALID; count == 0 is allowed.  Waits
 *   for the device.  mc_taxmap_end frees the names.
 * mc_taxmap_add matches one range.  status[8] = lines, rows with a target, rows with a wanted target (wanted as mc_taxmap_begin
 *   flagged it), names this call ranked, names still wanted after it, verdict, offence, 0.  With MC_TAXMAP_IRREGULAR [1] - [3] are 0.
 *   Without MC_TAXMAP_HOST bytes, status and workspace are DEVICE pointers (bytes and workspace 16-byte, status 8-byte aligned; workspace
 *   of mc_taxmap_scratch_bytes(nbytes) bytes) and the call is enqueued on `stream` (NULL: the context's) without any synchronisation,
 *   neither between its passes nor between calls: a name's winner is a minimum over {call, line start}, so earlier calls win by
 *   themselves.  The calls on one context are ordered by the caller (one stream, or events), which is what makes [3] and [4] those of
 *   the call order.  The same calls give the same bytes.  With MC_TAXMAP_HOST bytes and status are HOST arrays (workspace may be NULL),
 *   staged through the context; the call returns when status is filled.
 * mc_taxmap_result: taxid[i] / position[i] of name i (either may be NULL); position all ones = not found, taxid 0 then.  flags: 0
 *   (DEVICE pointers, 8-byte aligned, enqueued on `stream`; remaining must be NULL) or MC_TAXMAP_HOST (returns when filled; *remaining,
 *   may be NULL, = the wanted names not found).
 * mc_taxmap_stats: calls, bytes, then of the accepted ranges lines, rows with a target, rows with a wanted target, names ranked; ranges
 *   refused; 0.  Waits for the device.
 * MC_ERR_INVALID (checked first, before any device call): NULL ctx, offsets, flags array (count > 0), bytes or status, nbytes == 0 or
 *   > 2^31, unknown flags, misaligned device arrays, a workspace that is too small.  MC_ERR_STATE: no mc_taxmap_begin, or a context
 *   without a device (mc_open_metadata).  The calls work on a context without a loaded table (mc_create).  mc_timing_get names:
 *   "taxmap_validate", "taxmap_match" (the match, finish and status launches). */
#define MC_TAXMAP_HOST      1        /* the arrays are HOST arrays, staged through the context; the call returns when done */
#define MC_TAXMAP_OK        0
#define MC_TAXMAP_IRREGULAR 1
extern const uint32_t mc_taxmap_tile;                    /* bytes one block owns the line starts of (for tests and tools) */
extern const uint32_t mc_taxmap_max_line;                /* bytes of the longest regular line, its '\n' not counted */
int mc_taxmap_begin(mc_ctx* ctx, const char* names, const uint64_t* name_off, uint64_t count, const uint8_t* wanted);
uint64_t mc_taxmap_scratch_bytes(uint64_t nbytes);
int mc_taxmap_add(mc_ctx* ctx, const char* bytes, uint64_t nbytes, int flags, uint64_t status[8], void* workspace, uint64_t workspace_bytes,
                  void* stream);
int mc_taxmap_result(mc_ctx* ctx, int64_t* taxid, uint64_t* position, uint64_t* remaining, int flags, void* stream);
int mc_taxmap_stats(mc_ctx* ctx, uint64_t stats[8]);
void mc_taxmap_end(mc_ctx* ctx);

/* ---- table content: what `metacache info <db> statistics | featurecounts | featuremap` asks for ------
 * The reference answers these from its hash table (host_hashmap.hpp:376-445, printing.cpp:662-696).  They describe the CONTENT of the
 * database -- how many features, how many locations, the distribution of the list sizes, which locations a feature has -- and here the
 * table in HBM is the only copy of that content, so three calls read it back.  They are also the way to state that a loaded table
 * holds exactly what its file (or the arrays given to mc_load_batch) says, whatever the layout of the store.
 * All three work on the bucket table of a context with ONE part, never on the direct-address index; all arrays are HOST arrays; the
 * calls run on the context's own stream and return when their work is done.  NO QUERY MAY BE IN FLIGHT on the context's first pipe
 * (mc_query_device without MC_SECOND_PIPE, mc_candidates_from_*) meanwhile.  `flags` is reserved and must be 0.
 * mc_table_histogram: hist[s] = stored features whose list has s locations, s = 0 .. 255 (hist[0] is always 0: a feature that the
 *   load-time rules emptied is not stored); *dead (may be NULL) = features handed to the loader (the number announced to mc_load_begin,
 *   once all of them are in) that remove_overpopulated emptied = handed over - stored.  Features, locations, the largest size and the
 *   moments of the statistics line follow from hist in exact integers.
 * mc_table_features: every stored feature in ASCENDING feature order with its list size; *num = their number, the first
 *   min(capacity, *num) are copied.  keys / sizes may be NULL with capacity 0 (the size query, which does not sort).
 * mc_table_lookup: the lists of n features, in the order given -- any order, duplicates allowed, a feature that is not stored has an
 *   empty list: list i = locs[offsets[i] .. offsets[i + 1]) in the order of the database file (after max_locations_per_feature: its
 *   first locations), offsets has n + 1 entries.  If offsets[n] > capacity: MC_ERR_NOMEM, NO entry of locs is written, offsets is
 *   complete (the convention of mc_format_mappings), so that the caller can size locs and call again.  n == 0: MC_OK, offsets[0] = 0.
 * Errors, the arguments before any device call: MC_ERR_INVALID: NULL ctx, hist, num or offsets, NULL keys with n > 0 (mc_table_features:
 *   NULL keys or sizes with capacity > 0), NULL locs with capacity > 0, flags != 0.  MC_ERR_STATE: a context without a device
 *   (mc_open_metadata), a table that is not finished (mc_load_end not yet called).  MC_ERR_UNSUPPORTED: more than one part in the context
 *   (a list of the union is not a list of a file: open the parts one by one, mc_config.single_part), a key shard, a target-range shard,
 *   a stored size above 255.  MC_ERR_NOMEM also: the device cannot hold the temporaries (mc_table_features: 16 bytes per stored feature
 *   + the sort's own; mc_table_lookup: 24 bytes per key and 8 per location of a piece); the error text names the bytes asked for.
 * mc_timing_get names: "table_hist", "table_enumerate" (the write pass + the sort), "table_lookup" (sizes + offsets), "table_gather". */
int mc_table_histogram(mc_ctx* ctx, uint64_t hist[256], uint64_t* dead);
int mc_table_features(mc_ctx* ctx, uint32_t* keys, uint32_t* sizes, uint64_t capacity, uint64_t* num, int flags);
int mc_table_lookup(mc_ctx* ctx, const uint32_t* keys, uint64_t n, uint64_t* offsets, mc_location* locs, uint64_t capacity, int flags);

/* per-kernel timing with HIP events on the launching stream (for bench.py's roofline block).
 * names: "plan", "sketch_lane", "chunk_sketch", "chunk_probe", "probe_cands", "mid_cands_64", "mid_cands_128", "mid_cands_256",
 * "hash_cands_256", "hash_cands_512", "hash_cands_1024", the filtered path -- compact location store: "gw_filter_count" (gw_filter_count_kernel; "gw_filter" with
 * the tuning switch "gw_fuse" 0), "gw_filter2", "gw_compact" (+ the ordering of the stream filter's reads), "gw_filter_stream_fine" (the sixteen-wave instance), "gw_filter_stream" (+ the second gw_compact), "gw_count" (gw_count_kernel<9>), "gw_count_512" (<10>), "gw_count_1024" (<11>); 8-byte store:
 * "big_filter", "big_filter_2", "big_count", "big_count_2" --, "gw_sort", "gw_sorted_cands", "query_wave", "scan", "sort_candidates";
 * Mode K: "mask_features", "gather_lists", "pack_numbers", "owner_entries", "decode_union"; "sketch_probe" (sketch_probe_lane_kernel: instead of "sketch_lane" + "probe_cands" where the two are one kernel, see "lane_fusion"); "cands_from_hits" (mc_candidates_from_hits); "coverage_count_kernel" (inside mc_coverage_counts); "target_hits_sort" (block sort + merge passes) and "target_hits_bounds" (inside mc_target_hits_collect); "taxon_evaluate" (taxon_evaluate_kernel, mc_evaluate_assignments); "format_lengths" (format_lengths_kernel + tile_scan_kernel) and "format_write" (format_write_kernel, mc_format_mappings).  Returns accumulated milliseconds and launch counts since the last reset. */
int mc_timing_enable(mc_ctx* ctx, int on);
int mc_timing_reset(mc_ctx* ctx);
int mc_timing_get(mc_ctx* ctx, const char* kernel, double* total_ms, uint64_t* launches);

/* workload statistics of the LAST mc_query_device call (device reductions, synchronises):
 * stats[0] = total windows, [1] = valid features probed (F), [2] = locations returned (H),
 * [3] = features found in table, [4] = probe steps (bucket groups read) */
int mc_last_batch_stats(mc_ctx* ctx, uint64_t stats[8]);

/* ---- minimal database builder ------------------------------------------
 * Needed so that synthetic databases can be produced on the GPU box itself; it re-uses the
 * parity-proven sketch kernel.  Mirrors database::add_target (database.cpp:34-81) +
 * host_hashmap::add_target (host_hashmap.hpp:570-589) for a SINGLE-threaded build: target ids in
 * call order, window ids = running index of windows with >= k characters, buckets hold the first
 * max_locations_per_feature locations in (target, window) order (host_hashmap.hpp:593-605), and
 * database::write (database.cpp:247-325) for the file format.  cfg fields used: device, kmerlen,
 * sketchlen, winlen, winstride, target_id_bytes, max_locations_per_feature (0 => 254), remove_overpopulated (!= 0 => features
 * that reached the limit are dropped from the files and the table: -remove-overpopulated-features, building.cpp:516-534),
 * key_shard_index / key_shard_count (> 1: only this shard's features are kept; see mc_build_finish_shards). */
typedef struct mc_builder mc_builder;
typedef struct {
    int64_t  id;
    int64_t  parent;
    uint32_t rank;          /* taxonomy::rank as integer (taxonomy.hpp:68-91), 21 = none */
    const char* name;
} mc_taxon_rec;

int  mc_build_begin(const mc_config* cfg, mc_builder** out);
int  mc_build_add_target(mc_builder* b, const char* seq, uint64_t len, const char* name, int64_t parent_taxid,
                         const char* source_filename);
/* the same with the position of the sequence inside its file (taxon::file_source::index, building.cpp:414-416) */
int  mc_build_add_target_src(mc_builder* b, const char* seq, uint64_t len, const char* name, int64_t parent_taxid,
                             const char* source_filename, uint64_t source_index);
/* the same for a sequence that already lies in DEVICE memory (start 4-byte aligned, 16 readable bytes behind its last character):
 * nothing is staged or copied, the sketch kernels read it in place.  The memory must stay untouched until mc_build_flush or
 * mc_build_finish returns.  (The reference's GPU build takes host sequences only, gpu_hashmap.cu:1024-1120; collections that
 * are generated or decoded on the device -- bench.py's RefSeq-scale synthetic database -- go in without a PCIe round trip.) */
int  mc_build_add_target_device(mc_builder* b, const void* dseq, uint64_t len, const char* name, int64_t parent_taxid,
                                const char* source_filename, uint64_t source_index);
/* sketches everything staged so far (sources of mc_build_add_target_device calls may be reused afterwards) */
int  mc_build_flush(mc_builder* b);
/* allocates room for this many (feature, location) pairs up front (a builder that grows step by step holds two copies while growing) */
int  mc_build_reserve(mc_builder* b, uint64_t pairs);
/* re-ranks a target after it was added (try_to_rank_unranked_targets, building.cpp:196-232) */
int  mc_build_set_parent(mc_builder* b, uint64_t target, int64_t parent_taxid);
/* modify mode (main_mode_modify, mode_build.cpp:74-88: an existing database is read, then added to): the database's targets
 * (taxon::file_source fields from mc_db_taxon / mc_db_taxon_source) and the batches of its .cache file (hash_multimap.hpp:1037-1082:
 * keys, bucket sizes, packed {u32 window, target id of target_bytes} values) go into a fresh builder BEFORE the first new target;
 * their lists keep their order and stand in front of what is sketched afterwards, as in the reference's table after reading. */
int  mc_build_add_existing_target(mc_builder* b, const char* name, int64_t parent_taxid, const char* source_filename,
                                  uint64_t source_index, uint64_t windows);
int  mc_build_add_locations(mc_builder* b, const uint32_t* keys, const uint8_t* sizes, const void* values, uint64_t num_keys,
                            uint32_t target_bytes);
/* after mc_build_finish: features and locations the builder holds (database::feature_count / location_count, database.hpp:420-440) */
int  mc_build_counts(const mc_builder* b, uint64_t* keys, uint64_t* values);
/* After mc_build_finish: drops every feature whose locations lie in more than max_ambig (0 => 1) different taxa on one rank
 * (-remove-ambig-features <rank> -max-ambig-per-feature <n>: database.hpp:259-270, host_hashmap.hpp:499-540, called from
 * post_process_features, building.cpp:550-566).  ancestor_of_target[t] = any id of target t's ancestor on that rank, 0 = none
 * (all targets without one count as ONE taxon, as the reference's null pointer does); rank 'sequence': t + 1.  Key-sharded
 * builders: call it on every shard.  *removed (may be NULL) = number of features dropped. */
int  mc_build_remove_ambiguous(mc_builder* b, const uint32_t* ancestor_of_target, uint64_t num_targets, uint32_t max_ambig,
                               uint64_t* removed);
/* number of windows of a target (taxon::file_source::windows, database.cpp:64) */
int  mc_build_target_windows(const mc_builder* b, uint64_t target, uint64_t* windows);
/* sorts + bucketises everything added so far; if out_ctx != NULL also loads the table into a fresh
 * query context (see mc_build_set_query_config). */
int  mc_build_finish(mc_builder* b, mc_ctx** out_ctx);
/* One query table from n builders that were given the SAME targets and the key shards 0 .. n-1 of n (cfg.key_shard_index / _count:
 * a builder keeps only the features of its shard, as a Mode K context does): tables beyond the 2^32 (feature, location) pairs one
 * device sort takes are built shard after shard.  n == 1: the loading half of mc_build_finish. */
int  mc_build_finish_shards(mc_builder** builders, uint32_t n, mc_ctx** out_ctx);
/* Streaming form of mc_build_finish_shards for tables that do not fit next to all their builders (RefSeq scale: 2 x 10^10 locations):
 *   mc_build_table_begin  creates the query context and sizes its table for expect_keys features / expect_values locations
 *                         (0 = estimate from the FINISHED builder b: its counts times its key_shard_count, plus a margin);
 *   mc_build_table_add    inserts one finished builder -- a whole one or one key shard, same targets -- from its device arrays;
 *                         the builder can be freed right after;
 *   mc_build_table_end    closes the load (mc_load_end).  More keys or locations than announced fail with MC_ERR_INVALID.
 * Between _begin and _end (and between mc_partset_open and mc_partset_close) device blocks of 64 MB and more that the library frees are kept
 * for its next allocation of that size instead of going back to the device -- hipMalloc hands out scrubbed memory at ~18 GB/s, which was
 * most of a build's and of a part group's time --: at most MC_DEVCACHE_GB (environment, default 64) gigabytes, released by the closing
 * call or when an allocation cannot be served. */
int  mc_build_table_begin(mc_builder* b, uint64_t expect_keys, uint64_t expect_values, mc_ctx** out_ctx);
int  mc_build_table_add(mc_ctx* ctx, mc_builder* shard);
int  mc_build_table_end(mc_ctx* ctx);
/* fields of the query context mc_build_finish creates (max_candidates, slots, copy_allhits, load factor) */
int  mc_build_set_query_config(mc_builder* b, const mc_config* qcfg);
/* writes <name>.meta and <name>.cache0 in the reference's format (after mc_build_finish) */
int  mc_build_write(mc_builder* b, const char* name, const mc_taxon_rec* taxa, uint64_t ntaxa);
/* the same for the builders of one key-sharded set (see mc_build_finish_shards): one complete database */
int  mc_build_write_shards(mc_builder** builders, uint32_t n, const char* name, const mc_taxon_rec* taxa, uint64_t ntaxa);
/* the same shard by shard (a RefSeq-scale set of builders does not exist at once): begin writes <name>.meta (targets of b) and opens
 * <name>.cache0, add appends one finished builder (key shards 0 .. n-1 in order), end patches the totals into the header and closes;
 * any failure removes both files. */
typedef struct mc_db_writer mc_db_writer;
int  mc_build_write_begin(mc_builder* b, const char* name, const mc_taxon_rec* taxa, uint64_t ntaxa, mc_db_writer** out);
int  mc_build_write_add(mc_db_writer* w, mc_builder* shard);
int  mc_build_write_end(mc_db_writer* w);
void mc_build_free(mc_builder* b);
const char* mc_build_last_error(const mc_builder* b);

#ifdef __cplusplus
}
#endif
#endif /* METACACHE_AMD_H_ */
