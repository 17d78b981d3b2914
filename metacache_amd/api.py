"""ctypes binding of the C ABI in include/metacache_amd.h (the product's only entry points).

There is deliberately no CPU path here: if libmetacache_amd.so cannot be built / loaded, or no GPU
is usable, every call raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from . import build as _build

MC_OK, MC_BATCH_FULL = 0, 1
MC_ERR_NOMEM = -3
NUM_RANKS = 21

cand_dtype = np.dtype([("tgt", "<u4"), ("hits", "<u4"), ("beg", "<u4"), ("end", "<u4")])
loc_dtype = np.dtype([("win", "<u4"), ("tgt", "<u4")])
qstat_dtype = np.dtype([("hits", "<u4"), ("nfeat", "<u4"), ("nfound", "<u4"), ("nsteps", "<u4")])
assignment_dtype = np.dtype({"names": ["taxon", "rank", "voters"], "formats": ["<u4", "u1", "u1"], "offsets": [0, 4, 5], "itemsize": 8})   # mc_assignment, info split into its bytes
CLASSIFY_HOST, CLASSIFY_TALLY = 1, 2
COVERAGE_HOST = 1
TARGET_HITS_HOST = 1
EVALUATE_HOST, EVALUATE_TALLY, EVALUATE_COVERAGE = 1, 2, 4
FORMAT_HOST, FORMAT_QUERY_IDS, FORMAT_TRUTH, FORMAT_TOPHITS, FORMAT_LOCATIONS, FORMAT_MAPPED_ONLY = 1, 2, 4, 8, 16, 32
FORMAT_SCRATCH = 2048                    # MC_FORMAT_SCRATCH: entries of workspace behind a device line_off
MATCHES_WINDOWS = 2                      # MC_MATCHES_WINDOWS: mc_format_matches prints text/window:length, instead of text:length,
TEXT_RESULT, TEXT_TARGET_RESULT, TEXT_CANDIDATE = 0, 1, 2
verdict_dtype = np.dtype([("known", "u1"), ("correct", "u1"), ("flags", "u1"), ("reserved", "u1")])   # mc_verdict: kr, cr, bit 0 = counted wrong
RANK_NAMES = ["sequence", "form", "variety", "subspecies", "species", "subgenus", "genus", "subtribe", "tribe", "subfamily", "family",
              "suborder", "order", "subclass", "class", "subphylum", "phylum", "subkingdom", "kingdom", "domain", "root"]
target_hit_dtype = np.dtype([("tgt", "<u4"), ("beg", "<u4"), ("end", "<u4"), ("hits", "<u4"), ("query", "<u8")])   # mc_target_hit, 24 bytes


class McConfig(C.Structure):
    _fields_ = [("device", C.c_int32), ("kmerlen", C.c_uint32), ("sketchlen", C.c_uint32), ("winlen", C.c_uint32),
                ("winstride", C.c_uint32), ("max_candidates", C.c_uint32), ("target_id_bytes", C.c_uint32),
                ("num_parts", C.c_uint32), ("max_locations_per_feature", C.c_uint32), ("remove_overpopulated", C.c_uint32),
                ("max_load_factor", C.c_float), ("num_slots", C.c_uint32), ("slot_max_queries", C.c_uint32),
                ("slot_max_chars", C.c_uint32), ("copy_allhits", C.c_uint32), ("single_part", C.c_int32),
                ("key_shard_index", C.c_uint32), ("key_shard_count", C.c_uint32),
                ("target_shard_index", C.c_uint32), ("target_shard_count", C.c_uint32)]


class McResults(C.Structure):
    _fields_ = [("num_queries", C.c_uint32), ("max_candidates", C.c_uint32), ("cands", C.c_void_p),
                ("hit_offsets", C.c_void_p), ("hits", C.c_void_p), ("hit_counts", C.c_void_p)]


class McDeviceBatch(C.Structure):
    _fields_ = [("seq", C.c_void_p), ("qinfo", C.c_void_p), ("max_win", C.c_void_p), ("max_win_uniform", C.c_uint32),
                ("num_queries", C.c_uint32), ("num_chars", C.c_uint64)]


class McDeviceHits(C.Structure):
    _fields_ = [("hits", C.c_void_p), ("hit_offsets", C.c_void_p), ("max_win", C.c_void_p), ("max_win_uniform", C.c_uint32),
                ("num_queries", C.c_uint32)]


class McDevicePartialHits(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("hits", C.c_void_p), ("total_hits", C.c_uint64), ("max_win", C.c_void_p), ("max_win_uniform", C.c_uint32),
                ("num_queries", C.c_uint32), ("num_sources", C.c_uint32)]


class McDevicePartialNumbers(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("numbers", C.c_void_p), ("total", C.c_uint64)]


class McDevicePartialNumbersIn(C.Structure):
    _fields_ = [("counts", C.c_void_p), ("numbers", C.c_void_p), ("source_offsets", C.c_void_p), ("max_win", C.c_void_p), ("max_win_uniform", C.c_uint32),
                ("num_queries", C.c_uint32), ("num_sources", C.c_uint32)]


class McClassifyOptions(C.Structure):
    _fields_ = [("hits_min", C.c_uint32), ("hits_diff", C.c_float), ("lowest_rank", C.c_int32), ("highest_rank", C.c_int32)]


def hitdiff_factor(hitdiff: float) -> float:
    """-hitdiff as the command line reads it (options.cpp:1312): the value is kept as a float, one above 1 is a percentage --
    times 0.01 in double, rounded back to float"""
    v = np.float32(hitdiff)
    if v > np.float32(1):
        v = np.float32(np.float64(v) * 0.01)
    return float(v)


def percentile_factor(percentile: float) -> float:
    """-cov-percentile as the command line reads it (options.cpp:1313): kept as a float, a value above 1 is a percentage -- times
    0.01 in double, rounded back to float"""
    v = np.float32(percentile)
    if v > np.float32(1):
        v = np.float32(np.float64(v) * 0.01)
    return float(v)


def coverage_keep(covered, windows, percentile: float, order=None) -> np.ndarray:
    """mc_coverage_keep (filter_targets_by_coverage): covered / windows per target, percentile as on the command line (above 1 =
    percent), order = the target ids in visiting order (None: ascending) -> keep[targets] uint8"""
    covered = np.ascontiguousarray(covered, dtype=np.uint32)
    windows = np.ascontiguousarray(windows, dtype=np.uint32)
    if covered.shape != windows.shape or covered.ndim != 1:
        raise ValueError("coverage_keep: covered and windows must be one-dimensional and of one length")
    keep = np.zeros(len(covered), dtype=np.uint8)
    o = None if order is None else np.ascontiguousarray(order, dtype=np.uint32)
    rc = lib().mc_coverage_keep(covered.ctypes.data, windows.ctypes.data, len(covered), None if o is None else o.ctypes.data,
                                0 if o is None else len(o), percentile_factor(percentile), keep.ctypes.data)
    if rc != MC_OK:
        raise McError(f"mc_coverage_keep -> {rc}: percentile outside [0, 1] or not finite, or an id of `order` repeated or beyond the targets")
    return keep


def target_hits_tile() -> int:
    """records one block of the collect-side sort takes (the library's mc_target_hits_tile): n records take ceil(log2(ceil(n / tile))) merge passes"""
    return int(C.c_uint32.in_dll(lib(), "mc_target_hits_tile").value)


def parse_tile() -> int:
    """bytes one block of the parse kernels classifies (the library's mc_parse_tile): what lies in front of a tile comes from a scan over the tiles"""
    return int(C.c_uint32.in_dll(lib(), "mc_parse_tile").value)


def merge_results_tile() -> int:
    """bytes one block of the merge kernels owns the line starts of (the library's mc_merge_results_tile)"""
    return int(C.c_uint32.in_dll(lib(), "mc_merge_results_tile").value)


def taxmap_tile() -> int:
    """bytes one block of the taxmap kernels owns the line starts of (the library's mc_taxmap_tile)"""
    return int(C.c_uint32.in_dll(lib(), "mc_taxmap_tile").value)


def taxmap_max_line() -> int:
    """bytes of the longest line mc_taxmap_add accepts, its line end not counted (the library's mc_taxmap_max_line)"""
    return int(C.c_uint32.in_dll(lib(), "mc_taxmap_max_line").value)


def taxmap_scratch_bytes(nbytes: int) -> int:
    """bytes of the device workspace of mc_taxmap_add for a range of nbytes bytes"""
    return int(lib().mc_taxmap_scratch_bytes(nbytes))


def merge_results_scratch_bytes(nbytes: int) -> int:
    """bytes of device workspace ResultMerger.add_device needs for a range of nbytes bytes"""
    return int(lib().mc_merge_results_scratch_bytes(nbytes))


def parse_scratch_bytes(nbytes: int) -> int:
    """the workspace a device call of mc_parse_records needs for a range of nbytes"""
    return int(lib().mc_parse_scratch_bytes(nbytes))


PARSE_HOST, PARSE_PAIRS, CUT_OPEN = 1, 2, 4
INPUT_OK, INPUT_NOT_BGZF, INPUT_REFUSED, INPUT_TOO_LARGE, INPUT_NO_MEMORY, INPUT_EMPTY, INPUT_IRREGULAR, INPUT_RECORD_TOO_LARGE = range(8)
input_batch_dtype = np.dtype([("offset", "<u8"), ("nbytes", "<u8"), ("records", "<u4"), ("queries", "<u4"), ("half_pair", "<u4"), ("too_big", "<u4")])
PARSE_OK, PARSE_IRREGULAR, PARSE_OVERFLOW, PARSE_UNEQUAL = 0, 1, 2, 3


BGZF_OK, BGZF_FOREIGN = 0, 1
INFLATE_HOST = 1
INFLATE_OK, INFLATE_CORRUPT, INFLATE_OVERFLOW = 0, 1, 2
(INFLATE_R_BTYPE, INFLATE_R_STORED, INFLATE_R_LENGTHS, INFLATE_R_SYMBOL, INFLATE_R_DISTANCE, INFLATE_R_INPUT, INFLATE_R_OVER, INFLATE_R_SHORT,
 INFLATE_R_LEFT, INFLATE_R_CRC) = range(1, 11)
bgzf_block_dtype = np.dtype([("in_off", np.uint64), ("out_off", np.uint64), ("in_len", np.uint32), ("out_len", np.uint32)])   # mc_bgzf_block


def bgzf_index(data, capacity=None):
    """the members of a BGZF range (mc_bgzf_index; host code, no device): -> (blocks bgzf_block_dtype [members], out_bytes, verdict,
    offence).  With BGZF_FOREIGN the blocks are the members in front of the offence.  capacity: room for that many rows only (the
    counts stay complete)."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = np.zeros(4, dtype=np.uint64)

    def run(blocks):
        rc = lib().mc_bgzf_index(buf.ctypes.data if len(buf) else None, len(buf), blocks.ctypes.data if len(blocks) else None, len(blocks), info.ctypes.data)
        if rc < 0:
            raise McError(f"mc_bgzf_index -> {rc}: {lib().mc_last_error(None).decode()}")

    blocks = np.zeros(0 if capacity is None else capacity, dtype=bgzf_block_dtype)
    run(blocks)
    if capacity is None and int(info[0]):
        blocks = np.zeros(int(info[0]), dtype=bgzf_block_dtype)
        run(blocks)
    return blocks[:min(len(blocks), int(info[0]))], int(info[1]), int(info[2]), int(info[3])


GZIP_OK, GZIP_FOREIGN = 0, 1
INFLATE_R_HEADER, INFLATE_R_TRAILING = 11, 12
gzip_stream_dtype = np.dtype([("in_off", np.uint64), ("in_len", np.uint64), ("out_off", np.uint64), ("out_cap", np.uint64)])   # mc_gzip_stream
gzip_result_dtype = np.dtype([("produced", np.uint64), ("members", np.uint32), ("reason", np.uint32)])                       # mc_gzip_result


def gzip_hint(data):
    """what a gzip file's first header and last four bytes say (mc_gzip_hint; host code, no device): -> (verdict GZIP_OK / GZIP_FOREIGN,
    the offset of the first member's deflate stream, the trailing ISIZE, the offence: an INFLATE_R_* reason)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    info = np.zeros(4, dtype=np.uint64)
    rc = lib().mc_gzip_hint(buf.ctypes.data if len(buf) else None, len(buf), info.ctypes.data)
    if rc < 0:
        raise McError(f"mc_gzip_hint -> {rc}: {lib().mc_last_error(None).decode()}")
    return int(info[0]), int(info[1]), int(info[2]), int(info[3])


def parse_cut_scratch_bytes(nbytes: int) -> int:
    """the workspace a device call of mc_parse_cut needs for a range of nbytes"""
    return int(lib().mc_parse_cut_scratch_bytes(nbytes))


def parse_headers_scratch_bytes(max_records: int) -> int:
    """the workspace a device call of mc_parse_headers needs for outputs of max_records records"""
    return int(lib().mc_parse_headers_scratch_bytes(max_records))


def parse_mates_scratch_bytes(n1: int, n2: int, max_records: int) -> int:
    """the workspace a device call of mc_parse_mates needs for ranges of n1 and n2 bytes and outputs of max_records records"""
    return int(lib().mc_parse_mates_scratch_bytes(n1, n2, max_records))


class McParseOutput(C.Structure):
    _fields_ = [("hdr", C.c_void_p), ("qinfo", C.c_void_p), ("seq", C.c_void_p), ("seq_capacity", C.c_uint64), ("names", C.c_void_p),
                ("names_capacity", C.c_uint64), ("name_off", C.c_void_p), ("max_win", C.c_void_p), ("status", C.c_void_p), ("max_records", C.c_uint32)]


class McParseTargetsOutput(C.Structure):
    _fields_ = [("hdr", C.c_void_p), ("targets", C.c_void_p), ("seq", C.c_void_p), ("seq_capacity", C.c_uint64), ("status", C.c_void_p), ("max_records", C.c_uint32)]


parse_target_dtype = np.dtype([("seq_off", "<u8"), ("len", "<u4"), ("file", "<u4"), ("index", "<u4"), ("reserved", "<u4")])   # mc_parse_target


def parse_targets_scratch_bytes(nbytes: int, num_files: int, max_records: int) -> int:
    """the workspace a device call of mc_parse_targets needs for a range of nbytes in num_files files and outputs of max_records records"""
    return int(lib().mc_parse_targets_scratch_bytes(nbytes, num_files, max_records))


class McBatchRecordInfo(C.Structure):
    _fields_ = [("verdict", C.c_uint32), ("records", C.c_uint32), ("queries", C.c_uint32), ("half_pair", C.c_uint32), ("offence", C.c_uint64),
                ("hdr", C.c_void_p), ("qinfo", C.c_void_p)]


def classify_options(hitmin: int = 0, hitdiff: float = 1.0, lowest: int = 0, highest: int = NUM_RANKS - 1) -> McClassifyOptions:
    return McClassifyOptions(int(hitmin), hitdiff_factor(hitdiff), int(lowest), int(highest))


class McFormatOptions(C.Structure):
    _fields_ = [("column", C.c_char * 16), ("column_len", C.c_uint32), ("win_stride", C.c_uint32), ("win_len", C.c_uint32)]


def format_options(column: bytes = b"\t|\t", win_stride: int = 0, win_len: int = 0) -> McFormatOptions:
    """mc_format_options: the column separator (at most 16 bytes; a longer one is handed over as it is for the library to refuse) and
    the database's window stride and length"""
    o = McFormatOptions()
    C.memmove(C.addressof(o), bytes(column[:16]), min(len(column), 16))
    o.column_len, o.win_stride, o.win_len = len(column), int(win_stride), int(win_len)
    return o


def format_flags(*, query_ids=False, truth=False, tophits=False, locations=False, mapped_only=False) -> int:
    return ((FORMAT_QUERY_IDS if query_ids else 0) | (FORMAT_TRUTH if truth else 0) | (FORMAT_TOPHITS if tophits else 0) |
            (FORMAT_LOCATIONS if locations else 0) | (FORMAT_MAPPED_ONLY if mapped_only else 0))


def pack_strings(strings):
    """list of bytes -> (bytes, offsets uint64 [len + 1]): the form of mc_format_set_text and of the names of mc_format_mappings"""
    off = np.zeros(len(strings) + 1, dtype=np.uint64)
    if len(strings):
        off[1:] = np.cumsum([len(x) for x in strings], dtype=np.uint64)
    return b"".join(strings), off


def mapping_texts(taxa, taxon_lin, target_lin, *, lowest: int = 0, highest: int = NUM_RANKS - 2, taxids: bool = False, taxids_only: bool = False,
                  omit_ranks: bool = False, lineage: bool = False, separate_cols: bool = False, separator: str = "\t|\t", none: str = "--"):
    """The three string tables of mc_format_set_text for one set of output options, built as the command line prints
    (print_taxon, show_lineage, show_taxon, show_candidates; printing.cpp:160-310).  taxa: (id, parent, rank, name) per taxon as
    Database.taxa() gives them; taxon_lin[taxa, 21] and target_lin[targets, 21]: Database.taxon_table()[0] and Database.lineages()
    (taxon index + 1, 0 = none); lowest / highest: the ranks of -lowest / -highest (the command line's defaults: sequence .. domain).
    Needs no device: all three come from an mc_open_metadata context.
    -> {TEXT_RESULT: [bytes per taxon index + 1, entry 0 = unclassified], TEXT_TARGET_RESULT: [bytes per target],
        TEXT_CANDIDATE: [bytes per target]}"""
    show_id, show_name, show_rank = taxids or taxids_only, not taxids_only, not omit_ranks
    if lowest > highest:
        lowest = highest
    collapse, tax_sep, rank_suffix, id_prefix, id_suffix = True, ",", ":", "(", ")"
    if separate_cols:
        collapse, tax_sep, rank_suffix, id_prefix, id_suffix = False, separator, separator, separator, ""

    def print_taxon(name, tid, rank):
        s = ""
        if show_rank:
            s += (none if rank == NUM_RANKS else RANK_NAMES[rank]) + rank_suffix
        if show_name:
            s += name + (id_prefix + str(tid) + id_suffix if show_id else "")
        elif show_id:
            s += str(tid)
        return s

    def show_lineage(lin, lo, hi):
        parts = []
        for r in range(lo, hi + 1):
            x = int(lin[r])
            parts.append(print_taxon(taxa[x - 1][3], taxa[x - 1][0], taxa[x - 1][2]) if x else print_taxon(none, 0, r))
        return tax_sep.join(parts)

    def show_taxon(best, lin):
        if not best or taxa[best - 1][2] > highest:
            if collapse:
                return "0" if (show_id and not show_name and not show_rank) else none
            rmax = highest if lineage else lowest
            return tax_sep.join(print_taxon(none, 0, NUM_RANKS) for _ in range(lowest, rmax + 1))
        rmin = max(lowest, taxa[best - 1][2])
        return show_lineage(lin, rmin, highest if lineage else rmin)

    def candidate(row):
        if lowest == 0:
            x = int(row[0])
            return taxa[x - 1][3] if x else ""
        x = next((int(v) for v in row[lowest:] if v), 0)
        return str(taxa[x - 1][0]) if x else ""

    zeros = np.zeros(NUM_RANKS, dtype=np.uint32)
    result = [show_taxon(0, zeros)] + [show_taxon(x + 1, taxon_lin[x]) for x in range(len(taxa))]
    target_result = [show_taxon(int(row[0]), row) for row in target_lin]
    cand = [candidate(row) for row in target_lin]
    enc = lambda l: [x.encode() for x in l]
    return {TEXT_RESULT: enc(result), TEXT_TARGET_RESULT: enc(target_result), TEXT_CANDIDATE: enc(cand)}


def match_texts(taxa, target_lin, lowest: int = 0):
    """The table of mc_format_matches_set_text as the command line prints -allhits (show_matches, printing.cpp:315-365): per target the
    name of its own taxon (lowest == 0: the window form, MATCHES_WINDOWS; a target without a taxon has an empty entry and prints
    nothing), else the name of its ancestor on exactly rank `lowest`, or of its own taxon where it has none there.
    taxa / target_lin: as for mapping_texts.  -> [bytes per target]"""
    def name(x):
        return taxa[x - 1][3].encode() if x else b""
    return [name(int(row[0])) if lowest == 0 else name(int(row[lowest]) or int(row[0])) for row in target_lin]


class McEvaluation(C.Structure):
    _fields_ = [("assigned", C.c_uint64 * (NUM_RANKS + 1)), ("known", C.c_uint64 * (NUM_RANKS + 1)), ("correct", C.c_uint64 * (NUM_RANKS + 1)),
                ("wrong", C.c_uint64 * (NUM_RANKS + 1)), ("coverage", (C.c_uint64 * 4) * (NUM_RANKS + 1)), ("reads", C.c_uint64),
                ("out_of_table", C.c_uint64)]


class Confusion:
    """confusion_statistics of one rank (classification_statistics.hpp): the four counters of -taxon-coverage"""

    def __init__(self, row):
        self._tp, self._fp, self._tn, self._fn = (int(x) for x in row)

    def true_pos(self): return self._tp
    def false_pos(self): return self._fp
    def true_neg(self): return self._tn
    def false_neg(self): return self._fn
    def total(self): return self._tp + self._fp + self._tn + self._fn


class Evaluation:
    """The reference's classification_statistics (classification_statistics.hpp:135-227) over the per-rank bins of mc_evaluate_tally:
    bins[0..3] = assigned, known, correct, wrong ([22] each, [21] = none), coverage[22, 4] = true_pos, false_pos, true_neg, false_neg.
    A rank argument is the rank's number (0 = sequence .. 20 = root); without one the figure is over all ranks."""
    SUMMARY_RANKS = (0, 3, 4, 6, 10, 12, 14, 16, 18, 19, 20)      # what show_taxon_statistics prints (printing.cpp:505-513)

    def __init__(self, assigned, known, correct, wrong, coverage=None, reads=0, out_of_table=0):
        self.bins = np.array([assigned, known, correct, wrong], dtype=np.uint64).reshape(4, NUM_RANKS + 1)
        self.confusion = (np.zeros((NUM_RANKS + 1, 4), dtype=np.uint64) if coverage is None
                          else np.array(coverage, dtype=np.uint64).reshape(NUM_RANKS + 1, 4))
        self.reads, self.out_of_table = int(reads), int(out_of_table)

    def _upto(self, k, r):
        return int(self.bins[k, :(NUM_RANKS if r is None else r + 1)].sum())

    def assigned(self, r=None): return self._upto(0, r)
    def known(self, r=None): return self._upto(1, r)
    def correct(self, r=None): return self._upto(2, r)
    def wrong(self, r=None): return int(self.bins[3, (0 if r is None else r):NUM_RANKS].sum())
    def unassigned(self): return int(self.bins[0, NUM_RANKS])
    def unknown(self): return int(self.bins[1, NUM_RANKS])
    def total(self): return self.assigned() + self.unassigned()
    def _rate(self, x): return x / float(self.total()) if self.total() > 0 else 0.0
    def known_rate(self, r=None): return self._rate(self.known(r))
    def unknown_rate(self): return self._rate(self.unknown())
    def classification_rate(self, r): return self._rate(self.assigned(r))
    def unclassified_rate(self): return self._rate(self.unassigned())
    def sensitivity(self, r): return self.correct(r) / float(self.known(r)) if self.known(r) > 0 else 0.0

    def precision(self, r):
        tot = float(self.correct(r) + self.wrong(r))              # (in general neither assigned(r) nor known(r))
        return self.correct(r) / tot if tot > 0 else 0.0

    def coverage(self, r): return Confusion(self.confusion[r])

    def summary_lines(self, comment="# "):
        """show_taxon_statistics (printing.cpp:500-592) from 'unclassified:' to the end, numbers as the reference's stream prints them
        (%g: six significant digits)"""
        if self.assigned() < 1:
            return ["None of the input sequences could be classified."]
        ranks = [r for r in self.SUMMARY_RANKS if self.assigned(r) > 0]
        name = lambda r: RANK_NAMES[r].ljust(11)
        out = []
        if self.unassigned() > 0:
            out.append(f"{comment}unclassified: {100 * self.unclassified_rate():g}% ({self.unassigned()})")
        out.append(f"{comment}classified:")
        out += [f"{comment}  {name(r)}{100 * self.classification_rate(r):g}% ({self.assigned(r)})" for r in ranks]
        if self.known() > 0:
            if self.unknown() > 0:
                out.append(f"{comment}ground truth unknown: {100 * self.unknown_rate():g}% ({self.unknown()})")
            out.append(f"{comment}ground truth known:")
            out += [f"{comment}  {name(r)}{100 * self.known_rate(r):g}% ({self.known(r)})" for r in ranks]
            out.append(f"{comment}correctly classified:")
            out += [f"{comment}  {name(r)}{self.correct(r)}" for r in ranks]
            out.append(f"{comment}precision (correctly classified / classified) if ground truth known:")
            out += [f"{comment}  {name(r)}{100 * self.precision(r):g}%" for r in ranks]
            out.append(f"{comment}sensitivity (correctly classified / all) if ground truth known:")
            out += [f"{comment}  {name(r)}{100 * self.sensitivity(r):g}%" for r in ranks]
            if self.coverage(19).total() > 0:
                out.append(f"{comment}false positives (hit on taxa not covered in DB):")
                out += [f"{comment}  {name(r)}{self.coverage(r).false_pos()}" for r in ranks]
        return out


class McDeviceResults(C.Structure):
    _fields_ = [("cands", C.c_void_p), ("hit_counts", C.c_void_p), ("hit_offsets", C.c_void_p), ("hits", C.c_void_p),
                ("features", C.c_void_p), ("win_offsets", C.c_void_p)]


EXPORTS = ["mc_candidates_from_partial_numbers_on", "mc_runtime_warning", "mc_slot_stats", "mc_config_default", "mc_create", "mc_destroy", "mc_last_error", "mc_load_begin", "mc_load_batch", "mc_load_end", "mc_load_location_range", "mc_load_target_windows", "mc_table_layout", "mc_target_range", "mc_merge_part_candidates", "mc_partset_open", "mc_partset_close",
           "mc_partset_info", "mc_partset_classify", "mc_partset_last_error", "mc_partset_select_group", "mc_partset_classify_resident", "mc_partset_load_bytes",
           "mc_partial_numbers", "mc_candidates_from_partial_numbers", "mc_owner_stats", "mc_keyset_open", "mc_keyset_close", "mc_keyset_info", "mc_keyset_classify", "mc_keyset_last_error",
           "mc_open_database", "mc_open_metadata", "mc_load_stats", "mc_set_lineages", "mc_db_info", "mc_db_num_taxa", "mc_db_taxon", "mc_db_taxon_source", "mc_db_lineages",
           "mc_batch_add", "mc_batch_add_bulk", "mc_batch_submit", "mc_batch_wait", "mc_batch_clear", "mc_query_device", "mc_query_finish", "mc_query_wait", "mc_synchronize",
           "mc_key_owner", "mc_candidates_from_hits", "mc_candidates_from_partial_hits", "mc_copy_results",
           "mc_timing_enable", "mc_timing_reset", "mc_timing_get", "mc_last_batch_stats", "mc_set_tuning", "mc_copy_results_on",
           "mc_build_begin", "mc_build_add_target", "mc_build_add_target_src", "mc_build_add_target_device", "mc_build_flush", "mc_build_reserve",
           "mc_build_table_begin", "mc_build_table_add", "mc_build_table_end", "mc_build_set_parent", "mc_build_target_windows", "mc_build_remove_ambiguous", "mc_build_counts", "mc_build_add_existing_target", "mc_build_add_locations", "mc_build_finish", "mc_build_finish_shards", "mc_build_write_shards", "mc_build_write", "mc_build_write_begin", "mc_build_write_add", "mc_build_write_end", "mc_build_free", "mc_build_last_error",
           "mc_build_set_query_config", "mc_align_semiglobal", "mc_align_stats",
           "mc_classify_options_default", "mc_classify_candidates", "mc_classify_tally",
           "mc_coverage_add", "mc_coverage_counts", "mc_coverage_keep", "mc_coverage_set_keep", "mc_coverage_drop",
           "mc_target_hits_reserve", "mc_target_hits_add", "mc_target_hits_collect",
           "mc_set_taxon_table", "mc_db_taxon_table", "mc_evaluate_assignments", "mc_evaluate_tally",
           "mc_format_set_text", "mc_format_mappings", "mc_format_stats",
           "mc_format_matches_set_text", "mc_format_matches", "mc_format_mappings_with", "mc_format_matches_stats",
           "mc_table_histogram", "mc_table_features", "mc_table_lookup",
           "mc_parse_records", "mc_parse_scratch_bytes", "mc_parse_stats", "mc_batch_add_file_bytes", "mc_batch_records",
           "mc_parse_mates", "mc_parse_mates_scratch_bytes", "mc_batch_add_file_mates",
           "mc_parse_cut", "mc_parse_cut_scratch_bytes", "mc_parse_headers", "mc_parse_headers_scratch_bytes", "mc_batch_add_device_bytes", "mc_batch_headers",
           "mc_parse_targets", "mc_parse_targets_scratch_bytes", "mc_buffer_alloc", "mc_buffer_free",
           "mc_input_open", "mc_input_batches", "mc_input_download", "mc_input_close",
           "mc_merge_results_set_taxids", "mc_merge_results_begin", "mc_merge_results_reserve", "mc_merge_results_scratch_bytes", "mc_merge_results_add",
           "mc_merge_results_lists", "mc_merge_results_classify", "mc_merge_results_stats", "mc_merge_results_end",
           "mc_bgzf_index", "mc_inflate_blocks", "mc_inflate_stats", "mc_gzip_hint", "mc_inflate_streams", "mc_inflate_streams_stats",
           "mc_taxmap_begin", "mc_taxmap_scratch_bytes", "mc_taxmap_add", "mc_taxmap_result", "mc_taxmap_stats", "mc_taxmap_end"]

_lib = None


def lib() -> C.CDLL:
    """Loads (building first if needed) libmetacache_amd.so.  Raises if that is impossible."""
    global _lib
    if _lib is None:
        # PyTorch's wheel bundles its own libamdhip64 / libhsa-runtime64.  Two HSA runtimes in one
        # process do not both see the GPU, so when torch is present it is imported FIRST and our
        # library then binds (by SONAME libamdhip64.so.7) to the runtime that is already loaded.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        path = os.environ.get("MC_AMD_LIB") or _build.build_library()   # (MC_AMD_LIB: another build of the library, for A/B measurements)
        L = C.CDLL(path)
        L.mc_last_error.restype = C.c_char_p
        L.mc_last_error.argtypes = [C.c_void_p]
        L.mc_create.argtypes = [C.POINTER(McConfig), C.POINTER(C.c_void_p)]
        L.mc_destroy.argtypes = [C.c_void_p]
        L.mc_destroy.restype = None
        L.mc_open_database.argtypes = [C.c_char_p, C.POINTER(McConfig), C.POINTER(C.c_void_p)]
        L.mc_load_begin.argtypes = [C.c_void_p, C.c_uint32, C.c_uint64, C.c_uint64]
        L.mc_load_batch.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_load_end.argtypes = [C.c_void_p, C.c_uint32]
        L.mc_load_location_range.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32]
        L.mc_load_target_windows.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_table_layout.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_target_range.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_set_lineages.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_db_info.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_db_num_taxa.argtypes = [C.c_void_p, C.POINTER(C.c_uint64)]
        L.mc_db_taxon.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint32),
                                  C.POINTER(C.c_char_p)]
        L.mc_db_lineages.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.mc_batch_add.argtypes = [C.c_void_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_char_p, C.c_uint32, C.c_uint32]
        L.mc_batch_add_bulk.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint64]
        L.mc_batch_add_bulk.restype = C.c_int64
        L.mc_batch_submit.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
        L.mc_batch_wait.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(McResults)]
        L.mc_batch_clear.argtypes = [C.c_void_p, C.c_uint32]
        L.mc_query_device.argtypes = [C.c_void_p, C.POINTER(McDeviceBatch), C.c_int, C.c_int, C.POINTER(McDeviceResults), C.c_void_p]
        L.mc_query_finish.argtypes = [C.c_void_p, C.c_int]
        L.mc_query_wait.argtypes = [C.c_void_p, C.c_int]
        L.mc_synchronize.argtypes = [C.c_void_p]
        L.mc_key_owner.argtypes = [C.c_uint32, C.c_uint32]
        L.mc_key_owner.restype = C.c_uint32
        L.mc_candidates_from_hits.argtypes = [C.c_void_p, C.POINTER(McDeviceHits), C.c_int, C.POINTER(McDeviceResults), C.c_void_p]
        L.mc_copy_results.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.mc_timing_enable.argtypes = [C.c_void_p, C.c_int]
        L.mc_timing_reset.argtypes = [C.c_void_p]
        L.mc_timing_get.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_double), C.POINTER(C.c_uint64)]
        L.mc_last_batch_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        L.mc_align_semiglobal.argtypes = [C.c_void_p] + [C.c_void_p] * 6 + [C.c_uint64] + [C.c_void_p] * 6 + [C.c_uint64, C.c_void_p]
        L.mc_align_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_classify_options_default.argtypes = [C.POINTER(McClassifyOptions)]
        L.mc_classify_options_default.restype = None
        L.mc_classify_candidates.argtypes = [C.c_void_p, C.POINTER(McClassifyOptions), C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.mc_classify_tally.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]
        L.mc_coverage_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int, C.c_void_p]
        L.mc_coverage_counts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_int]
        L.mc_coverage_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_float, C.c_void_p]
        L.mc_coverage_set_keep.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_coverage_drop.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.mc_target_hits_reserve.argtypes = [C.c_void_p, C.c_uint64]
        L.mc_target_hits_add.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int32, C.c_int, C.c_void_p]
        L.mc_target_hits_collect.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_void_p, C.c_int]
        L.mc_set_taxon_table.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_db_taxon_table.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.mc_evaluate_assignments.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
        L.mc_evaluate_tally.argtypes = [C.c_void_p, C.POINTER(McEvaluation), C.c_int]
        L.mc_format_set_text.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_format_mappings.argtypes = [C.c_void_p, C.POINTER(McFormatOptions), C.c_void_p, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64,
                                         C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mc_format_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_format_matches_set_text.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_format_matches.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mc_format_mappings_with.argtypes = L.mc_format_mappings.argtypes + [C.c_void_p, C.c_void_p]
        L.mc_format_matches_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_table_histogram.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_uint64)]
        L.mc_table_features.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64), C.c_int]
        L.mc_table_lookup.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int]
        L.mc_parse_scratch_bytes.argtypes = [C.c_uint64]
        L.mc_parse_scratch_bytes.restype = C.c_uint64
        L.mc_parse_records.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(McParseOutput), C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_parse_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_batch_add_file_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64]
        L.mc_batch_records.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(McBatchRecordInfo)]
        L.mc_parse_mates_scratch_bytes.argtypes = [C.c_uint64, C.c_uint64, C.c_uint32]
        L.mc_parse_mates_scratch_bytes.restype = C.c_uint64
        L.mc_parse_mates.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.POINTER(McParseOutput), C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_batch_add_file_mates.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_uint64]
        L.mc_parse_cut_scratch_bytes.argtypes = [C.c_uint64]
        L.mc_parse_cut_scratch_bytes.restype = C.c_uint64
        L.mc_parse_cut.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_parse_headers_scratch_bytes.argtypes = [C.c_uint32]
        L.mc_parse_headers_scratch_bytes.restype = C.c_uint64
        L.mc_parse_headers.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p,
                                       C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_parse_targets_scratch_bytes.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32]
        L.mc_parse_targets_scratch_bytes.restype = C.c_uint64
        L.mc_parse_targets.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint32, C.c_int, C.POINTER(McParseTargetsOutput), C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_batch_add_device_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64]
        L.mc_batch_headers.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.mc_input_open.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint32, C.c_uint64, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p), C.c_void_p]
        L.mc_input_batches.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
        L.mc_input_download.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_input_close.argtypes = [C.c_void_p]
        L.mc_input_close.restype = None
        L.mc_merge_results_set_taxids.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64]
        L.mc_merge_results_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint32, C.c_int32]
        L.mc_merge_results_reserve.argtypes = [C.c_void_p, C.c_uint64]
        L.mc_merge_results_scratch_bytes.argtypes = [C.c_uint64]
        L.mc_merge_results_scratch_bytes.restype = C.c_uint64
        L.mc_merge_results_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_merge_results_lists.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mc_merge_results_classify.argtypes = [C.c_void_p, C.POINTER(McClassifyOptions), C.c_int, C.c_uint64, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mc_merge_results_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_merge_results_end.argtypes = [C.c_void_p]
        L.mc_merge_results_end.restype = None
        L.mc_bgzf_index.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_inflate_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p]
        L.mc_inflate_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_gzip_hint.argtypes = [C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_inflate_streams.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mc_inflate_streams_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_taxmap_begin.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_taxmap_scratch_bytes.argtypes = [C.c_uint64]
        L.mc_taxmap_scratch_bytes.restype = C.c_uint64
        L.mc_taxmap_add.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p, C.c_void_p, C.c_uint64, C.c_void_p]
        L.mc_taxmap_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        L.mc_taxmap_stats.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_taxmap_end.argtypes = [C.c_void_p]
        L.mc_taxmap_end.restype = None
        if hasattr(L, "mc_build_begin"):
            L.mc_build_begin.argtypes = [C.POINTER(McConfig), C.POINTER(C.c_void_p)]
            L.mc_build_add_target.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int64, C.c_char_p]
            L.mc_build_finish.argtypes = [C.c_void_p, C.POINTER(C.c_void_p)]
            L.mc_build_write.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64]
            L.mc_build_free.argtypes = [C.c_void_p]
            L.mc_build_free.restype = None
        _lib = L
    return _lib


class McError(RuntimeError):
    pass


def table_statistics(hist, dead: int = 0, load_factor: float = 0.8) -> dict:
    """The statistics of `metacache info <db> statistics` (print_content_properties, printing.cpp:662-696) from the histogram of list
    sizes (Database.table_histogram; hist[s] = features with s locations): features, locations, max, mean, stddev, skewness, buckets.
    n = features, S1 = locations, S2 and S3 = the sums of the squared and cubed sizes are exact integers; the moments then follow the
    reference's arithmetic on doubles made from them (stat_moments.hpp:685-707, :836-854):
        cm2 = (S2 - S1 * S1 / n) / (n - 1), stddev = sqrt(cm2), cm3 = (n^2 * S3 - 3 * n * (S1 * S2) + 2 * (S1 * S1 * S1)) / (n * n^2),
        skewness = cm3 / pow(cm2, 1.5); both 0 for n < 2.
    buckets = what the reference's hash table of features + dead keys reserves (hash_multimap.hpp:552-554 with the database's default
    load factor 0.8): uint64(1.0f + float(features + dead) / 0.8f) in single precision.  Several parts: sum the histograms, and the
    parts' bucket counts.
    Above about 5 * 10^8 features the reference's own running double sums are no longer exact (S3 passes 2^53): its printed six digits are
    what this matches, not its last bit."""
    h = [int(x) for x in hist]
    n = sum(h)
    s1 = sum(s * c for s, c in enumerate(h))
    s2 = sum(s * s * c for s, c in enumerate(h))
    s3 = sum(s * s * s * c for s, c in enumerate(h))
    top = max((s for s, c in enumerate(h) if c), default=0)
    stddev = skewness = 0.0
    if n >= 2:
        dn, d1, d2, d3 = float(n), float(s1), float(s2), float(s3)
        cm2 = (d2 - d1 * d1 / dn) / (dn - 1.0)
        n2 = dn * dn
        cm3 = (n2 * d3 - 3.0 * dn * (d1 * d2) + 2.0 * (d1 * d1 * d1)) / (dn * n2)
        stddev = float(np.sqrt(cm2))
        skewness = float(cm3 / np.power(cm2, 1.5)) if cm2 > 0 else 0.0
    buckets = int(np.uint64(np.float32(1.0) + np.float32(n + int(dead)) / np.float32(load_factor)))
    return dict(features=n, locations=s1, max=top, mean=(float(s1) / float(n)) if n else 0.0, stddev=stddev, skewness=skewness, buckets=buckets)


def default_config(**kw) -> McConfig:
    cfg = McConfig()
    lib().mc_config_default(C.byref(cfg))
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _view(ptr, n, dtype):
    if not ptr or n == 0:
        return np.zeros(0, dtype=dtype)
    buf = (C.c_uint8 * (n * dtype.itemsize)).from_address(ptr)
    return np.frombuffer(buf, dtype=dtype, count=n)


class Database:
    """Host-side mirror of what the reference's `database` gives the query layer
    (database.hpp:386-408): open files, run batches, read results."""

    def __init__(self, handle, cfg: McConfig):
        self.h = C.c_void_p(handle)
        self.cfg = cfg
        self.refresh_info()

    def refresh_info(self):
        info = np.zeros(8, dtype=np.uint64)
        self._check(lib().mc_db_info(self.h, info.ctypes.data_as(C.c_void_p)))
        (self.k, self.s, self.w, self.stride, self.max_locs, self.n_targets, self.n_parts, self.n_locations) = map(int, info)

    # ---- construction ----------------------------------------------------------------------
    @classmethod
    def open(cls, name: str, **kw) -> "Database":
        kw.setdefault("kmerlen", 0); kw.setdefault("sketchlen", 0); kw.setdefault("winlen", 0); kw.setdefault("winstride", 0)
        cfg = default_config(**kw)
        h = C.c_void_p()
        rc = lib().mc_open_database(name.encode(), C.byref(cfg), C.byref(h))
        if rc != MC_OK:
            raise McError(f"mc_open_database({name}) -> {rc}: {lib().mc_last_error(None).decode()}")
        return cls(h.value, cfg)

    @classmethod
    def from_handle(cls, handle, cfg) -> "Database":
        return cls(handle, cfg)

    @classmethod
    def create(cls, **kw) -> "Database":
        """a context on the device without a database (mc_create): what the calls that need no table run on -- the parse calls among them"""
        cfg = default_config(**kw)
        h = C.c_void_p()
        rc = lib().mc_create(C.byref(cfg), C.byref(h))
        if rc != MC_OK:
            raise McError(f"mc_create -> {rc}: {lib().mc_last_error(None).decode()}")
        return cls(h.value, cfg)

    def close(self):
        if self.h:
            lib().mc_destroy(self.h)
            self.h = None

    def _check(self, rc):
        if rc < 0:
            raise McError(f"metacache_amd error {rc}: {lib().mc_last_error(self.h).decode()}")
        return rc

    def info(self):
        info = np.zeros(8, dtype=np.uint64)
        self._check(lib().mc_db_info(self.h, info.ctypes.data_as(C.c_void_p)))
        return list(map(int, info))

    def set_lineages(self, lin: np.ndarray):
        """lin[targets, 21] uint32: taxon index + 1 per rank, 0 = none (mc_set_lineages) -- needed for lowest > 0 on contexts that
        were not opened from database files"""
        lin = np.ascontiguousarray(lin, dtype=np.uint32)
        assert lin.ndim == 2 and lin.shape[1] == 21
        self._check(lib().mc_set_lineages(self.h, lin.ctypes.data_as(C.c_void_p), lin.shape[0]))

    # ---- taxonomy --------------------------------------------------------------------------
    def taxa(self):
        n = C.c_uint64()
        self._check(lib().mc_db_num_taxa(self.h, C.byref(n)))
        out = []
        for i in range(n.value):
            tid, par, rk, nm = C.c_int64(), C.c_int64(), C.c_uint32(), C.c_char_p()
            self._check(lib().mc_db_taxon(self.h, i, C.byref(tid), C.byref(par), C.byref(rk), C.byref(nm)))
            out.append((tid.value, par.value, rk.value, nm.value.decode()))
        return out

    def lineages(self) -> np.ndarray:
        p, n = C.c_void_p(), C.c_uint64()
        self._check(lib().mc_db_lineages(self.h, C.byref(p), C.byref(n)))
        return _view(p.value, n.value * NUM_RANKS, np.dtype("<u4")).reshape(n.value, NUM_RANKS).copy()

    def max_windows_in_range(self, l1: int, l2: int = 0, insert_max: int = 0) -> int:
        """candidate_structs.hpp:143-145 (stride = the database's window stride)"""
        return (2 + max(l1 + l2, insert_max) // self.stride) & 0xFFFFFFFF

    # ---- host slot path ---------------------------------------------------------------------
    def query(self, reads, mates=None, lowest: int = 0, insert_max: int = 0, slot: int = 0):
        """Runs all reads (bytes) through slot batches.
        -> (cands[n, K] cand_dtype, hit_counts[n], allhits list or None)"""
        L = lib()
        n = len(reads)
        K = self.cfg.max_candidates
        cands = np.zeros((n, K), dtype=cand_dtype)
        counts = np.zeros(n, dtype=np.uint32)
        allhits = [None] * n if self.cfg.copy_allhits else None
        start = 0

        def flush(upto):
            nonlocal start
            self._check(L.mc_batch_submit(self.h, slot, lowest))
            res = McResults()
            self._check(L.mc_batch_wait(self.h, slot, C.byref(res)))
            m = res.num_queries
            assert m == upto - start
            cands[start:upto] = _view(res.cands, m * K, cand_dtype).reshape(m, K)
            counts[start:upto] = _view(res.hit_counts, m, np.dtype("<u4"))
            if allhits is not None:
                off = _view(res.hit_offsets, m + 1, np.dtype("<u8"))
                hits = _view(res.hits, int(off[m]), loc_dtype)
                for i in range(m):
                    allhits[start + i] = hits[int(off[i]):int(off[i + 1])].copy()
            self._check(L.mc_batch_clear(self.h, slot))
            start = upto

        for i in range(n):
            a = bytes(reads[i]); b = bytes(mates[i]) if mates is not None else b""
            mw = self.max_windows_in_range(len(a), len(b), insert_max)
            rc = self._check(L.mc_batch_add(self.h, slot, a, len(a), b, len(b), mw))
            if rc == MC_BATCH_FULL:
                flush(i)
                rc = self._check(L.mc_batch_add(self.h, slot, a, len(a), b, len(b), mw))
                if rc != MC_OK:
                    raise McError("query does not fit an empty slot")
        flush(n)
        return cands, counts, allhits

    def query_bulk(self, seqs: np.ndarray, offs: np.ndarray, lowest: int = 0, insert_max: int = 0, slot: int = 0) -> np.ndarray:
        """single-end reads given as one byte array + offsets; host slot path (H2D of the characters, D2H of the
        candidates) -> cands[n, K]"""
        L = lib()
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8); offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        K = self.cfg.max_candidates
        out = np.zeros((n, K), dtype=cand_dtype)
        done = 0
        while done < n:
            added = L.mc_batch_add_bulk(self.h, slot, seqs.ctypes.data_as(C.c_void_p), offs[done:].ctypes.data_as(C.c_void_p), n - done, insert_max)
            self._check(added)
            if added == 0:
                raise McError("query does not fit an empty slot")
            self._check(L.mc_batch_submit(self.h, slot, lowest))
            res = McResults()
            self._check(L.mc_batch_wait(self.h, slot, C.byref(res)))
            out[done:done + added] = _view(res.cands, added * K, cand_dtype).reshape(added, K)
            self._check(L.mc_batch_clear(self.h, slot))
            done += added
        return out

    # ---- device path (pointers are device addresses, e.g. torch tensors' data_ptr()) ----------
    def query_device(self, seq_ptr: int, qinfo_ptr: int, n: int, num_chars: int, max_win_ptr: int = 0, max_win_uniform: int = 0,
                     lowest: int = 0, want_allhits: bool = False, want_features: bool = False,
                     stream: int = 0, want_partial_hits: bool = False, second_pipe: bool = False, want_partial_numbers: bool = False,
                     defer_tail: bool = False) -> McDeviceResults:
        b = McDeviceBatch(seq_ptr, qinfo_ptr, max_win_ptr or None, max_win_uniform, n, num_chars)
        r = McDeviceResults()
        self._check(lib().mc_query_device(self.h, C.byref(b), lowest, int(want_allhits) | (2 if want_features else 0) | (4 if want_partial_hits else 0) | (8 if second_pipe else 0) | (16 if want_partial_numbers else 0) | (32 if defer_tail else 0), C.byref(r),
                                          stream or None))
        return r

    def query_finish(self, second_pipe: bool = False):
        """the tail of the last query_device(defer_tail=True) call on that pipe (mc_query_finish)"""
        self._check(lib().mc_query_finish(self.h, 8 if second_pipe else 0))

    def query_wait(self, second_pipe: bool = False):
        """waits for ONE pipe's stream (mc_query_wait)"""
        self._check(lib().mc_query_wait(self.h, 8 if second_pipe else 0))

    def candidates_from_hits(self, hits_ptr: int, hit_offsets_ptr: int, n: int, max_win_ptr: int = 0, max_win_uniform: int = 0,
                             lowest: int = 0, stream: int = 0) -> McDeviceResults:
        """Mode K: rows 8-10 on gathered location lists (device pointers)"""
        h = McDeviceHits(hits_ptr, hit_offsets_ptr, max_win_ptr or None, max_win_uniform, n)
        r = McDeviceResults()
        self._check(lib().mc_candidates_from_hits(self.h, C.byref(h), lowest, C.byref(r), stream or None))
        return r

    def candidates_from_partial_hits(self, counts_ptr: int, hits_ptr: int, total_hits: int, n: int, sources: int, max_win_ptr: int = 0,
                                     max_win_uniform: int = 0, lowest: int = 0, stream: int = 0) -> McDeviceResults:
        """Mode K owner side: union of the sources' partial lists + rows 8-10, all on the device (mc_candidates_from_partial_hits)"""
        L = lib()
        L.mc_candidates_from_partial_hits.argtypes = [C.c_void_p, C.POINTER(McDevicePartialHits), C.c_int, C.POINTER(McDeviceResults), C.c_void_p]
        h = McDevicePartialHits(counts_ptr, hits_ptr or None, total_hits, max_win_ptr or None, max_win_uniform, n, sources)
        r = McDeviceResults()
        self._check(L.mc_candidates_from_partial_hits(self.h, C.byref(h), lowest, C.byref(r), stream or None))
        return r

    def partial_numbers(self, res: McDeviceResults, n: int, cut_queries, stream: int = 0):
        """Mode K shard side, 4-byte wire: the partial lists of the last query_device(want_partial_hits=True) as global window numbers
        (mc_partial_numbers).  -> (McDevicePartialNumbers, cut_offsets uint64 [len(cut_queries)])"""
        L = lib()
        L.mc_partial_numbers.argtypes = [C.c_void_p, C.POINTER(McDeviceResults), C.c_uint32, C.c_void_p, C.c_uint32, C.c_void_p, C.POINTER(McDevicePartialNumbers), C.c_void_p]
        cq = np.ascontiguousarray(cut_queries, dtype=np.uint32)
        co = np.zeros(len(cq), dtype=np.uint64)
        out = McDevicePartialNumbers()
        self._check(L.mc_partial_numbers(self.h, C.byref(res), n, cq.ctypes.data, len(cq), co.ctypes.data, C.byref(out), stream or None))
        return out, co

    def candidates_from_partial_numbers(self, counts_ptr: int, numbers_ptr: int, source_offsets, n: int, max_win_ptr: int = 0,
                                        max_win_uniform: int = 0, lowest: int = 0, stream: int = 0) -> McDeviceResults:
        """Mode K owner side, 4-byte wire (mc_candidates_from_partial_numbers); source_offsets: host array [sources + 1]"""
        L = lib()
        L.mc_candidates_from_partial_numbers.argtypes = [C.c_void_p, C.POINTER(McDevicePartialNumbersIn), C.c_int, C.POINTER(McDeviceResults), C.c_void_p]
        so = np.ascontiguousarray(source_offsets, dtype=np.uint64)
        h = McDevicePartialNumbersIn(counts_ptr, numbers_ptr or None, so.ctypes.data, max_win_ptr or None, max_win_uniform, n, len(so) - 1)
        r = McDeviceResults()
        self._check(L.mc_candidates_from_partial_numbers(self.h, C.byref(h), lowest, C.byref(r), stream or None))
        return r

    # ---- classification: one taxon per read (mc_classify_*) ----------------------------------------
    def classify_device(self, cands_ptr: int, n: int, stride: int, *, hitmin: int = 0, hitdiff: float = 1.0, lowest: int = 0,
                        highest: int = NUM_RANKS - 1, tally: bool = False, out_ptr: int, stream: int = 0):
        """the ranked-LCA vote on candidate lists in device memory (cands_ptr: n x stride mc_candidate) -> n mc_assignment at out_ptr
        (8 bytes each: assignment_dtype); asynchronous on `stream` (0 = the context's).  hitdiff as on the command line: above 1 = percent"""
        o = classify_options(hitmin, hitdiff, lowest, highest)
        self._check(lib().mc_classify_candidates(self.h, C.byref(o), cands_ptr or None, n, stride, CLASSIFY_TALLY if tally else 0,
                                                 out_ptr or None, stream or None))

    def classify_candidates(self, cands: np.ndarray, *, hitmin: int = 0, hitdiff: float = 1.0, lowest: int = 0, highest: int = NUM_RANKS - 1,
                            tally: bool = False) -> np.ndarray:
        """the same on a host array cands[n, stride] (cand_dtype, e.g. what query() returns) -> assignment_dtype [n]: taxon (index + 1
        as in lineages(), 0 = unclassified), rank (21 = unclassified), voters"""
        cands = np.ascontiguousarray(cands, dtype=cand_dtype)
        if cands.ndim != 2:
            raise ValueError("classify_candidates: cands must be [n, stride]")
        n, stride = cands.shape
        out = np.zeros(n, dtype=assignment_dtype)
        o = classify_options(hitmin, hitdiff, lowest, highest)
        self._check(lib().mc_classify_candidates(self.h, C.byref(o), cands.ctypes.data if n else None, n, stride,
                                                 CLASSIFY_HOST | (CLASSIFY_TALLY if tally else 0), out.ctypes.data if n else None, None))
        return out

    def classify(self, reads, mates=None, *, hitmin: int = 0, hitdiff: float = 1.0, lowest: int = 0, highest: int = NUM_RANKS - 1,
                 insert_max: int = 0, tally: bool = False) -> np.ndarray:
        """query() followed by classify_candidates(): one assignment per read (pair)"""
        cands, _, _ = self.query(reads, mates, lowest=lowest, insert_max=insert_max)
        return self.classify_candidates(cands, hitmin=hitmin, hitdiff=hitdiff, lowest=lowest, highest=highest, tally=tally)

    def tally(self, reset: bool = False):
        """the counts of all classify calls with tally=True since the last reset -> (assigned[22] uint64: reads per result rank,
        [21] = unclassified; taxon_counts uint64: reads per taxon, index = taxon index + 1)"""
        L = lib()
        num = C.c_uint64()
        self._check(L.mc_classify_tally(self.h, None, None, 0, C.byref(num), 0))
        assigned = np.zeros(NUM_RANKS + 1, dtype=np.uint64)
        counts = np.zeros(num.value, dtype=np.uint64)
        self._check(L.mc_classify_tally(self.h, assigned.ctypes.data, counts.ctypes.data, counts.size, None, int(reset)))
        return assigned, counts

    # ---- evaluation against a ground truth: -precision / -taxon-coverage (mc_evaluate_*) ------------
    def set_taxon_table(self, lin: np.ndarray, rank=None, covered=None):
        """lin[taxa, 21] uint32: every taxon's ranked lineage as taxon index + 1 (0 = none); rank[taxa] uint8 (21 = none; None: derived
        from the rows); covered[taxa] uint8 (None: no -taxon-coverage counters) -- for contexts that were not opened from database files"""
        lin = np.ascontiguousarray(lin, dtype=np.uint32)
        if lin.ndim != 2 or lin.shape[1] != NUM_RANKS:
            raise ValueError("set_taxon_table: lin must be [taxa, 21]")
        rank = None if rank is None else np.ascontiguousarray(rank, dtype=np.uint8)
        covered = None if covered is None else np.ascontiguousarray(covered, dtype=np.uint8)
        if any(x is not None and x.shape != (lin.shape[0],) for x in (rank, covered)):
            raise ValueError("set_taxon_table: rank and covered have one entry per taxon")
        self._check(lib().mc_set_taxon_table(self.h, lin.ctypes.data, None if rank is None else rank.ctypes.data,
                                             None if covered is None else covered.ctypes.data, lin.shape[0]))

    def taxon_table(self):
        """-> (lin[taxa, 21] uint32, rank[taxa] uint8, covered[taxa] uint8 or None): copies of the context's taxon table"""
        pl, pr, pc, n = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(lib().mc_db_taxon_table(self.h, C.byref(pl), C.byref(pr), C.byref(pc), C.byref(n)))
        lin = _view(pl.value, n.value * NUM_RANKS, np.dtype("<u4")).reshape(n.value, NUM_RANKS).copy()
        return lin, _view(pr.value, n.value, np.dtype("u1")).copy(), (_view(pc.value, n.value, np.dtype("u1")).copy() if pc.value else None)

    def evaluate_device(self, assigned_ptr: int, truth_ptr: int, n: int, *, tally: bool = True, coverage: bool = False, verdicts_ptr: int = 0,
                        stream: int = 0):
        """judges n assignments in device memory (mc_assignment, 8 bytes each) by the truths at truth_ptr (uint32: taxon index + 1,
        0 = unknown) -> n mc_verdict at verdicts_ptr (4 bytes each, 0 = none wanted) and / or the context's evaluation tallies;
        asynchronous on `stream` (0 = the context's)"""
        flags = (EVALUATE_TALLY if tally else 0) | (EVALUATE_COVERAGE if coverage else 0)
        self._check(lib().mc_evaluate_assignments(self.h, assigned_ptr or None, truth_ptr or None, n, flags, verdicts_ptr or None, stream or None))

    def evaluate(self, assigned: np.ndarray, truth: np.ndarray, *, tally: bool = True, coverage: bool = False) -> np.ndarray:
        """the same on host arrays: assigned[n] (assignment_dtype, e.g. what classify() returns), truth[n] uint32 -> verdict_dtype [n]"""
        assigned = np.ascontiguousarray(assigned, dtype=assignment_dtype)
        truth = np.ascontiguousarray(truth, dtype=np.uint32)
        if assigned.ndim != 1 or truth.shape != assigned.shape:
            raise ValueError("evaluate: assigned and truth must be one-dimensional and of one length")
        n = len(truth)
        out = np.zeros(n, dtype=verdict_dtype)
        flags = EVALUATE_HOST | (EVALUATE_TALLY if tally else 0) | (EVALUATE_COVERAGE if coverage else 0)
        self._check(lib().mc_evaluate_assignments(self.h, assigned.ctypes.data if n else None, truth.ctypes.data if n else None, n, flags,
                                                  out.ctypes.data, None))
        return out

    def evaluation(self, reset: bool = False) -> Evaluation:
        """the tallies of all evaluate calls with tally=True since the last reset (mc_evaluate_tally)"""
        e = McEvaluation()
        self._check(lib().mc_evaluate_tally(self.h, C.byref(e), int(reset)))
        return Evaluation(list(e.assigned), list(e.known), list(e.correct), list(e.wrong), [list(row) for row in e.coverage], e.reads, e.out_of_table)

    # ---- mapping lines: the per-read output of the command line (mc_format_*) ------------------------
    def format_set_text(self, which: int, strings):
        """one of the three string tables (TEXT_RESULT, TEXT_TARGET_RESULT, TEXT_CANDIDATE): a list of bytes, e.g. from mapping_texts()"""
        data, off = pack_strings([bytes(x) for x in strings])
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        self._check(lib().mc_format_set_text(self.h, which, buf.ctypes.data, off.ctypes.data, len(off) - 1))

    def format_device(self, opt: McFormatOptions, cands_ptr: int, stride: int, assigned_ptr: int, names_ptr: int, name_off_ptr: int, n: int, *,
                      flags: int = 0, truth_ptr: int = 0, query_ids_ptr: int = 0, first_query_id: int = 0, out_ptr: int, out_capacity: int,
                      line_off_ptr: int, stream: int = 0, extra_ptr: int = 0, extra_off_ptr: int = 0, with_extra: bool = False):
        """renders n mapping lines from arrays in device memory into out_ptr (16-byte aligned); line_off_ptr: n + 1 + FORMAT_SCRATCH
        uint64, entry n = the bytes all lines need (more than out_capacity: nothing was written); asynchronous on `stream`.
        extra_ptr / extra_off_ptr (or with_extra): through mc_format_mappings_with -- one more column, piece i of extra, behind the truth column"""
        args = (self.h, C.byref(opt), cands_ptr or None, stride, assigned_ptr or None, truth_ptr or None,
                query_ids_ptr or None, first_query_id, names_ptr or None, name_off_ptr or None, n, flags,
                out_ptr or None, out_capacity, line_off_ptr or None, stream or None)
        if extra_ptr or extra_off_ptr or with_extra:
            self._check(lib().mc_format_mappings_with(*args, extra_ptr or None, extra_off_ptr or None))
        else:
            self._check(lib().mc_format_mappings(*args))

    def format_mappings(self, opt: McFormatOptions, cands: np.ndarray, assigned: np.ndarray, names, *, flags: int = 0, truth=None,
                        query_ids=None, first_query_id: int = 0, extra=None, extra_off=None):
        """the same on host arrays: cands[n, stride] (cand_dtype), assigned[n] (assignment_dtype), names: n bytes objects
        -> (bytes: all lines, line_off uint64 [n + 1]).  extra (bytes) / extra_off (uint64 [n + 1]): one more column behind the truth
        column, e.g. what format_matches returned (mc_format_mappings_with)"""
        cands = np.ascontiguousarray(cands, dtype=cand_dtype)
        assigned = np.ascontiguousarray(assigned, dtype=assignment_dtype)
        if cands.ndim != 2 or assigned.shape != (cands.shape[0],) or len(names) != cands.shape[0]:
            raise ValueError("format_mappings: cands must be [n, stride], assigned and names of length n")
        n, stride = cands.shape
        nbytes, noff = pack_strings([bytes(x) for x in names])
        nbuf = np.frombuffer(nbytes, dtype=np.uint8) if nbytes else np.zeros(1, dtype=np.uint8)
        tr = None if truth is None else np.ascontiguousarray(truth, dtype=np.uint32)
        ids = None if query_ids is None else np.ascontiguousarray(query_ids, dtype=np.uint64)
        line_off = np.zeros(n + 1, dtype=np.uint64)
        args = lambda out, cap: (self.h, C.byref(opt), cands.ctypes.data if n else None, stride, assigned.ctypes.data if n else None,
                                 None if tr is None else tr.ctypes.data, None if ids is None else ids.ctypes.data, first_query_id,
                                 nbuf.ctypes.data, noff.ctypes.data, n, flags | FORMAT_HOST, out, cap, line_off.ctypes.data, None)
        call = lib().mc_format_mappings
        if extra is not None:
            xoff = np.ascontiguousarray(extra_off, dtype=np.uint64)
            if xoff.shape != (n + 1,):
                raise ValueError("format_mappings: extra_off must have n + 1 entries")
            xbuf = np.frombuffer(bytes(extra) or b"\0", dtype=np.uint8)
            call = lambda *a: lib().mc_format_mappings_with(*a, xbuf.ctypes.data, xoff.ctypes.data)
        rc = call(*args(None, 0))                                           # the size first: line_off is complete either way
        if rc != -3:
            self._check(rc)
        total = int(line_off[n])
        out = np.zeros(max(total, 1), dtype=np.uint8)
        if total:
            self._check(call(*args(out.ctypes.data, total)))
        return out[:total].tobytes(), line_off

    def format_stats(self):
        """-> [mc_format_mappings calls, reads, lines written, bytes written, result indices beyond their table]"""
        st = np.zeros(5, dtype=np.uint64)
        self._check(lib().mc_format_stats(self.h, st.ctypes.data))
        return [int(x) for x in st]

    # ---- reads out of a FASTA / FASTQ byte range (mc_parse_*) -----------------------------------------
    def parse_device(self, bytes_ptr: int, nbytes: int, *, hdr_ptr: int, qinfo_ptr: int, seq_ptr: int, seq_capacity: int, names_ptr: int,
                     names_capacity: int, name_off_ptr: int, max_win_ptr: int, status_ptr: int, max_records: int, workspace_ptr: int,
                     workspace_bytes: int, pairs: bool = False, insert_max: int = 0, stream: int = 0):
        """cuts the range at bytes_ptr (device memory, 16-byte aligned) into reads: hdr [max_records, 2] uint32, qinfo [max_records, 4]
        uint32, seq, names, name_off [max_records + 1] uint64, max_win [max_records] uint32, status [8] uint64 -- all device memory;
        workspace of parse_scratch_bytes(nbytes); asynchronous on `stream`.  status[4] is the verdict (PARSE_OK: the arrays are filled)"""
        o = McParseOutput(hdr_ptr or None, qinfo_ptr or None, seq_ptr or None, seq_capacity, names_ptr or None, names_capacity,
                          name_off_ptr or None, max_win_ptr or None, status_ptr or None, max_records)
        self._check(lib().mc_parse_records(self.h, bytes_ptr or None, nbytes, PARSE_PAIRS if pairs else 0, insert_max, C.byref(o),
                                           workspace_ptr or None, workspace_bytes, stream or None))

    def parse_records(self, data, pairs: bool = False, insert_max: int = 0, *, max_records=None, seq_capacity=None, names_capacity=None):
        """the same on host memory: data (bytes) -> dict(status uint64 [8], and with the verdict PARSE_OK: hdr [records, 2], qinfo
        [queries, 4], seq (bytes, with the 16 behind the last read), names (bytes), name_off [queries + 1], max_win [queries]).
        Capacities that are left out are taken from a first call's status (PARSE_OVERFLOW reports what is needed).  "raw": the arrays as the
        last call left them, at their capacities (with another verdict than PARSE_OK: untouched)."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        status = np.zeros(8, dtype=np.uint64)

        def run(mr, sc, nc):
            a = dict(hdr=np.zeros((max(mr, 1), 2), dtype=np.uint32), qinfo=np.zeros((max(mr, 1), 4), dtype=np.uint32), seq=np.zeros(max(sc, 1), dtype=np.uint8),
                     names=np.zeros(max(nc, 1), dtype=np.uint8), name_off=np.zeros(mr + 1, dtype=np.uint64), max_win=np.zeros(max(mr, 1), dtype=np.uint32))
            o = McParseOutput(a["hdr"].ctypes.data, a["qinfo"].ctypes.data, a["seq"].ctypes.data, sc, a["names"].ctypes.data, nc,
                              a["name_off"].ctypes.data, a["max_win"].ctypes.data, status.ctypes.data, mr)
            self._check(lib().mc_parse_records(self.h, buf.ctypes.data if len(buf) else None, len(buf), PARSE_HOST | (PARSE_PAIRS if pairs else 0),
                                               insert_max, C.byref(o), None, 0, None))
            return a

        sized = max_records is not None and seq_capacity is not None and names_capacity is not None
        a = run(max_records or 0, seq_capacity or 0, names_capacity or 0)
        if not sized and int(status[4]) == PARSE_OVERFLOW:
            a = run(int(status[0]) if max_records is None else max_records, int(status[2]) if seq_capacity is None else seq_capacity,
                    int(status[3]) if names_capacity is None else names_capacity)
        out = dict(status=status.copy())
        if int(status[4]) == PARSE_OK:
            r, q = int(status[0]), int(status[1])
            out.update(hdr=a["hdr"][:r].copy(), qinfo=a["qinfo"][:q].copy(), seq=a["seq"][:int(status[2])].tobytes(), names=a["names"][:int(status[3])].tobytes(),
                       name_off=a["name_off"][:q + 1].copy(), max_win=a["max_win"][:q].copy())
        out["raw"] = a
        return out

    def parse_mates_device(self, bytes1_ptr: int, n1: int, bytes2_ptr: int, n2: int, *, hdr_ptr: int, qinfo_ptr: int, seq_ptr: int, seq_capacity: int,
                           names_ptr: int, names_capacity: int, name_off_ptr: int, max_win_ptr: int, status_ptr: int, max_records: int,
                           workspace_ptr: int, workspace_bytes: int, insert_max: int = 0, stream: int = 0, flags: int = 0):
        """cuts two ranges of mates (device memory, 16-byte aligned; query q = record q of each) into pairs, as parse_device does one range;
        status [10] uint64; workspace of parse_mates_scratch_bytes(n1, n2, max_records); asynchronous on `stream` (mc_parse_mates)"""
        o = McParseOutput(hdr_ptr or None, qinfo_ptr or None, seq_ptr or None, seq_capacity, names_ptr or None, names_capacity,
                          name_off_ptr or None, max_win_ptr or None, status_ptr or None, max_records)
        self._check(lib().mc_parse_mates(self.h, bytes1_ptr or None, n1, bytes2_ptr or None, n2, flags, insert_max, C.byref(o),
                                         workspace_ptr or None, workspace_bytes, stream or None))

    def parse_mates(self, data1, data2, insert_max: int = 0, *, max_records=None, seq_capacity=None, names_capacity=None):
        """the same on host memory: data1, data2 (bytes) -> dict(status uint64 [10], and with the verdict PARSE_OK the arrays of
        parse_records(pairs=True), hdr rows 2q / 2q + 1 being places in data1 / data2).  Capacities that are left out are taken from a
        first call's status.  "raw": the arrays as the last call left them."""
        b1, b2 = np.frombuffer(bytes(data1), dtype=np.uint8), np.frombuffer(bytes(data2), dtype=np.uint8)
        status = np.zeros(10, dtype=np.uint64)

        def run(mr, sc, nc):
            a = dict(hdr=np.zeros((max(mr, 1), 2), dtype=np.uint32), qinfo=np.zeros((max(mr, 1), 4), dtype=np.uint32), seq=np.zeros(max(sc, 1), dtype=np.uint8),
                     names=np.zeros(max(nc, 1), dtype=np.uint8), name_off=np.zeros(mr + 1, dtype=np.uint64), max_win=np.zeros(max(mr, 1), dtype=np.uint32))
            o = McParseOutput(a["hdr"].ctypes.data, a["qinfo"].ctypes.data, a["seq"].ctypes.data, sc, a["names"].ctypes.data, nc,
                              a["name_off"].ctypes.data, a["max_win"].ctypes.data, status.ctypes.data, mr)
            self._check(lib().mc_parse_mates(self.h, b1.ctypes.data if len(b1) else None, len(b1), b2.ctypes.data if len(b2) else None, len(b2),
                                             PARSE_HOST, insert_max, C.byref(o), None, 0, None))
            return a

        sized = max_records is not None and seq_capacity is not None and names_capacity is not None
        a = run(max_records or 0, seq_capacity or 0, names_capacity or 0)
        if not sized and int(status[4]) == PARSE_OVERFLOW:
            a = run(int(status[0]) if max_records is None else max_records, int(status[2]) if seq_capacity is None else seq_capacity,
                    int(status[3]) if names_capacity is None else names_capacity)
        out = dict(status=status.copy())
        if int(status[4]) == PARSE_OK:
            r, q = int(status[0]), int(status[1])
            out.update(hdr=a["hdr"][:r].copy(), qinfo=a["qinfo"][:q].copy(), seq=a["seq"][:int(status[2])].tobytes(), names=a["names"][:int(status[3])].tobytes(),
                       name_off=a["name_off"][:q + 1].copy(), max_win=a["max_win"][:q].copy())
        out["raw"] = a
        return out

    def batch_records(self, slot: int = 0) -> dict:
        """what the device made of a raw slot (mc_batch_records, after the wait): verdict, offence, records, queries, half_pair, and copies
        of hdr [records, 2] and qinfo [queries, 4] (empty with another verdict than PARSE_OK)"""
        info = McBatchRecordInfo()
        self._check(lib().mc_batch_records(self.h, slot, C.byref(info)))
        return dict(verdict=info.verdict, offence=info.offence, records=info.records, queries=info.queries, half_pair=info.half_pair,
                    hdr=_view(info.hdr, 2 * info.records, np.dtype("<u4")).reshape(info.records, 2).copy(),
                    qinfo=_view(info.qinfo, 4 * info.queries, np.dtype("<u4")).reshape(info.queries, 4).copy())

    def query_file_bytes(self, data, pairs: bool = False, lowest: int = 0, insert_max: int = 0, slot: int = 0):
        """one slot batch from a byte range of a FASTA / FASTQ file, cut into reads on the device (mc_batch_add_file_bytes)
        -> (cands[n, K], hit_counts[n], allhits list or None, records: batch_records()); n = 0 where the device refused the range
        (records["verdict"] says why) -- the caller then cuts that batch itself.  Raises McError("... does not fit ...") on MC_BATCH_FULL."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rc = self._check(lib().mc_batch_add_file_bytes(self.h, slot, buf.ctypes.data if len(buf) else None, len(buf), PARSE_PAIRS if pairs else 0, insert_max))
        return self._query_raw_slot(rc, lowest, slot)

    def query_file_mates(self, data1, data2, lowest: int = 0, insert_max: int = 0, slot: int = 0):
        """one slot batch from the byte ranges of two mate files (query q = record q of each), cut on the device (mc_batch_add_file_mates)
        -> as query_file_bytes; records["hdr"] rows 2q / 2q + 1 are places in data1 / data2"""
        b1, b2 = np.frombuffer(bytes(data1), dtype=np.uint8), np.frombuffer(bytes(data2), dtype=np.uint8)
        rc = self._check(lib().mc_batch_add_file_mates(self.h, slot, b1.ctypes.data if len(b1) else None, len(b1), b2.ctypes.data if len(b2) else None, len(b2), insert_max))
        return self._query_raw_slot(rc, lowest, slot)

    def _query_raw_slot(self, rc: int, lowest: int, slot: int, headers: bool = False):
        L = lib()
        if rc == MC_BATCH_FULL:
            raise McError("the byte range does not fit the slot's character capacity")
        K = self.cfg.max_candidates
        try:
            self._check(L.mc_batch_submit(self.h, slot, lowest))
            res = McResults()
            self._check(L.mc_batch_wait(self.h, slot, C.byref(res)))
            m = res.num_queries
            cands = _view(res.cands, m * K, cand_dtype).reshape(m, K).copy()
            counts = _view(res.hit_counts, m, np.dtype("<u4")).copy()
            allhits = None
            if self.cfg.copy_allhits:
                off = _view(res.hit_offsets, m + 1, np.dtype("<u8")) if m else np.zeros(1, dtype=np.uint64)
                hits = _view(res.hits, int(off[m]), loc_dtype)
                allhits = [hits[int(off[i]):int(off[i + 1])].copy() for i in range(m)]
            records = self.batch_records(slot)
            if headers:
                records["headers"] = self.batch_headers(slot)
        finally:
            self._check(L.mc_batch_clear(self.h, slot))
        return cands, counts, allhits, records

    # ---- batch borders of a FASTA / FASTQ range, the headers of a parsed one, slots that take device bytes -----------
    def parse_cut_device(self, bytes_ptr: int, nbytes: int, records_per_batch: int, *, cuts_ptr: int, capacity: int, status_ptr: int, workspace_ptr: int,
                         workspace_bytes: int, pairs: bool = False, open: bool = False, stream: int = 0):
        """the batch borders of the range at bytes_ptr (device memory, ANY address): cuts [capacity] uint64, status [8] uint64 -- device memory;
        workspace of parse_cut_scratch_bytes(nbytes); asynchronous on `stream` (mc_parse_cut).  status[4] is the verdict"""
        flags = (PARSE_PAIRS if pairs else 0) | (CUT_OPEN if open else 0)
        self._check(lib().mc_parse_cut(self.h, bytes_ptr or None, nbytes, records_per_batch, flags, cuts_ptr or None, capacity, status_ptr or None,
                                       workspace_ptr or None, workspace_bytes, stream or None))

    def parse_cut(self, data, records_per_batch: int, pairs: bool = False, open: bool = False, capacity=None):
        """the same on host memory: data (bytes) -> dict(status uint64 [8] = whole, nb, consumed, record starts seen, verdict, offence, the
        largest batch in bytes, half pair; and with the verdict PARSE_OK: cuts uint64 [nb + 1]).  A capacity that is left out is taken from a
        first call's status (PARSE_OVERFLOW reports nb).  "raw": cuts as the last call left it, at its capacity."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        status = np.zeros(8, dtype=np.uint64)
        flags = PARSE_HOST | (PARSE_PAIRS if pairs else 0) | (CUT_OPEN if open else 0)

        def run(cap):
            cuts = np.zeros(max(cap, 1), dtype=np.uint64)
            self._check(lib().mc_parse_cut(self.h, buf.ctypes.data if len(buf) else None, len(buf), records_per_batch, flags, cuts.ctypes.data, cap,
                                           status.ctypes.data, None, 0, None))
            return cuts

        cuts = run(1 if capacity is None else capacity)
        if capacity is None and int(status[4]) == PARSE_OVERFLOW:
            cuts = run(int(status[1]) + 1)
        out = dict(status=status.copy(), raw=cuts)
        if int(status[4]) == PARSE_OK:
            out["cuts"] = cuts[:int(status[1]) + 1].copy()
        return out

    def parse_headers_device(self, bytes_ptr: int, nbytes: int, *, hdr_ptr: int, parse_status_ptr: int, max_records: int, out_ptr: int, out_capacity: int,
                             out_off_ptr: int, status_ptr: int, workspace_ptr: int, workspace_bytes: int, stream: int = 0):
        """packs the headers of the range at bytes_ptr that parse_device has cut (hdr, parse_status: what it left) into out, with out_off
        [max_records + 1] uint64 and status [4] uint64 -- all device memory; workspace of parse_headers_scratch_bytes(max_records);
        asynchronous on `stream`, behind the parse (mc_parse_headers).  status[2] is the verdict"""
        self._check(lib().mc_parse_headers(self.h, bytes_ptr or None, nbytes, hdr_ptr or None, parse_status_ptr or None, max_records, 0, out_ptr or None,
                                           out_capacity, out_off_ptr or None, status_ptr or None, workspace_ptr or None, workspace_bytes, stream or None))

    def parse_headers(self, data, hdr, parse_status, *, max_records=None, out_capacity=None):
        """the same on host memory: data (bytes), hdr [records, 2] uint32 and parse_status [8] uint64 as parse_records gives them -> dict(status
        uint64 [4] = records, bytes needed, verdict, 0; and with the verdict PARSE_OK: out (bytes), out_off uint64 [records + 1]).  "raw":
        (out, out_off) as the call left them, at their capacities."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        hdr = np.ascontiguousarray(hdr, dtype=np.uint32).reshape(-1, 2)
        ps = np.ascontiguousarray(parse_status, dtype=np.uint64)
        mr = len(hdr) if max_records is None else max_records
        cap = len(buf) if out_capacity is None else out_capacity
        out, off, status = np.zeros(max(cap, 1), dtype=np.uint8), np.zeros(mr + 1, dtype=np.uint64), np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_parse_headers(self.h, buf.ctypes.data if len(buf) else None, len(buf), hdr.ctypes.data if mr else None, ps.ctypes.data, mr, PARSE_HOST,
                                           out.ctypes.data if cap else None, cap, off.ctypes.data, status.ctypes.data, None, 0, None))
        res = dict(status=status, raw=(out, off))
        if int(status[2]) == PARSE_OK:
            res.update(out=out[:int(status[1])].tobytes(), out_off=off[:int(status[0]) + 1].copy())
        return res

    # ---- targets out of many FASTA files in one range: the input side of a build -------------------------------------
    def parse_targets_device(self, bytes_ptr: int, nbytes: int, file_off_ptr: int, num_files: int, *, hdr_ptr: int, targets_ptr: int, seq_ptr: int,
                             seq_capacity: int, status_ptr: int, max_records: int, workspace_ptr: int, workspace_bytes: int, stream: int = 0):
        """(device ADDRESSES as integers -- a torch tensor's data_ptr() --, as every *_device method of this class takes them)
        cuts the range at bytes_ptr (device memory, 16-byte aligned), whose files begin at the uint64 offsets at file_off_ptr [num_files + 1],
        into targets: hdr [max_records, 2] uint32, targets [max_records] parse_target_dtype, seq, status [8] uint64 -- all device memory;
        workspace of parse_targets_scratch_bytes(nbytes, num_files, max_records); asynchronous on `stream` (mc_parse_targets).  status[4] is
        the verdict (PARSE_OK: the arrays are filled)"""
        o = McParseTargetsOutput(hdr_ptr or None, targets_ptr or None, seq_ptr or None, seq_capacity, status_ptr or None, max_records)
        self._check(lib().mc_parse_targets(self.h, bytes_ptr or None, nbytes, file_off_ptr or None, num_files, 0, C.byref(o), workspace_ptr or None,
                                           workspace_bytes, stream or None))

    def parse_targets(self, data, file_off, *, max_records=None, seq_capacity=None):
        """the same on host memory: data (bytes), file_off [files + 1] -> dict(status uint64 [8], and with the verdict PARSE_OK: hdr
        [records, 2], targets [records] parse_target_dtype, seq (bytes, with the 16 behind the last sequence)).  Capacities that are left
        out are taken from a first call's status (PARSE_OVERFLOW reports what is needed).  "raw": the arrays as the last call left them."""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        off = np.ascontiguousarray(file_off, dtype=np.uint64)
        status = np.zeros(8, dtype=np.uint64)

        def run(mr, sc):
            a = dict(hdr=np.zeros((max(mr, 1), 2), dtype=np.uint32), targets=np.zeros(max(mr, 1), dtype=parse_target_dtype), seq=np.zeros(max(sc, 1), dtype=np.uint8))
            o = McParseTargetsOutput(a["hdr"].ctypes.data, a["targets"].ctypes.data, a["seq"].ctypes.data, sc, status.ctypes.data, mr)
            self._check(lib().mc_parse_targets(self.h, buf.ctypes.data if len(buf) else None, len(buf), off.ctypes.data if len(off) else None, max(len(off), 1) - 1,
                                               PARSE_HOST, C.byref(o), None, 0, None))
            return a

        sized = max_records is not None and seq_capacity is not None
        a = run(max_records or 0, seq_capacity or 0)
        if not sized and int(status[4]) == PARSE_OVERFLOW:
            a = run(int(status[0]) if max_records is None else max_records, int(status[2]) if seq_capacity is None else seq_capacity)
        out = dict(status=status.copy())
        if int(status[4]) == PARSE_OK:
            r = int(status[0])
            out.update(hdr=a["hdr"][:r].copy(), targets=a["targets"][:r].copy(), seq=a["seq"][:int(status[2])].tobytes())
        out["raw"] = a
        return out

    def batch_headers(self, slot: int = 0):
        """the headers of a slot that was filled with device bytes (mc_batch_headers, after the wait) -> [bytes] per record; None with another
        verdict than PARSE_OK"""
        text, off, n = C.c_void_p(), C.c_void_p(), C.c_uint64()
        self._check(lib().mc_batch_headers(self.h, slot, C.byref(text), C.byref(off), C.byref(n)))
        if not off.value:
            return None
        o = _view(off.value, n.value + 1, np.dtype("<u8"))
        total = int(o[n.value])
        t = _view(text.value, total, np.dtype("u1")).tobytes()
        return [t[int(o[r]):int(o[r + 1])] for r in range(n.value)]

    def query_device_bytes(self, ptr: int, nbytes: int, pairs: bool = False, lowest: int = 0, insert_max: int = 0, slot: int = 0):
        """one slot batch from a byte range of a FASTA / FASTQ file that lies in device memory at ptr (any address; mc_batch_add_device_bytes)
        -> (cands, hit_counts, allhits, records) as query_file_bytes, records["headers"] being batch_headers().  The memory stays untouched
        until this returns."""
        rc = self._check(lib().mc_batch_add_device_bytes(self.h, slot, ptr or None, nbytes, PARSE_PAIRS if pairs else 0, insert_max))
        return self._query_raw_slot(rc, lowest, slot, headers=True)

    def resident_input(self, file_bytes, records_per_batch: int, pairs: bool = False, piece_bytes: int = 1 << 31, slot_bytes=None, max_resident_bytes: int = 1 << 62):
        """a query file's bytes (plain or BGZF) made resident and cut into batches (mc_input_open) -> dict(info uint64 [8] = verdict, detail,
        plain bytes, pieces, batches, records, inflated, second detail; handle (None where nothing is resident), ptr: the device address of
        the plain bytes, nbytes, batches: input_batch_dtype rows).  close_input(handle) frees it."""
        buf = np.frombuffer(bytes(file_bytes), dtype=np.uint8)
        info, h = np.zeros(8, dtype=np.uint64), C.c_void_p()
        self._check(lib().mc_input_open(self.h, buf.ctypes.data if len(buf) else None, len(buf), PARSE_PAIRS if pairs else 0, records_per_batch, piece_bytes,
                                        self.cfg.slot_max_chars if slot_bytes is None else slot_bytes, max_resident_bytes, C.byref(h), info.ctypes.data))
        out = dict(info=info, handle=h.value, ptr=0, nbytes=0, batches=np.zeros(0, dtype=input_batch_dtype))
        if h.value:
            rows, ptr, n = np.zeros(int(info[4]), dtype=input_batch_dtype), C.c_void_p(), C.c_uint64()
            self._check(lib().mc_input_batches(h, rows.ctypes.data if len(rows) else None, len(rows), C.byref(ptr), C.byref(n)))
            out.update(ptr=ptr.value or 0, nbytes=n.value, batches=rows)
        return out

    def download_input(self, handle: int, nbytes: int) -> bytes:
        """the plain bytes of a resident file, copied back (mc_input_download)"""
        buf = np.zeros(max(nbytes, 1), dtype=np.uint8)
        self._check(lib().mc_input_download(handle, buf.ctypes.data, nbytes))
        return buf[:nbytes].tobytes()

    def close_input(self, handle):
        if handle:
            lib().mc_input_close(handle)

    def parse_stats(self):
        """-> [mc_parse_records calls, bytes handed over, records of the accepted ranges, ranges refused]"""
        st = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_parse_stats(self.h, st.ctypes.data))
        return [int(x) for x in st]

    # ---- BGZF members inflated on the device (mc_inflate_*) ------------------------------------------------
    def inflate_device(self, bytes_ptr: int, nbytes: int, blocks_ptr: int, num_blocks: int, out_ptr: int, out_capacity: int, status_ptr: int, stream: int = 0):
        """inflates the members that the rows at blocks_ptr (bgzf_block_dtype) name out of the range at bytes_ptr into out -- all device
        memory (bytes, out: 16-byte aligned; blocks, status [4] uint64: 8-byte); asynchronous on `stream`.  status = verdict, lowest bad
        row, its reason, bytes of out covered"""
        self._check(lib().mc_inflate_blocks(self.h, bytes_ptr or None, nbytes, blocks_ptr or None, num_blocks, 0, out_ptr or None, out_capacity,
                                            status_ptr or None, stream or None))

    def inflate_raw(self, data, blocks, out_capacity=None):
        """the host form as it is: -> (out uint8 [out_capacity], status uint64 [4]); out_capacity defaults to the end of the last slice"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rows = np.ascontiguousarray(blocks, dtype=bgzf_block_dtype)
        if out_capacity is None:
            out_capacity = int((rows["out_off"] + rows["out_len"]).max()) if len(rows) else 0
        out = np.zeros(max(out_capacity, 1), dtype=np.uint8)
        status = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_inflate_blocks(self.h, buf.ctypes.data if len(buf) else None, len(buf), rows.ctypes.data if len(rows) else None, len(rows),
                                            INFLATE_HOST, out.ctypes.data, out_capacity, status.ctypes.data, None))
        return out[:out_capacity], status

    def inflate(self, data, blocks=None):
        """a BGZF range -> the bytes gzip.decompress gives (host form; indexes first where blocks is None).  None for a range that is
        not BGZF; McError with .verdict, .block and .reason where the device refuses a member"""
        if blocks is None:
            blocks, _, verdict, _ = bgzf_index(data)
            if verdict != BGZF_OK:
                return None
        out, status = self.inflate_raw(data, blocks)
        if int(status[0]) != INFLATE_OK:
            e = McError(f"mc_inflate_blocks: verdict {int(status[0])}, block {int(status[1])}, reason {int(status[2])}")
            e.verdict, e.block, e.reason = int(status[0]), int(status[1]), int(status[2])
            raise e
        return out.tobytes()

    def inflate_stats(self):
        """-> [mc_inflate_blocks calls, bytes in, bytes out of the accepted calls, calls refused]"""
        st = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_inflate_stats(self.h, st.ctypes.data))
        return [int(x) for x in st]

    # ---- whole gzip files inflated on the device (mc_inflate_streams) ----------------------------------------
    def inflate_streams_device(self, bytes_ptr: int, nbytes: int, rows_ptr: int, num_rows: int, out_ptr: int, out_capacity: int, results_ptr: int,
                               status_ptr: int, stream: int = 0):
        """inflates the gzip files that the rows at rows_ptr (gzip_stream_dtype) name out of the range at bytes_ptr, each into its own slice
        of out -- all device memory (bytes, out: 16-byte aligned; rows, results gzip_result_dtype [num_rows], status [4] uint64: 8-byte);
        asynchronous on `stream`.  The slices must be disjoint.  status = verdict, lowest refused row, its reason, accepted rows"""
        self._check(lib().mc_inflate_streams(self.h, bytes_ptr or None, nbytes, rows_ptr or None, num_rows, 0, out_ptr or None, out_capacity,
                                             results_ptr or None, status_ptr or None, stream or None))

    def inflate_streams_raw(self, data, rows, out_capacity=None):
        """the host form as it is: -> (out uint8 [out_capacity], results gzip_result_dtype [rows], status uint64 [4]); out_capacity defaults
        to the end of the last slice"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        rows = np.ascontiguousarray(rows, dtype=gzip_stream_dtype)
        if out_capacity is None:
            out_capacity = int((rows["out_off"] + rows["out_cap"]).max()) if len(rows) else 0
        out = np.zeros(max(out_capacity, 1), dtype=np.uint8)
        results = np.zeros(max(len(rows), 1), dtype=gzip_result_dtype)
        status = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_inflate_streams(self.h, buf.ctypes.data if len(buf) else None, len(buf), rows.ctypes.data if len(rows) else None, len(rows),
                                             INFLATE_HOST, out.ctypes.data, out_capacity, results.ctypes.data, status.ctypes.data, None))
        return out[:out_capacity], results[:len(rows)], status

    def inflate_streams(self, files, out_caps=None):
        """gzip files (a list of bytes) -> (a list with each accepted file's plain bytes and None for a refused one, results
        gzip_result_dtype [files]).  Host form.  out_caps: room per file; default: each file's trailing ISIZE (gzip_hint)"""
        files = [bytes(f) for f in files]
        if out_caps is None:
            out_caps = [gzip_hint(f)[2] for f in files]
        rows = np.zeros(len(files), dtype=gzip_stream_dtype)
        in_at = out_at = 0
        for i, (f, cap) in enumerate(zip(files, out_caps)):
            rows[i] = (in_at, len(f), out_at, cap)
            in_at += (len(f) + 15) // 16 * 16
            out_at += cap
        data = b"".join(f + bytes(-len(f) % 16) for f in files)
        out, results, _ = self.inflate_streams_raw(data, rows, out_at)
        plain = [None if int(r["reason"]) else out[int(w["out_off"]):int(w["out_off"]) + int(r["produced"])].tobytes() for w, r in zip(rows, results)]
        return plain, results

    def inflate_streams_stats(self):
        """-> [mc_inflate_streams calls, bytes in, bytes out of the accepted rows, rows refused]"""
        st = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_inflate_streams_stats(self.h, st.ctypes.data))
        return [int(x) for x in st]

    # ---- the all-hits column: location lists, run-length encoded (mc_format_matches*) ----------------
    def format_matches_set_text(self, strings):
        """the table of texts indexed by target: a list of bytes, e.g. from match_texts()"""
        data, off = pack_strings([bytes(x) for x in strings])
        buf = np.frombuffer(data, dtype=np.uint8) if data else np.zeros(1, dtype=np.uint8)
        self._check(lib().mc_format_matches_set_text(self.h, buf.ctypes.data, off.ctypes.data, len(off) - 1))

    def format_matches_device(self, hits_ptr: int, hit_off_ptr: int, n: int, *, flags: int = 0, out_ptr: int, out_capacity: int, piece_off_ptr: int,
                              stream: int = 0):
        """renders the pieces of n location lists in device memory into out_ptr (16-byte aligned); piece_off_ptr: n + 1 + FORMAT_SCRATCH
        uint64, entry n = the bytes all pieces need (more than out_capacity: nothing was written); asynchronous on `stream`"""
        self._check(lib().mc_format_matches(self.h, hits_ptr or None, hit_off_ptr or None, n, flags, out_ptr or None, out_capacity,
                                            piece_off_ptr or None, stream or None))

    def format_matches(self, hits: np.ndarray, hit_off: np.ndarray, *, flags: int = 0):
        """the same on host arrays: hits (loc_dtype: win, tgt), hit_off uint64 [n + 1] -> (bytes: all pieces, piece_off uint64 [n + 1])"""
        hits = np.ascontiguousarray(hits, dtype=loc_dtype)
        hit_off = np.ascontiguousarray(hit_off, dtype=np.uint64)
        n = len(hit_off) - 1
        piece_off = np.zeros(n + 1, dtype=np.uint64)
        args = lambda out, cap: (self.h, hits.ctypes.data if len(hits) else None, hit_off.ctypes.data, n, flags | FORMAT_HOST, out, cap,
                                 piece_off.ctypes.data, None)
        rc = lib().mc_format_matches(*args(None, 0))                         # the size first: piece_off is complete either way
        if rc != -3:
            self._check(rc)
        total = int(piece_off[n])
        out = np.zeros(max(total, 1), dtype=np.uint8)
        if total:
            self._check(lib().mc_format_matches(*args(out.ctypes.data, total)))
        return out[:total].tobytes(), piece_off

    def format_matches_stats(self):
        """-> [mc_format_matches calls, reads, runs printed, bytes written, runs whose target lay beyond the table]"""
        st = np.zeros(5, dtype=np.uint64)
        self._check(lib().mc_format_matches_stats(self.h, st.ctypes.data))
        return [int(x) for x in st]

    # ---- target coverage: the two passes of -cov-percentile (mc_coverage_*) -----------------------
    def load_target_windows(self, windows: np.ndarray):
        """the targets' window counts (mc_load_target_windows) for contexts that were not opened from database files; before any table load"""
        windows = np.ascontiguousarray(windows, dtype=np.uint32)
        self._check(lib().mc_load_target_windows(self.h, windows.ctypes.data, len(windows)))

    def coverage_add_device(self, cands_ptr: int, n: int, stride: int, *, hitmin: int = 0, lowest: int = 0, stream: int = 0):
        """marks the windows that the qualifying candidates of n rows in device memory cover; asynchronous on `stream` (0 = the context's)"""
        self._check(lib().mc_coverage_add(self.h, cands_ptr or None, n, stride, int(hitmin), int(lowest), 0, stream or None))

    def coverage_add(self, cands: np.ndarray, hitmin: int = 0, lowest: int = 0):
        """the same for a host array cands[n, stride] (cand_dtype, e.g. what query() returns)"""
        cands = np.ascontiguousarray(cands, dtype=cand_dtype)
        if cands.ndim != 2:
            raise ValueError("coverage_add: cands must be [n, stride]")
        n, stride = cands.shape
        self._check(lib().mc_coverage_add(self.h, cands.ctypes.data if n else None, n, stride, int(hitmin), int(lowest), COVERAGE_HOST, None))

    def coverage_counts(self, reset: bool = False):
        """-> (covered[targets] uint32, windows[targets] uint32, stats dict: marked entries, out-of-range entries, bits, add calls)"""
        L = lib()
        num = C.c_uint64()
        self._check(L.mc_coverage_counts(self.h, None, None, 0, C.byref(num), None, 0))
        covered = np.zeros(num.value, dtype=np.uint32)
        windows = np.zeros(num.value, dtype=np.uint32)
        st = np.zeros(4, dtype=np.uint64)
        self._check(L.mc_coverage_counts(self.h, covered.ctypes.data, windows.ctypes.data, num.value, None, st.ctypes.data, int(reset)))
        return covered, windows, dict(marked=int(st[0]), out_of_range=int(st[1]), bits=int(st[2]), calls=int(st[3]))

    def coverage_set_keep(self, keep):
        """the targets whose candidates coverage_drop keeps (uint8 per target, e.g. from coverage_keep); None = no mask"""
        if keep is None:
            self._check(lib().mc_coverage_set_keep(self.h, None, 0))
            return
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        self._check(lib().mc_coverage_set_keep(self.h, keep.ctypes.data, len(keep)))

    def coverage_drop_device(self, in_ptr: int, n: int, stride: int, out_ptr: int, stream: int = 0):
        """rows in device memory without the candidates of dropped targets (out_ptr may be in_ptr); asynchronous on `stream`"""
        self._check(lib().mc_coverage_drop(self.h, in_ptr or None, n, stride, 0, out_ptr or None, stream or None))

    def coverage_drop(self, cands: np.ndarray) -> np.ndarray:
        """the same for a host array cands[n, stride] -> a new array"""
        cands = np.ascontiguousarray(cands, dtype=cand_dtype)
        if cands.ndim != 2:
            raise ValueError("coverage_drop: cands must be [n, stride]")
        n, stride = cands.shape
        out = np.zeros_like(cands)
        self._check(lib().mc_coverage_drop(self.h, cands.ctypes.data if n else None, n, stride, COVERAGE_HOST, out.ctypes.data if n else None, None))
        return out

    def classify_by_coverage(self, reads, mates=None, *, percentile: float, hitmin: int = 0, hitdiff: float = 1.0, lowest: int = 0,
                             highest: int = NUM_RANKS - 1, insert_max: int = 0, order=None) -> np.ndarray:
        """CLEARS the context's accumulated coverage, before and after, and replaces its keep mask: not for callers that gather coverage
        over several batches (they call the steps themselves).  -cov-percentile for one set of reads: query, coverage_add,
        coverage_counts, coverage_keep (targets visited in `order`, None = ascending id), coverage_drop and the vote -> assignment_dtype [n]"""
        cands, _, _ = self.query(reads, mates, lowest=lowest, insert_max=insert_max)
        self.coverage_counts(reset=True)
        self.coverage_add(cands, hitmin=hitmin, lowest=lowest)
        covered, windows, _ = self.coverage_counts(reset=True)
        self.coverage_set_keep(coverage_keep(covered, windows, percentile, order))
        left = self.coverage_drop(cands)
        return self.classify_candidates(left, hitmin=hitmin, hitdiff=hitdiff, lowest=lowest, highest=highest)

    # ---- per-target hit lists: -hits-per-ref (mc_target_hits_*) -----------------------------------
    def target_hits_reserve(self, capacity: int):
        """sizes the device log to `capacity` records (what it holds stays); 0 frees it and drops what was accumulated"""
        self._check(lib().mc_target_hits_reserve(self.h, int(capacity)))

    def target_hits_add_device(self, cands_ptr: int, n: int, stride: int, *, query_ids_ptr: int = 0, first_query_id: int = 0, hitmin: int = 0,
                               lowest: int = 0, stream: int = 0):
        """one record per qualifying candidate of n rows in device memory (query = query_ids[i] where query_ids_ptr is given, else
        first_query_id + i); asynchronous on `stream` (0 = the context's); never allocates: target_hits_reserve first"""
        self._check(lib().mc_target_hits_add(self.h, cands_ptr or None, query_ids_ptr or None, int(first_query_id), n, stride, int(hitmin), int(lowest), 0,
                                             stream or None))

    def target_hits_add(self, cands: np.ndarray, query_ids=None, first_query_id: int = 0, hitmin: int = 0, lowest: int = 0):
        """the same for a host array cands[n, stride] (cand_dtype, e.g. what query() returns); the log grows as needed, up to
        set_tuning("target_hits_max_mb"); McError (MC_ERR_NOMEM, nothing added) beyond that"""
        cands = np.ascontiguousarray(cands, dtype=cand_dtype)
        if cands.ndim != 2:
            raise ValueError("target_hits_add: cands must be [n, stride]")
        n, stride = cands.shape
        ids = None
        if query_ids is not None:
            ids = np.ascontiguousarray(query_ids, dtype=np.uint64)
            if ids.shape != (n,):
                raise ValueError("target_hits_add: one query id per row")
        self._check(lib().mc_target_hits_add(self.h, cands.ctypes.data if n else None, ids.ctypes.data if ids is not None and n else None, int(first_query_id),
                                             n, stride, int(hitmin), int(lowest), TARGET_HITS_HOST, None))

    def target_hits_stats(self, reset: bool = False) -> dict:
        """the size query of mc_target_hits_collect: targets, records and the statistics; answers when records were dropped, too"""
        nt, nr = C.c_uint64(), C.c_uint64()
        st = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_target_hits_collect(self.h, None, 0, C.byref(nt), None, 0, C.byref(nr), st.ctypes.data, int(reset)))
        return dict(targets=int(nt.value), records=int(nr.value), stored=int(st[0]), dropped=int(st[1]), calls=int(st[2]), targets_hit=int(st[3]))

    def target_hits_collect(self, reset: bool = False):
        """-> (offsets[targets + 1] uint64, records (target_hit_dtype) sorted by (tgt, beg, end, query, hits), stats dict);
        records[offsets[t]:offsets[t + 1]] is target t's list.  McError (MC_ERR_STATE) if records were dropped for lack of room."""
        size = self.target_hits_stats()
        offsets = np.zeros(size["targets"] + 1, dtype=np.uint64)
        records = np.zeros(size["records"], dtype=target_hit_dtype)
        st = np.zeros(4, dtype=np.uint64)
        self._check(lib().mc_target_hits_collect(self.h, offsets.ctypes.data, size["targets"], None, records.ctypes.data if len(records) else None, len(records),
                                                 None, st.ctypes.data, int(reset)))
        return offsets, records, dict(stored=int(st[0]), dropped=int(st[1]), calls=int(st[2]), targets_hit=int(st[3]))

    def copy_results(self, dst_ptr: int, src_ptr: int, nbytes: int, to_host: bool = False, stream: int = 0, second_pipe: bool = False, from_host: bool = False):
        L = lib()
        L.mc_copy_results_on.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_void_p]
        self._check(L.mc_copy_results_on(self.h, dst_ptr, src_ptr, nbytes, (1 if to_host else 0) | (2 if from_host else 0) | (8 if second_pipe else 0), stream or None))

    def load_stats(self) -> dict:
        """how mc_open_database read the database files (mc_load_stats)"""
        L = lib()
        L.mc_load_stats.argtypes = [C.c_void_p, C.c_void_p]
        a = (C.c_uint64 * 4)()
        self._check(L.mc_load_stats(self.h, a))
        return dict(bytes=int(a[0]), seconds=a[1] / 1e9, index_seconds=a[2] / 1e9, feeder_wait_seconds=a[3] / 1e9,
                    GB_per_s=(a[0] / a[1]) if a[1] else 0.0)

    def table_layout(self) -> dict:
        """bytes per stored location (4 = compact store: global window numbers), gap between two targets' numbers, buckets, stored list locations (mc_table_layout)"""
        a = (C.c_uint64 * 4)()
        self._check(lib().mc_table_layout(self.h, a))
        return {"location_bytes": int(a[0]) & 0xFF, "direct_index": bool(int(a[0]) >> 32), "window_gap": int(a[1]) & 0xFFFFFFFF, "list_align": int(a[1]) >> 32, "buckets": int(a[2]), "list_locations": int(a[3])}

    # ---- table content: what the table in HBM holds (mc_table_*) --------------------------------
    def table_histogram(self):
        """-> (hist[256] uint64: stored features per list size, dead: features the load-time rules emptied); table_statistics(hist)
        makes the statistics line of `info <db> statistics` from it"""
        hist = np.zeros(256, dtype=np.uint64)
        dead = C.c_uint64()
        self._check(lib().mc_table_histogram(self.h, hist.ctypes.data, C.byref(dead)))
        return hist, int(dead.value)

    def table_features(self):
        """-> (keys uint32, sizes uint32): every stored feature in ascending order with the length of its location list"""
        L = lib()
        num = C.c_uint64()
        self._check(L.mc_table_features(self.h, None, None, 0, C.byref(num), 0))
        keys = np.zeros(num.value, dtype=np.uint32)
        sizes = np.zeros(num.value, dtype=np.uint32)
        if num.value:
            self._check(L.mc_table_features(self.h, keys.ctypes.data, sizes.ctypes.data, num.value, C.byref(num), 0))
        return keys, sizes

    def table_lookup(self, keys):
        """-> (offsets[n + 1] uint64, locs (loc_dtype)): locs[offsets[i]:offsets[i + 1]] = the locations of feature keys[i] in the order of
        the database file; any order of keys, duplicates allowed, a feature the table does not hold has an empty list"""
        L = lib()
        keys = np.ascontiguousarray(keys, dtype=np.uint32)
        if keys.ndim != 1:
            raise ValueError("table_lookup: keys must be one-dimensional")
        n = len(keys)
        offsets = np.zeros(n + 1, dtype=np.uint64)
        rc = L.mc_table_lookup(self.h, keys.ctypes.data if n else None, n, offsets.ctypes.data, None, 0, 0)
        if rc != MC_ERR_NOMEM:                                     # (MC_ERR_NOMEM with the offsets complete is the size query's answer)
            self._check(rc)
        total = int(offsets[n])
        locs = np.zeros(total, dtype=loc_dtype)
        if total:
            self._check(L.mc_table_lookup(self.h, keys.ctypes.data, n, offsets.ctypes.data, locs.ctypes.data, total, 0))
        return offsets, locs

    def target_range(self) -> tuple:
        """[lo, hi): the targets whose locations this context holds (mc_target_range)"""
        a = (C.c_uint64 * 4)()
        self._check(lib().mc_target_range(self.h, a))
        self.n_features = int(a[2])                               # (features the table holds)
        return int(a[0]), int(a[1])

    def set_tuning(self, name: str, value: int):
        L = lib()
        L.mc_set_tuning.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
        self._check(L.mc_set_tuning(self.h, name.encode(), value))

    def synchronize(self):
        self._check(lib().mc_synchronize(self.h))

    def timing(self, on: bool):
        self._check(lib().mc_timing_enable(self.h, int(on)))

    def timing_reset(self):
        self._check(lib().mc_timing_reset(self.h))

    def timing_get(self, kernel: str):
        ms, cnt = C.c_double(), C.c_uint64()
        self._check(lib().mc_timing_get(self.h, kernel.encode(), C.byref(ms), C.byref(cnt)))
        return ms.value, cnt.value

    def last_batch_stats(self):
        st = np.zeros(8, dtype=np.uint64)
        self._check(lib().mc_last_batch_stats(self.h, st.ctypes.data_as(C.c_void_p)))
        return dict(windows=int(st[0]), features=int(st[1]), locations=int(st[2]), found=int(st[3]), probe_steps=int(st[4]),
                    filtered_kept=int(st[5]), filtered_reads=int(st[6]) & 0xFFFFFFFF, filtered_over_512=int(st[6]) >> 32,
                    filter_second_kernel=int(st[7]) & 0xFFFFFFFF, filter_handed_back=int(st[7]) >> 32)


class PartSet:
    """A partitioned database, `resident` parts in HBM at a time (mc_partset_*): the next group of parts is loaded while the reads run
    against this one, per-part candidates gathered over RCCL and merged on the device in part order."""

    def __init__(self, name: str, resident: int = 0, devices=None, **kw):
        L = lib()
        L.mc_partset_open.argtypes = [C.c_char_p, C.POINTER(McConfig), C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mc_partset_close.argtypes = [C.c_void_p]
        L.mc_partset_info.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_partset_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]
        L.mc_partset_last_error.argtypes = [C.c_void_p]
        L.mc_partset_last_error.restype = C.c_char_p
        kw.setdefault("kmerlen", 0); kw.setdefault("sketchlen", 0); kw.setdefault("winlen", 0); kw.setdefault("winstride", 0)   # (the database's own, as Database.open)
        self.cfg = default_config(**kw)
        self.h = C.c_void_p()
        dv = np.asarray(devices if devices is not None else [], dtype=np.int32)
        rc = L.mc_partset_open(name.encode(), C.byref(self.cfg), resident, dv.ctypes.data if len(dv) else None, len(dv), C.byref(self.h))
        if rc != 0:
            raise McError(f"mc_partset_open({name}): {L.mc_partset_last_error(None).decode()} (rc {rc})")

    def info(self) -> dict:
        a = (C.c_uint64 * 6)()
        lib().mc_partset_info(self.h, a)
        nb = C.c_uint64()
        lib().mc_partset_load_bytes(self.h, C.byref(nb))
        return dict(parts=int(a[0]), resident=int(a[1]), groups=int(a[2]), devices=int(a[3]), load_s=a[4] / 1e9, wait_s=a[5] / 1e9, load_bytes=int(nb.value))

    def select_group(self, g: int):
        L = lib()
        L.mc_partset_select_group.argtypes = [C.c_void_p, C.c_uint32]
        rc = L.mc_partset_select_group(self.h, g)
        if rc != 0:
            raise McError(f"mc_partset_select_group: {L.mc_partset_last_error(self.h).decode()} (rc {rc})")

    def classify_resident(self, reads, mates, out: np.ndarray, has_prior: bool, lowest: int = 0, insert_max: int = 0):
        """one batch through the resident group's parts; out (cand_dtype [n, K]) holds the earlier groups' lists (has_prior) and receives the merged ones"""
        def pack(rs):
            offs = np.zeros(len(rs) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(r) for r in rs])
            return np.frombuffer(b"".join(rs) + b"\0", dtype=np.uint8), offs
        s1, o1 = pack(reads)
        s2, o2 = pack(mates) if mates is not None else (None, None)
        L = lib()
        L.mc_partset_classify_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
        rc = L.mc_partset_classify_resident(self.h, s1.ctypes.data, o1.ctypes.data, s2.ctypes.data if s2 is not None else None,
                                            o2.ctypes.data if o2 is not None else None, len(reads), lowest, insert_max, int(has_prior), out.ctypes.data)
        if rc != 0:
            raise McError(f"mc_partset_classify_resident: {L.mc_partset_last_error(self.h).decode()} (rc {rc})")

    def classify_resident_packed(self, seqs: np.ndarray, offs: np.ndarray, out: np.ndarray, has_prior: bool, lowest: int = 0):
        """classify_resident for single-end reads given as one byte array + n + 1 offsets"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8); offs = np.ascontiguousarray(offs, dtype=np.uint64)
        L = lib()
        L.mc_partset_classify_resident.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_int, C.c_void_p]
        rc = L.mc_partset_classify_resident(self.h, seqs.ctypes.data, offs.ctypes.data, None, None, len(offs) - 1, lowest, 0, int(has_prior), out.ctypes.data)
        if rc != 0:
            raise McError(f"mc_partset_classify_resident: {L.mc_partset_last_error(self.h).decode()} (rc {rc})")

    def classify(self, reads, mates=None, lowest: int = 0, insert_max: int = 0) -> np.ndarray:
        """reads / mates: lists of bytes -> cand_dtype [n, max_candidates]"""
        def pack(rs):
            offs = np.zeros(len(rs) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(r) for r in rs])
            return np.frombuffer(b"".join(rs) + b"\0", dtype=np.uint8), offs
        n = len(reads)
        s1, o1 = pack(reads)
        s2, o2 = pack(mates) if mates is not None else (None, None)
        out = np.zeros((n, self.cfg.max_candidates), dtype=cand_dtype)
        L = lib()
        rc = L.mc_partset_classify(self.h, s1.ctypes.data, o1.ctypes.data, s2.ctypes.data if s2 is not None else None,
                                   o2.ctypes.data if o2 is not None else None, n, lowest, insert_max, out.ctypes.data)
        if rc != 0:
            raise McError(f"mc_partset_classify: {L.mc_partset_last_error(self.h).decode()} (rc {rc})")
        return out

    def classify_packed(self, seqs: np.ndarray, offs: np.ndarray, lowest: int = 0, insert_max: int = 0) -> np.ndarray:
        """single-end reads as one byte array + n + 1 offsets (what mc_partset_classify takes) -> cand_dtype [n, max_candidates]"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8); offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        out = np.zeros((n, self.cfg.max_candidates), dtype=cand_dtype)
        L = lib()
        rc = L.mc_partset_classify(self.h, seqs.ctypes.data, offs.ctypes.data, None, None, n, lowest, insert_max, out.ctypes.data)
        if rc != 0:
            raise McError(f"mc_partset_classify: {L.mc_partset_last_error(self.h).decode()} (rc {rc})")
        return out

    def close(self):
        if self.h:
            lib().mc_partset_close(self.h)
            self.h = C.c_void_p()


class KeySet:
    """ONE database key-sharded over the GPUs of the node (mc_keyset_*, Mode K from C++): every shard looks up its own features for all
    reads, the partial lists travel as 4-byte global window numbers to the shard that owns the read (RCCL between devices)."""

    def __init__(self, name: str, shards: int = 0, devices=None, **kw):
        L = lib()
        L.mc_keyset_open.argtypes = [C.c_char_p, C.POINTER(McConfig), C.c_uint32, C.c_void_p, C.c_uint32, C.POINTER(C.c_void_p)]
        L.mc_keyset_close.argtypes = [C.c_void_p]
        L.mc_keyset_info.argtypes = [C.c_void_p, C.c_void_p]
        L.mc_keyset_classify.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint64, C.c_int, C.c_uint64, C.c_void_p]
        L.mc_keyset_last_error.argtypes = [C.c_void_p]
        L.mc_keyset_last_error.restype = C.c_char_p
        self.cfg = default_config(**kw)
        self.h = C.c_void_p()
        dv = np.asarray(devices if devices is not None else [], dtype=np.int32)
        rc = L.mc_keyset_open(name.encode(), C.byref(self.cfg), shards, dv.ctypes.data if len(dv) else None, len(dv), C.byref(self.h))
        if rc != 0:
            raise McError(f"mc_keyset_open({name}): {L.mc_keyset_last_error(None).decode()} (rc {rc})")

    def info(self) -> dict:
        a = (C.c_uint64 * 8)()
        lib().mc_keyset_info(self.h, a)
        return dict(shards=int(a[0]), devices=int(a[1]), rccl=bool(a[2]), locations=int(a[3]), numbers_sent=int(a[4]), batches=int(a[5]),
                    reads_filtered=int(a[6]), locations_sorted=int(a[7]))

    def classify(self, reads, mates=None, lowest: int = 0, insert_max: int = 0) -> np.ndarray:
        """reads / mates: lists of bytes -> cand_dtype [n, max_candidates]"""
        def pack(rs):
            offs = np.zeros(len(rs) + 1, dtype=np.uint64)
            offs[1:] = np.cumsum([len(r) for r in rs])
            return np.frombuffer(b"".join(rs) + b"\0", dtype=np.uint8), offs
        n = len(reads)
        s1, o1 = pack(reads)
        s2, o2 = pack(mates) if mates is not None else (None, None)
        out = np.zeros((n, self.cfg.max_candidates), dtype=cand_dtype)
        L = lib()
        rc = L.mc_keyset_classify(self.h, s1.ctypes.data, o1.ctypes.data, s2.ctypes.data if s2 is not None else None,
                                  o2.ctypes.data if o2 is not None else None, n, lowest, insert_max, out.ctypes.data)
        if rc != 0:
            raise McError(f"mc_keyset_classify: {L.mc_keyset_last_error(self.h).decode()} (rc {rc})")
        return out

    def classify_packed(self, seqs: np.ndarray, offs: np.ndarray, lowest: int = 0, insert_max: int = 0) -> np.ndarray:
        """single-end reads as one byte array + n + 1 offsets (what mc_keyset_classify takes) -> cand_dtype [n, max_candidates]"""
        seqs = np.ascontiguousarray(seqs, dtype=np.uint8); offs = np.ascontiguousarray(offs, dtype=np.uint64)
        n = len(offs) - 1
        out = np.zeros((n, self.cfg.max_candidates), dtype=cand_dtype)
        L = lib()
        rc = L.mc_keyset_classify(self.h, seqs.ctypes.data, offs.ctypes.data, None, None, n, lowest, insert_max, out.ctypes.data)
        if rc != 0:
            raise McError(f"mc_keyset_classify: {L.mc_keyset_last_error(self.h).decode()} (rc {rc})")
        return out

    def close(self):
        if self.h:
            lib().mc_keyset_close(self.h)
            self.h = C.c_void_p()


class Builder:
    """Minimal database builder (mc_build_*): sketches targets on the GPU, writes reference-format files."""

    def __init__(self, **kw):
        self.cfg = default_config(**kw)
        self.h = C.c_void_p()
        rc = lib().mc_build_begin(C.byref(self.cfg), C.byref(self.h))
        if rc != MC_OK:
            raise McError(f"mc_build_begin -> {rc}: {lib().mc_last_error(None).decode()}")
        lib().mc_build_last_error.restype = C.c_char_p
        lib().mc_build_last_error.argtypes = [C.c_void_p]

    def _check(self, rc):
        if rc < 0:
            raise McError(f"builder error {rc}: {lib().mc_build_last_error(self.h).decode()}")

    def add_target(self, seq: np.ndarray | bytes, name: str, parent_taxid: int = 0, filename: str = ""):
        a = np.frombuffer(seq, dtype=np.uint8) if isinstance(seq, (bytes, bytearray)) else np.ascontiguousarray(seq, dtype=np.uint8)
        self._check(lib().mc_build_add_target(self.h, a.ctypes.data_as(C.c_void_p), a.size, name.encode(), parent_taxid, filename.encode()))

    def add_target_device(self, ptr: int, length: int, name: str, parent_taxid: int = 0, filename: str = "", file_index: int = 0):
        """a target whose characters are already in device memory (mc_build_add_target_device): valid until flush() / finish()"""
        L = lib()
        L.mc_build_add_target_device.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_char_p, C.c_int64, C.c_char_p, C.c_uint64]
        self._check(L.mc_build_add_target_device(self.h, ptr, length, name.encode(), parent_taxid, filename.encode(), file_index))

    def add_parsed_targets(self, seq_ptr: int, targets, names, parents=None, filenames=None):
        """the targets of a range that parse_targets_device has cut, in order: seq_ptr = the device address of its seq, targets = its rows
        (host copy, parse_target_dtype), names[r] per record, parents[r] (None: 0), filenames[file] (None: "").  Records with len == 0 are
        skipped, as the build loop skips them.  The memory stays valid until flush() / finish().  -> targets added"""
        added = 0
        for r, t in enumerate(targets):
            if int(t["len"]) == 0:
                continue
            self.add_target_device(seq_ptr + int(t["seq_off"]), int(t["len"]), names[r], 0 if parents is None else int(parents[r]),
                                   "" if filenames is None else filenames[int(t["file"])], int(t["index"]))
            added += 1
        return added

    def flush(self):
        lib().mc_build_flush.argtypes = [C.c_void_p]
        self._check(lib().mc_build_flush(self.h))

    def reserve(self, pairs: int):
        lib().mc_build_reserve.argtypes = [C.c_void_p, C.c_uint64]
        self._check(lib().mc_build_reserve(self.h, pairs))

    def table_begin(self, expect_keys: int = 0, expect_values: int = 0) -> "Database":
        """streaming table build (mc_build_table_begin): -> Database whose table takes finished builders through table_add()"""
        self._sync_cfg()
        out = C.c_void_p()
        lib().mc_build_table_begin.argtypes = [C.c_void_p, C.c_uint64, C.c_uint64, C.POINTER(C.c_void_p)]
        self._check(lib().mc_build_table_begin(self.h, expect_keys, expect_values, C.byref(out)))
        cfg = McConfig.from_buffer_copy(self.cfg)
        cfg.key_shard_index, cfg.key_shard_count = 0, 1
        return Database.from_handle(out.value, cfg)

    def table_add(self, db: "Database"):
        lib().mc_build_table_add.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib().mc_build_table_add(db.h, self.h))

    @staticmethod
    def table_end(db: "Database"):
        lib().mc_build_table_end.argtypes = [C.c_void_p]
        db._check(lib().mc_build_table_end(db.h))
        db.refresh_info()

    def finish(self, load: bool = True, **query_kw) -> "Database | None":
        """Sort + bucketise.  load=True also returns a query Database holding the table."""
        if not load:
            self._check(lib().mc_build_finish(self.h, None))
            return None
        for k, v in query_kw.items():
            setattr(self.cfg, k, v)
        # the builder creates the query context from ITS config; update it first
        out = C.c_void_p()
        self._sync_cfg()
        self._check(lib().mc_build_finish(self.h, C.byref(out)))
        return Database.from_handle(out.value, self.cfg)

    @staticmethod
    def finish_shards(builders: "list[Builder]") -> "Database":
        """One query table from builders that were given the same targets and the key shards 0 .. n-1 of n (mc_build_finish_shards)."""
        for b in builders:
            b._sync_cfg()
        arr = (C.c_void_p * len(builders))(*[b.h for b in builders])
        out = C.c_void_p()
        lib().mc_build_finish_shards.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.POINTER(C.c_void_p)]
        builders[0]._check(lib().mc_build_finish_shards(arr, len(builders), C.byref(out)))
        cfg = McConfig.from_buffer_copy(builders[0].cfg)
        cfg.key_shard_index, cfg.key_shard_count = 0, 1
        return Database.from_handle(out.value, cfg)

    def counts(self) -> tuple[int, int]:
        """(features, locations) held after finish (mc_build_counts)"""
        k, v = C.c_uint64(), C.c_uint64()
        lib().mc_build_counts.argtypes = [C.c_void_p, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
        self._check(lib().mc_build_counts(self.h, C.byref(k), C.byref(v)))
        return k.value, v.value

    def remove_ambiguous(self, ancestor_of_target: np.ndarray, max_ambig: int = 1) -> int:
        """-remove-ambig-features after finish(load=False): ancestor_of_target[t] = id of target t's taxon on the chosen rank (0 = none).
        Returns the number of features dropped (mc_build_remove_ambiguous)."""
        a = np.ascontiguousarray(ancestor_of_target, dtype=np.uint32)
        rem = C.c_uint64()
        lib().mc_build_remove_ambiguous.argtypes = [C.c_void_p, C.c_void_p, C.c_uint64, C.c_uint32, C.POINTER(C.c_uint64)]
        self._check(lib().mc_build_remove_ambiguous(self.h, a.ctypes.data_as(C.c_void_p), a.size, max_ambig, C.byref(rem)))
        return rem.value

    def _sync_cfg(self):
        lib().mc_build_set_query_config.argtypes = [C.c_void_p, C.POINTER(McConfig)]
        lib().mc_build_set_query_config(self.h, C.byref(self.cfg))

    def write(self, name: str, taxa: list[tuple[int, int, int, str]]):
        """taxa: (id, parent, rank, name) of the non-target taxa"""
        class Rec(C.Structure):
            _fields_ = [("id", C.c_int64), ("parent", C.c_int64), ("rank", C.c_uint32), ("name", C.c_char_p)]
        arr = (Rec * max(len(taxa), 1))()
        keep = []
        for i, (tid, par, rk, nm) in enumerate(taxa):
            b = nm.encode(); keep.append(b)
            arr[i] = Rec(tid, par, rk, b)
        self._check(lib().mc_build_write(self.h, name.encode(), C.cast(arr, C.c_void_p), len(taxa)))

    @staticmethod
    def write_shards(builders: "list[Builder]", name: str, taxa: list[tuple[int, int, int, str]]):
        """<name>.meta + <name>.cache0 from the finished builders of one key-sharded set (mc_build_write_shards)"""
        class Rec(C.Structure):
            _fields_ = [("id", C.c_int64), ("parent", C.c_int64), ("rank", C.c_uint32), ("name", C.c_char_p)]
        arr = (Rec * max(len(taxa), 1))()
        keep = []
        for i, (tid, par, rk, nm) in enumerate(taxa):
            b = nm.encode(); keep.append(b)
            arr[i] = Rec(tid, par, rk, b)
        hs = (C.c_void_p * len(builders))(*[b.h for b in builders])
        lib().mc_build_write_shards.argtypes = [C.POINTER(C.c_void_p), C.c_uint32, C.c_char_p, C.c_void_p, C.c_uint64]
        builders[0]._check(lib().mc_build_write_shards(hs, len(builders), name.encode(), C.cast(arr, C.c_void_p), len(taxa)))

    def write_begin(self, name: str, taxa: list[tuple[int, int, int, str]]):
        """streaming writer (mc_build_write_begin): -> handle for write_add / write_end"""
        class Rec(C.Structure):
            _fields_ = [("id", C.c_int64), ("parent", C.c_int64), ("rank", C.c_uint32), ("name", C.c_char_p)]
        arr = (Rec * max(len(taxa), 1))()
        keep = []
        for i, (tid, par, rk, nm) in enumerate(taxa):
            b = nm.encode(); keep.append(b)
            arr[i] = Rec(tid, par, rk, b)
        w = C.c_void_p()
        lib().mc_build_write_begin.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_uint64, C.POINTER(C.c_void_p)]
        self._check(lib().mc_build_write_begin(self.h, name.encode(), C.cast(arr, C.c_void_p), len(taxa), C.byref(w)))
        return w

    def write_add(self, writer):
        lib().mc_build_write_add.argtypes = [C.c_void_p, C.c_void_p]
        self._check(lib().mc_build_write_add(writer, self.h))

    @staticmethod
    def write_end(writer):
        lib().mc_build_write_end.argtypes = [C.c_void_p]
        rc = lib().mc_build_write_end(writer)
        if rc < 0:
            raise McError(f"mc_build_write_end -> {rc}")

    def free(self):
        if self.h:
            lib().mc_build_free(self.h)
            self.h = None


# ---- semi-global alignment (mc_align_semiglobal) -------------------------------------------------------------------------------
def _packed(seqs):
    """byte strings -> (characters, n + 1 offsets) as the C ABI takes them"""
    seqs = [x.encode() if isinstance(x, str) else bytes(x) for x in seqs]
    off = np.zeros(len(seqs) + 1, dtype=np.uint64)
    if seqs:
        off[1:] = np.cumsum([len(x) for x in seqs], dtype=np.uint64)
    chars = np.frombuffer(b"".join(seqs) + b"\0", dtype=np.uint8)
    return chars, off


class Aligner:
    """A context without a table for align_semiglobal (any Database's handle does as well)."""

    def __init__(self, handle=None, **kw):
        self.own = handle is None
        if self.own:
            cfg = default_config(**kw)
            h = C.c_void_p()
            rc = lib().mc_create(C.byref(cfg), C.byref(h))
            if rc != MC_OK:
                raise McError(f"mc_create -> {rc}: {lib().mc_last_error(None).decode()}")
            handle = h.value
        self.h = C.c_void_p(handle)

    def close(self):
        if self.own and self.h:
            lib().mc_destroy(self.h)
        self.h = None

    def set_tuning(self, name: str, value: int):
        if lib().mc_set_tuning(self.h, name.encode(), value) < 0:
            raise McError(lib().mc_last_error(self.h).decode())

    def stats(self):
        """[problems, cells of read 1's matrices, nanoseconds of the kernels, sub-batches] since the context was made"""
        st = np.zeros(4, dtype=np.uint64)
        lib().mc_align_stats(self.h, st.ctypes.data_as(C.c_void_p))
        return list(map(int, st))

    def align_packed(self, rc, ro, sc, so, mc=None, mo=None):
        """packed arrays in (uint8 characters, uint64 offsets), arrays out: raw[n, 4] int32 = read 1 forward, reverse, mate forward,
        reverse; reversed[n] uint8; aligned characters and their n + 1 offsets (first half of a problem's range: the read)"""
        n = len(ro) - 1
        raw = np.zeros((4, max(n, 1)), dtype=np.int32)
        rev = np.zeros(max(n, 1), dtype=np.uint8)
        lq = (ro[1:] - ro[:-1]).astype(np.int64); ls = (so[1:] - so[:-1]).astype(np.int64)
        cap = int(2 * np.maximum(1, lq + ls).sum()) if n else 0
        aligned = np.zeros(cap + 1, dtype=np.uint8)
        aoff = np.zeros(n + 1, dtype=np.uint64)
        p = lambda a: a.ctypes.data_as(C.c_void_p) if a is not None else None
        r = lib().mc_align_semiglobal(self.h, p(rc), p(ro), p(mc), p(mo), p(sc), p(so), n, p(raw[0]), p(raw[1]), p(raw[2]), p(raw[3]), p(rev), p(aligned), cap, p(aoff))
        if r < 0:
            raise McError(f"mc_align_semiglobal -> {r}: {lib().mc_last_error(self.h).decode()}")
        return raw[:, :n].T.copy(), rev[:n], aligned, aoff

    def align(self, reads, subjects, mates=None):
        if len(reads) != len(subjects) or (mates is not None and len(mates) != len(reads)):
            raise ValueError("align_semiglobal: one subject (and mate) per read")
        rc, ro = _packed(reads); sc, so = _packed(subjects)
        mc, mo = _packed([m if m is not None else b"" for m in mates]) if mates is not None else (None, None)
        raw, rev, aligned, aoff = self.align_packed(rc, ro, sc, so, mc, mo)
        out = []
        buf = aligned.tobytes()
        for i in range(len(reads)):
            a, b = int(aoff[i]), int(aoff[i + 1])
            h = (b - a) // 2
            out.append((int(raw[i, 1] if rev[i] else raw[i, 0]), bool(rev[i]), buf[a:a + h], buf[a + h:b]))
        return out, raw


def align_semiglobal(reads, subjects, mates=None, handle=None, scratch_mb=None):
    """Semi-global alignment of reads[i] (with mates[i], if given) to subjects[i] on the GPU, as `query -align` shows it.
    -> ([(score, reversed, aligned_query, aligned_target)], raw[n, 4] int32: read 1 forward, reverse, mate forward, reverse)"""
    A = Aligner(handle)
    try:
        if scratch_mb is not None:
            A.set_tuning("align_scratch_mb", int(scratch_mb))
        return A.align(reads, subjects, mates)
    finally:
        A.close()


MERGE_HOST, MERGE_CONTINUE = 1, 2
MERGE_OK, MERGE_IRREGULAR, MERGE_OVERFLOW = 0, 1, 2


class ResultMerger:
    """Per-part result files merged on the device (mc_merge_results_*): a context of its own, or any Database's handle.
    set_taxa, begin, then add per file (or piece of a file) in order; lists() / classify() read the store."""

    def __init__(self, handle=None, **kw):
        self.own = handle is None
        if self.own:
            cfg = default_config(**kw)
            h = C.c_void_p()
            rc = lib().mc_create(C.byref(cfg), C.byref(h))
            if rc != MC_OK:
                raise McError(f"mc_create -> {rc}: {lib().mc_last_error(None).decode()}")
            handle = h.value
        self.h = C.c_void_p(handle)
        self.capacity = self.max_candidates = 0

    def _check(self, rc, what):
        if rc < 0:
            raise McError(f"{what} -> {rc}: {lib().mc_last_error(self.h).decode()}")
        return rc

    def close(self):
        if self.h:
            lib().mc_merge_results_end(self.h)
            if self.own:
                lib().mc_destroy(self.h)
        self.h = None

    def set_taxa(self, lin, rank, ids):
        """the taxon table (lin[taxa, 21] taxon index + 1, rank[taxa] or None) and the taxid of every row"""
        lin = np.ascontiguousarray(lin, dtype=np.uint32)
        ids = np.ascontiguousarray(ids, dtype=np.int64)
        if lin.ndim != 2 or lin.shape[1] != NUM_RANKS or len(ids) != len(lin):
            raise ValueError("set_taxa: lin must be [taxa, 21] with one id per row")
        rank = None if rank is None else np.ascontiguousarray(rank, dtype=np.uint8)
        self._check(lib().mc_set_taxon_table(self.h, lin.ctypes.data, None if rank is None else rank.ctypes.data, None, len(lin)), "mc_set_taxon_table")
        self._check(lib().mc_merge_results_set_taxids(self.h, ids.ctypes.data, len(ids)), "mc_merge_results_set_taxids")

    def begin(self, capacity: int, max_candidates: int = 2, merge_below: int = 4):
        self._check(lib().mc_merge_results_begin(self.h, capacity, max_candidates, merge_below), "mc_merge_results_begin")
        self.capacity, self.max_candidates = int(capacity), int(max_candidates)

    def reserve(self, capacity: int):
        self._check(lib().mc_merge_results_reserve(self.h, capacity), "mc_merge_results_reserve")
        self.capacity = max(self.capacity, int(capacity))

    def add(self, data, tophits_column: int, file_lines: int = 0, cont: bool = False):
        """a host range (bytes) -> status[8]: result lines, comment lines, lists, entries folded, unknown taxids, verdict, offence, capacity needed"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        st = np.zeros(8, dtype=np.uint64)
        self._check(lib().mc_merge_results_add(self.h, buf.ctypes.data, len(buf), tophits_column, file_lines, MERGE_HOST | (MERGE_CONTINUE if cont else 0),
                                               st.ctypes.data, None, 0, None), "mc_merge_results_add")
        return [int(x) for x in st]

    def add_device(self, bytes_ptr: int, nbytes: int, tophits_column: int, *, status_ptr: int, workspace_ptr: int, workspace_bytes: int,
                   file_lines: int = 0, cont: bool = False, stream: int = 0):
        """device pointers; enqueued on `stream` (0: the context's), nothing is waited for"""
        self._check(lib().mc_merge_results_add(self.h, bytes_ptr, nbytes, tophits_column, file_lines, MERGE_CONTINUE if cont else 0, status_ptr,
                                               workspace_ptr, workspace_bytes, stream or None), "mc_merge_results_add")

    def lists(self, first: int = 0, count=None):
        """-> lists [count, max_candidates, 2] uint32 (taxon entry, hits), header places [count, 3] uint32 (call, offset, length), number of lists"""
        count = self.capacity - first if count is None else count
        lists = np.zeros((count, self.max_candidates, 2), dtype=np.uint32)
        places = np.zeros((count, 3), dtype=np.uint32)
        n = C.c_uint64(0)
        self._check(lib().mc_merge_results_lists(self.h, first, count, MERGE_HOST, lists.ctypes.data, places.ctypes.data, C.addressof(n), None), "mc_merge_results_lists")
        return lists, places, int(n.value)

    def lists_device(self, first: int, count: int, *, lists_ptr: int, places_ptr: int, num_ptr: int = 0, stream: int = 0):
        self._check(lib().mc_merge_results_lists(self.h, first, count, 0, lists_ptr or None, places_ptr or None, num_ptr or None, stream or None), "mc_merge_results_lists")

    def classify(self, options: McClassifyOptions, tally: bool = False, first: int = 0, count=None):
        """-> [count, 2] uint32: taxon entry, info (bits 0-7 rank, 8-15 voters) of the queries first .. first + count"""
        count = self.capacity - first if count is None else count
        out = np.zeros((count, 2), dtype=np.uint32)
        self._check(lib().mc_merge_results_classify(self.h, C.byref(options), 1 | (2 if tally else 0), first, count, out.ctypes.data, None), "mc_merge_results_classify")
        return out

    def classify_device(self, options: McClassifyOptions, first: int, count: int, out_ptr: int, stream: int = 0, tally: bool = False):
        self._check(lib().mc_merge_results_classify(self.h, C.byref(options), 2 if tally else 0, first, count, out_ptr, stream or None), "mc_merge_results_classify")

    def tally(self, reset: bool = False):
        """the tallies of the classify(..., tally=True) calls (mc_classify_tally) -> assigned [22] uint64 (reads per result rank, [21] =
        unclassified), per_taxon [taxa + 1] uint64 (index = taxon entry)"""
        n = C.c_uint64(0)
        assigned = np.zeros(NUM_RANKS + 1, dtype=np.uint64)
        self._check(lib().mc_classify_tally(self.h, assigned.ctypes.data, None, 0, C.byref(n), 0), "mc_classify_tally")
        per_taxon = np.zeros(int(n.value), dtype=np.uint64)
        self._check(lib().mc_classify_tally(self.h, assigned.ctypes.data, per_taxon.ctypes.data, len(per_taxon), None, 1 if reset else 0), "mc_classify_tally")
        return assigned, per_taxon

    def stats(self):
        """[calls, bytes, result lines of accepted ranges, entries folded, unknown taxids, ranges refused]"""
        st = np.zeros(6, dtype=np.uint64)
        self._check(lib().mc_merge_results_stats(self.h, st.ctypes.data), "mc_merge_results_stats")
        return [int(x) for x in st]


TAXMAP_HOST = 1
TAXMAP_OK, TAXMAP_IRREGULAR = 0, 1
TAXMAP_NOT_FOUND = 0xFFFFFFFFFFFFFFFF


class TaxonMapper:
    """Targets ranked from accession2taxid tables on the device (mc_taxmap_*): a context of its own, or any Database's handle.
    begin with the target names, then add per piece of a table in order; result() reads every name's taxid and the place of its row."""

    def __init__(self, handle=None, **kw):
        self.own = handle is None
        if self.own:
            cfg = default_config(**kw)
            h = C.c_void_p()
            rc = lib().mc_create(C.byref(cfg), C.byref(h))
            if rc != MC_OK:
                raise McError(f"mc_create -> {rc}: {lib().mc_last_error(None).decode()}")
            handle = h.value
        self.h = C.c_void_p(handle)
        self.count = 0

    def _check(self, rc, what):
        if rc < 0:
            raise McError(f"{what} -> {rc}: {lib().mc_last_error(self.h).decode()}")
        return rc

    def close(self):
        if self.h:
            lib().mc_taxmap_end(self.h)
            if self.own:
                lib().mc_destroy(self.h)
        self.h = None

    def begin(self, names, wanted=None):
        """names: byte strings, strictly ascending; wanted: a flag per name (None: all)"""
        names = [bytes(n) for n in names]
        flags = np.ones(len(names), dtype=np.uint8) if wanted is None else np.ascontiguousarray(np.asarray(wanted) != 0, dtype=np.uint8)
        if len(flags) != len(names):
            raise ValueError("begin: one flag per name")
        text = np.frombuffer(b"".join(names) + b"\0", dtype=np.uint8)
        off = np.zeros(len(names) + 1, dtype=np.uint64)
        if names:
            off[1:] = np.cumsum([len(n) for n in names], dtype=np.uint64)
        self._check(lib().mc_taxmap_begin(self.h, text.ctypes.data, off.ctypes.data, len(names), flags.ctypes.data if len(names) else None), "mc_taxmap_begin")
        self.count = len(names)

    def add(self, data):
        """a host range (bytes) -> status[8]: lines, rows with a target, rows with a wanted target, names newly ranked, names still wanted,
        verdict, offence, 0"""
        buf = np.frombuffer(bytes(data), dtype=np.uint8)
        st = np.zeros(8, dtype=np.uint64)
        self._check(lib().mc_taxmap_add(self.h, buf.ctypes.data if len(buf) else None, len(buf), TAXMAP_HOST, st.ctypes.data, None, 0, None), "mc_taxmap_add")
        return [int(x) for x in st]

    def add_device(self, bytes_ptr: int, nbytes: int, *, status_ptr: int, workspace_ptr: int, workspace_bytes: int, stream: int = 0):
        """device pointers; enqueued on `stream` (0: the context's), nothing is waited for"""
        self._check(lib().mc_taxmap_add(self.h, bytes_ptr or None, nbytes, 0, status_ptr or None, workspace_ptr or None, workspace_bytes, stream or None), "mc_taxmap_add")

    def add_file(self, path, piece_bytes: int = 256 << 20):
        """a whole table: the first line is dropped, the rest goes through add() in pieces of at most piece_bytes cut at line ends, until
        no name is wanted -> the statuses of the calls (the last one's verdict is not TAXMAP_OK where the device refused a piece)"""
        with open(path, "rb") as f:
            data = f.read()
        nl = data.find(b"\n")
        pos = len(data) if nl < 0 else nl + 1
        out = []
        while pos < len(data):
            end = min(len(data), pos + piece_bytes)
            if end < len(data):
                cut = data.rfind(b"\n", pos, end)
                if cut < 0:
                    cut = data.find(b"\n", end)
                end = len(data) if cut < 0 else cut + 1
            st = self.add(data[pos:end])
            out.append(st)
            if st[5] != TAXMAP_OK or st[4] == 0:
                break
            pos = end
        return out

    def result(self):
        """-> taxid [count] int64, position [count] uint64 (call * 2^32 + line start; TAXMAP_NOT_FOUND: none), wanted names not found"""
        taxid = np.zeros(self.count, dtype=np.int64)
        position = np.zeros(self.count, dtype=np.uint64)
        remaining = C.c_uint64(0)
        self._check(lib().mc_taxmap_result(self.h, taxid.ctypes.data if self.count else None, position.ctypes.data if self.count else None,
                                           C.addressof(remaining), TAXMAP_HOST, None), "mc_taxmap_result")
        return taxid, position, int(remaining.value)

    def result_device(self, *, taxid_ptr: int, position_ptr: int, stream: int = 0):
        self._check(lib().mc_taxmap_result(self.h, taxid_ptr or None, position_ptr or None, None, 0, stream or None), "mc_taxmap_result")

    def stats(self):
        """[calls, bytes, lines / rows with a target / rows with a wanted target / names ranked of the accepted ranges, ranges refused, 0]"""
        st = np.zeros(8, dtype=np.uint64)
        self._check(lib().mc_taxmap_stats(self.h, st.ctypes.data), "mc_taxmap_stats")
        return [int(x) for x in st]
