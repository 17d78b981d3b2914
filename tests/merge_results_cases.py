"""Inputs for the tests of mc_merge_results_*: the toy taxonomy as the merge reads it, the golden part files, generated part files
(gaps in the ids, ties, the same taxon with more / as many / fewer hits, unknown and negative taxids, empty lists, a taxon without a
rank), files laid out around the tile, and one irregular file per clause of the line rule."""
import os

import numpy as np

import evaluate_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
TAXONOMY = os.path.join(GOLDEN, "build_in", "taxonomy")
NUM_RANKS = 21

DUMP_RANKS = {"sequence": 0, "genome": 0, "form": 1, "forma": 1, "variety": 2, "varietas": 2, "subspecies": 3, "species": 4, "species group": 5,
              "species subgroup": 5, "subgenus": 5, "genus": 6, "subtribe": 7, "tribe": 8, "subfamily": 9, "family": 10, "superfamily": 11,
              "parvorder": 11, "infraorder": 11, "suborder": 11, "order": 12, "superorder": 13, "infraclass": 13, "subclass": 13, "class": 14,
              "superclass": 15, "subphylum": 15, "phylum": 16, "division": 16, "superphylum": 17, "subkingdom": 17, "kingdom": 18,
              "subdomain": 18, "superkingdom": 19, "domain": 19, "root": 20}
RANK_NAMES = ["sequence", "form", "variety", "subspecies", "species", "subgenus", "genus", "subtribe", "tribe", "subfamily", "family", "suborder",
              "order", "subclass", "class", "subphylum", "phylum", "subkingdom", "kingdom", "domain", "root"]


def _fields(line):
    return [f.strip() for f in line.rstrip("\n").split("|")]


def read_taxonomy(path=TAXONOMY):
    """the taxa of `merge` (taxonomy_io.cpp:55-175): merged ids first (no rank, the new id as parent), then the nodes; taxon 1 is the root.
    -> [(id, parent, rank)] in table order"""
    taxa, seen, merged = [], set(), {}

    def emplace(i, p, r):
        if i != 0 and i not in seen:
            seen.add(i)
            taxa.append((i, p, r))

    mp = os.path.join(path, "merged.dmp")
    if os.path.exists(mp):
        for line in open(mp):
            f = _fields(line)
            if len(f) >= 2 and f[0]:
                merged.setdefault(int(f[0]), int(f[1]))
                emplace(int(f[0]), int(f[1]), NUM_RANKS)
    for line in open(os.path.join(path, "nodes.dmp")):
        f = _fields(line)
        if len(f) < 3 or not f[0]:
            continue
        i, p = int(f[0]), int(f[1])
        emplace(merged.get(i, i), merged.get(p, p), DUMP_RANKS.get(f[2].lower(), NUM_RANKS))
    return [(i, p, NUM_RANKS - 1 if i == 1 else r) for i, p, r in taxa]


def toy_table():
    """-> ids [n] int64, lin [n, 21] uint32, rank [n] uint8, covered [n] uint8 of the toy taxonomy"""
    taxa = read_taxonomy()
    lin, rank, covered = evaluate_ref.taxon_table(taxa)
    return np.array([t[0] for t in taxa], dtype=np.int64), lin, rank, covered


def golden_part(name: str) -> bytes:
    with open(os.path.join(GOLDEN, "merge_in", name), "rb") as f:
        return f.read()


def tophits_column(data: bytes) -> int:
    """the column of top_hits behind query_id in the file's TABLE_LAYOUT line (results_file_properties)"""
    for line in data.split(b"\n"):
        if line.startswith(b"# TABLE_LAYOUT:"):
            cols = [c.strip() for c in line[15:].split(b"|")]
            assert cols[0] == b"query_id"
            return cols.index(b"top_hits")
    raise ValueError("no TABLE_LAYOUT")


HEAD = b"# Classification will be constrained to ranks from 'species' to 'domain'.\n# TABLE_LAYOUT: query_id\t|\tquery_header\t|\ttop_hits\t|\trank:taxname\n"
COL = 2


def line(ident, header, entries, tail=b"--") -> bytes:
    hits = b",".join(b"%d:%d" % e for e in entries)
    return b"%d\t|\t%s\t|\t%s\t|\t%s\n" % (ident, header, hits, tail)


def generated_files(ids, rank):
    """three part files written at maxcand 8 over the same reads -> {name: bytes}"""
    rng = np.random.default_rng(20261020)
    ranked = [int(i) for i, r in zip(ids, rank) if r < NUM_RANKS and i > 0]
    unranked = [int(i) for i, r in zip(ids, rank) if r == NUM_RANKS]
    species = [int(i) for i, r in zip(ids, rank) if r == 4]
    files = {}
    # ids with gaps: file a reaches id 60 on 40 lines, file b has 25 lines up to id 30 (the cut), file c 33 lines up to id 45
    always = {1, 2, 4, 5, 6}
    only_a = 58                                                       # a query in one file only (and beyond the others' line counts)
    plan = {"a": sorted(set(rng.choice(np.arange(8, 58), 30, replace=False).tolist()) | always | {7, only_a, 60}),
            "b": [i for i in range(1, 31) if i != 7],                 # id 7: absent from file b
            "c": sorted(set(rng.choice(np.arange(8, 45), 25, replace=False).tolist()) | always | {7, 45})}
    for name, idents in plan.items():
        out = [HEAD, b"# generated part " + name.encode() + b"\n"]
        for k, ident in enumerate(idents):
            n = int(rng.integers(0, 9))
            hits = sorted((int(h) for h in rng.integers(1, 40, n)), reverse=True)
            taxa = [int(t) for t in rng.choice(species if k % 3 else ranked, n, replace=len(species) < n)] if n else []
            entries = list(zip(taxa, hits))
            if ident == 1:                                            # an empty list in every file
                entries = []
            if ident == 2:                                            # ties between the files
                entries = [(species[0], 12), (species[1], 12)] if name != "b" else [(species[2], 12), (species[1], 12)]
            if ident == 4:                                            # the same taxon with more / as many / fewer hits in the later files
                entries = {"a": [(species[0], 10), (species[1], 9)], "b": [(species[0], 14), (species[1], 9)], "c": [(species[0], 3), (species[2], 9)]}[name]
            if ident == 5:                                            # an unknown taxid and a negative one
                entries = [(999999937, 20), (species[0], 8), (-7, 6)]
            if ident == 6 and unranked:                               # the top candidate's taxon has no rank
                entries = [(unranked[0], 30), (species[0], 5)]
            out.append(line(ident, b"read%04d" % (ident - 1), entries))
            if k % 11 == 5:
                out.append(b"# a comment between the lines\n")
        out.append(b"# queries: %d\n# time: 0 ms\n" % len(idents))
        files[name] = b"".join(out)
    assert only_a in plan["a"] and only_a not in plan["b"] and only_a not in plan["c"]
    return files


def sweep_zones(T: int):
    """where the tail sweeps lie: lengths L .. L + 15 inside one tile, and with T - 8 <= L < T + 8 around the tile border"""
    return (("one_tile", 208), ("tile_border", T - 8))


def tile_files(T: int, ids, rank):
    """regular files laid out around the tile T -> {name: bytes}"""
    sp = [int(i) for i, r in zip(ids, rank) if r == 4]
    first = line(1, b"r0", [(sp[0], 7)])

    def pad_comment(to):                                              # a comment line that ends (with its '\n') at byte `to`
        return b"#" + b"c" * (to - 2) + b"\n"

    def after(prefix_len, rest):                                      # `rest` begins at byte prefix_len, a comment fills the front
        return pad_comment(prefix_len) + rest

    out = {}
    out["line_starts_at_T"] = after(T, first + line(2, b"r1", [(sp[1], 5)]))
    out["newline_at_T_minus_1"] = out["line_starts_at_T"]             # (the same layout: the '\n' of the comment is byte T - 1)
    out["id_straddles_T"] = after(T - 2, line(12345, b"r12344", [(sp[0], 9)]))
    out["header_straddles_T"] = after(T - 8, line(3, b"a_long_header_token", [(sp[0], 9)]))
    l = line(4, b"r3", [(sp[1], 123456), (sp[0], 77)])
    at = l.index(b"%d:" % sp[1])
    out["taxid_straddles_T"] = after(T - at - 1, l)
    out["colon_straddles_T"] = after(T - at - len(b"%d" % sp[1]), l)
    out["hits_straddle_T"] = after(T - at - len(b"%d:" % sp[1]) - 3, l)
    out["comment_across_T"] = first + b"#" + b"x" * T + b"\n" + line(2, b"r1", [(sp[1], 5)])
    out["line_longer_than_T"] = b"5\t|\tr4\t|\t%d:6\t|\t%s\n" % (sp[0], b"free text " * (T // 8)) + line(6, b"r5", [(sp[1], 2)])
    many = [line(k + 1, b"q%d" % k, [(sp[k % len(sp)], 1 + k % 50)]) for k in range(2500)]
    out["many_tiles"] = b"".join(l + b"#" + b"p" * 400 + b"\n" for l in many)   # > 256 tiles of 4096 bytes
    out["no_final_newline"] = line(1, b"only", [(sp[0], 5), (sp[1], 4)])[:-1]
    out["comments_only"] = HEAD + b"# nothing\n"
    # a range that ends inside a thread's 16 bytes: every length L .. L + 15 inside one tile and around the tile border, the last line whole
    # and without its '\n', and a (comment) line that starts in the range's last byte
    for zone, L in sweep_zones(T):
        for i in range(16):
            last = line(3 + i, b"s%d" % i, [(sp[i % len(sp)], 1 + i)])
            out["sweep_%s_%02d" % (zone, i)] = first + pad_comment(L + i - len(first) - len(last)) + last
            out["sweep_%s_%02d_cut" % (zone, i)] = first + pad_comment(L + i + 1 - len(first) - len(last)) + last[:-1]
            out["sweep_%s_%02d_last_byte" % (zone, i)] = first + pad_comment(L + i - 1 - len(first)) + b"#"
    assert all(len(out["sweep_%s_%02d%s" % (z, i, k)]) == L + i for z, L in sweep_zones(T) for i in range(16) for k in ("", "_cut", "_last_byte"))
    return out


def irregular_files(ids, rank):
    """one irregular file per clause -> {name: (bytes, offence)}; every file has regular lines in front of the offending one"""
    sp = [int(i) for i, r in zip(ids, rank) if r == 4]
    good = HEAD + line(1, b"r0", [(sp[0], 7)]) + line(2, b"r1", [])
    tail = line(9, b"r8", [(sp[1], 3)])
    bad = {
        "empty_line": b"\n",
        "crlf": line(3, b"r2", [(sp[0], 5)])[:-1] + b"\r\n",
        "bar_in_header": b"3\t|\tr2|x\t|\t%d:5\t|\t--\n" % sp[0],
        "empty_header": b"3\t|\t",
        "too_few_bars": b"3\t|\tr2\t%d:5\n" % sp[0],
        "no_tab": b"3\t|\tr2 |%d:5\n" % sp[0],
        "name_for_taxid": b"3\t|\tr2\t|\tname:5\t|\t--\n",
        "zero_hits": b"3\t|\tr2\t|\t9:0\t|\t--\n",
        "no_hits": b"3\t|\tr2\t|\t9:\t|\t--\n",
        "trailing_comma": b"3\t|\tr2\t|\t9:5,\t|\t--\n",
        "hits_11_digits": b"3\t|\tr2\t|\t9:12345678901\t|\t--\n",
        "id_2_pow_32": b"4294967296\t|\tr2\t|\t9:5\t|\t--\n",
        "duplicate_query": line(2, b"again", [(sp[0], 5)]),
        "nul_byte": b"3\0\t|\tr2\t|\t%d:5\t|\t--\n" % sp[0],
        "nul_behind_the_list": line(3, b"r2", [(sp[0], 5)])[:-1] + b"\0\n",
    }
    out = {}
    for name, b in bad.items():
        if name == "empty_header":
            b = b + b"\n"
        out[name] = (good + b + tail, len(good))
    # a line that starts in the last byte of the range, at every residue of the length: an id without the rest of its line
    for zone, L in sweep_zones(4096):
        for i in range(16):
            data = good + b"#" + b"c" * (L + i - len(good) - 3) + b"\n7"
            assert len(data) == L + i
            out["last_byte_%s_%02d" % (zone, i)] = (data, L + i - 1)
    return out
