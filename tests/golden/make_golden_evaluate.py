#!/usr/bin/env python3
"""Input for the -taxon-coverage tests: a read file whose headers name taxa the database does not cover.

Needs cli_truth.fa (written by make_golden_cli.py) and the toy32 database, against whose taxonomy the ids below are checked.  Writes data only:

  evaluate_truth.fa             the reads of cli_truth.fa; every third one under a new header `e<i> taxid|<id>|x` whose id is a taxon of
                                toy32 that no target covers -- ranked ones and ones without a rank (the next ranked ancestor is then
                                the truth) --, the rest under the headers they had

There is NO recorded reference output beside it.  The reference's `query toy32 evaluate_truth.fa -taxon-coverage ...` (and the same on
cli_truth.fa) ends with a segmentation fault before it prints a line: taxonomy::make_lineage (taxonomy.hpp:619-644), which
taxonomy_cache::covers calls for every target, stores the taxon at index `rank` of a vector that is still empty.  What the tests hold
the false-positive block to is therefore the model (tests/evaluate_ref.py) and `mcq`'s own host loop, not a recorded file.

Usage:  python tests/golden/make_golden_evaluate.py
"""
from __future__ import annotations

import ctypes as C
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

# taxa of toy32 outside every target's parent chain: order, class, phylum, genus, family, species ...
UNCOVERED_RANKED = [51291, 28216, 976, 780, 28256, 1048758, 204428, 809]
# ... and without a rank (their next ranked ancestor stands in for them)
UNCOVERED_UNRANKED = [113236, 235573, 171554, 83553, 1301081, 710]


def check_ids():
    """what the file is for holds of toy32 as it is: every id is a taxon of the database that no target covers, the first list's have
    a rank, the second list's have none but a ranked ancestor (from the library's own taxon table of toy32.meta; no device needed)"""
    from metacache_amd import api
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(HERE, "toy32").encode(), C.byref(h)) == 0
    try:
        n = C.c_uint64()
        L.mc_db_num_taxa(h, C.byref(n))
        index_of_id = {}
        for i in range(n.value):
            tid = C.c_int64()
            L.mc_db_taxon(h, i, C.byref(tid), None, None, None)
            index_of_id[tid.value] = i
        pl, pr, pc, nt = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_uint64()
        assert L.mc_db_taxon_table(h, C.byref(pl), C.byref(pr), C.byref(pc), C.byref(nt)) == 0 and pc.value
        lin = (C.c_uint32 * (nt.value * 21)).from_address(pl.value)
        rank = (C.c_uint8 * nt.value).from_address(pr.value)
        covered = (C.c_uint8 * nt.value).from_address(pc.value)
        for tid in UNCOVERED_RANKED + UNCOVERED_UNRANKED:
            assert tid in index_of_id, f"taxon {tid} is not in toy32"
            i = index_of_id[tid]
            assert not covered[i], f"taxon {tid} is covered by a target"
            if tid in UNCOVERED_RANKED:
                assert rank[i] < 21, f"taxon {tid} has no rank"
            else:
                assert rank[i] == 21 and any(lin[i * 21:(i + 1) * 21]), f"taxon {tid}: ranked, or without a ranked ancestor"
    finally:
        L.mc_destroy(h)


def main():
    check_ids()
    recs = []
    with open(os.path.join(HERE, "cli_truth.fa")) as f:
        for line in f.read().split("\n"):
            if line.startswith(">"):
                recs.append([line[1:], []])
            elif line.strip():
                recs[-1][1].append(line.strip())
    ids = UNCOVERED_RANKED + UNCOVERED_UNRANKED
    with open(os.path.join(HERE, "evaluate_truth.fa"), "w") as f:
        for i, (header, seq) in enumerate(recs):
            if i % 3 == 0:
                header = f"e{i:04d} taxid|{ids[(i // 3) % len(ids)]}|x"
            f.write(">" + header + "\n" + "\n".join(seq) + "\n")
    print(f"{len(recs)} reads, {(len(recs) + 2) // 3} under new headers")


if __name__ == "__main__":
    main()
