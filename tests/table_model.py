"""TEST INFRASTRUCTURE: a numpy model of the arrays a table was loaded from, and the comparison of a loaded table (mc_table_histogram,
mc_table_features, mc_table_lookup) with it.  Shared by tests/test_gpu_table_info.py and the builder's tests (tests/builder_lists.py)."""
import numpy as np


class Table:
    """the arrays of one table: keys[n] (distinct), sizes[n] (1 .. 255), vals[sum sizes, 2] = {win, tgt} in file order"""

    def __init__(self, keys, sizes, vals):
        self.keys = np.asarray(keys, dtype=np.uint32)
        self.sizes = np.asarray(sizes, dtype=np.uint8)
        self.vals = np.ascontiguousarray(vals, dtype=np.uint32).reshape(-1, 2)
        assert len(np.unique(self.keys)) == len(self.keys) and int(self.sizes.astype(np.int64).sum()) == len(self.vals)
        assert len(self.sizes) == 0 or self.sizes.min() >= 1
        self.first = np.concatenate([[0], np.cumsum(self.sizes.astype(np.int64))])[:-1].astype(np.int64)

    def stored(self, max_locs=0, rm_over=0):
        """the sizes after the load-time rules (0: not stored)"""
        eff = self.sizes.astype(np.int64)
        if rm_over:
            eff = np.where(eff > rm_over, 0, eff)
        if max_locs:
            eff = np.minimum(eff, max_locs)
        return eff

    def features(self, **rules):
        eff = self.stored(**rules)
        order = np.argsort(self.keys, kind="stable")
        order = order[eff[order] > 0]
        return self.keys[order], eff[order].astype(np.uint32)

    def lookup(self, queries, **rules):
        """-> (offsets[n + 1], locs[total, 2]) of the model"""
        eff = self.stored(**rules)
        queries = np.asarray(queries, dtype=np.uint32)
        if len(self.keys) == 0:                                             # a table without features answers every lookup with nothing
            return np.zeros(len(queries) + 1, dtype=np.uint64), self.vals[:0]
        order = np.argsort(self.keys, kind="stable")
        pos = np.searchsorted(self.keys[order], queries)
        pos = np.minimum(pos, len(order) - 1)
        idx = order[pos]
        found = self.keys[idx] == queries
        n = np.where(found, eff[idx], 0)
        offsets = np.concatenate([[0], np.cumsum(n)]).astype(np.uint64)
        total = int(offsets[-1])
        flat = np.repeat(self.first[idx], n) + (np.arange(total) - np.repeat(offsets[:-1].astype(np.int64), n))
        return offsets, self.vals[flat]


def as_pairs(locs):
    return np.stack([locs["win"], locs["tgt"]], axis=1)


def check_table(db, table, queries, **rules):
    """histogram, enumeration and lookups of a loaded table against the model"""
    keys, sizes = table.features(**rules)
    hist, dead = db.table_histogram()
    assert hist.dtype == np.uint64 and np.array_equal(hist, np.bincount(sizes, minlength=256)) and hist[0] == 0
    assert dead == len(table.keys) - len(keys)
    gk, gs = db.table_features()
    assert np.array_equal(gk, keys) and np.array_equal(gs, sizes)
    for q in (queries, keys, keys[::-1]):
        off, locs = db.table_lookup(q)
        eoff, elocs = table.lookup(q, **rules)
        assert np.array_equal(off, eoff)
        assert np.array_equal(as_pairs(locs), elocs)
