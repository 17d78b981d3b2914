"""CPU: the mc_target_hits_* calls without a device -- the names, the record's layout, the order of the checks (arguments first, then
state) -- and the model of target_hits_ref.py on hand-written cases."""
import ctypes as C
import os

import numpy as np

import classify_ref
import target_hits_ref as ref
from metacache_amd import api

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MC_OK, MC_ERR_INVALID, MC_ERR_STATE = 0, -1, -6
NAMES = ("mc_target_hits_reserve", "mc_target_hits_add", "mc_target_hits_collect")


class McTargetHit(C.Structure):                                          # the header's typedef, field by field
    _fields_ = [("tgt", C.c_uint32), ("beg", C.c_uint32), ("end", C.c_uint32), ("hits", C.c_uint32), ("query", C.c_uint64)]


def test_names_are_exported_and_declared():
    L = C.CDLL(api._build.build_library())
    header = open(os.path.join(os.path.dirname(GOLDEN), "..", "include", "metacache_amd.h")).read()
    for n in NAMES:
        assert hasattr(L, n) and n in api.EXPORTS and ("int " + n + "(") in header
    assert "#define MC_TARGET_HITS_HOST 1" in header and api.TARGET_HITS_HOST == 1
    assert "typedef struct { uint32_t tgt, beg, end, hits; uint64_t query; } mc_target_hit;" in header
    tile = api.target_hits_tile()
    assert tile >= 256 and tile & (tile - 1) == 0


def test_record_is_24_bytes_and_matches_the_binding():
    assert C.sizeof(McTargetHit) == 24
    d = api.target_hit_dtype
    assert d.itemsize == 24 and d == ref.hit_dtype
    for name, _ in McTargetHit._fields_:
        assert d.fields[name][1] == getattr(McTargetHit, name).offset
        assert d.fields[name][0].itemsize == getattr(McTargetHit, name).size


def test_error_order_arguments_first_then_state():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(GOLDEN, "toy32").encode(), C.byref(h)) == MC_OK      # lineages, but no device
    try:
        cands = np.zeros((8, 2), dtype=api.cand_dtype)
        ids = np.zeros(8, dtype=np.uint64)

        def add(ctx=h, c=cands.ctypes.data, q=ids.ctypes.data, n=4, stride=2, hitmin=0, lowest=0, flags=api.TARGET_HITS_HOST):
            return L.mc_target_hits_add(ctx, c, q, 0, n, stride, hitmin, lowest, flags, None)

        assert add(ctx=None) == MC_ERR_INVALID
        assert add(c=None) == MC_ERR_INVALID and add(c=None, flags=0) == MC_ERR_INVALID
        assert add(stride=0) == MC_ERR_INVALID and add(stride=0, n=0) == MC_ERR_INVALID          # looked at even when there is nothing to do
        assert add(lowest=-1) == MC_ERR_INVALID and add(lowest=21) == MC_ERR_INVALID and add(lowest=21, n=0) == MC_ERR_INVALID
        assert add(flags=2) == MC_ERR_INVALID and add(flags=3) == MC_ERR_INVALID and add(flags=1 << 24) == MC_ERR_INVALID
        assert add(flags=0, c=cands.ctypes.data + 4) == MC_ERR_INVALID                           # device arrays: alignment
        assert L.mc_last_error(h)
        assert add(n=0) == MC_OK and add(n=0, c=None, q=None) == MC_OK and add(n=0, flags=0) == MC_OK
        assert add() == MC_ERR_STATE and add(q=None) == MC_ERR_STATE and add(lowest=20) == MC_ERR_STATE
        assert add(stride=0) == MC_ERR_INVALID                                                   # bad arguments win over the missing state

        st = np.zeros(4, dtype=np.uint64)
        assert L.mc_target_hits_reserve(None, 16) == MC_ERR_INVALID
        assert L.mc_target_hits_reserve(h, 16) == MC_ERR_STATE
        assert L.mc_target_hits_collect(None, None, 0, None, None, 0, None, st.ctypes.data, 0) == MC_ERR_INVALID
        assert L.mc_target_hits_collect(h, None, 0, None, None, 0, None, st.ctypes.data, 0) == MC_ERR_STATE
    finally:
        L.mc_destroy(h)


def hand_lineages():
    lin = np.zeros((5, ref.NUM_RANKS), dtype=np.uint32)
    lin[:, 0] = [1, 2, 0, 4, 5]                                            # target 2 has no sequence-level taxon ...
    lin[2, 3] = 9                                                          # ... but one on rank 3
    lin[3, 0] = 0                                                          # target 3 has nothing at all
    return lin


def rows(entries, stride):
    c = np.zeros((len(entries), stride), dtype=api.cand_dtype)
    for i, e in enumerate(entries):
        for j, x in enumerate(e):
            c[i, j] = x
    return c


def test_model_orders_by_end_before_query_and_by_64_bit_queries():
    lin = hand_lineages()
    big = 2 ** 32
    #              (tgt, hits, beg, end)
    cands = rows([[(1, 5, 10, 14), (0, 3, 2, 2)],                          # query big + 7
                  [(1, 6, 10, 12), (4, 2, 0, 1)],                          # query 3: the same (tgt, beg), a smaller end
                  [(1, 7, 10, 12)],                                        # query 2 * big: the same range as query 3
                  [(1, 4, 10, 12)]], 2)                                    # query big - 1
    ids = np.array([big + 7, 3, 2 * big, big - 1], dtype=np.uint64)
    off, rec, hit = ref.collect(ref.records_of(lin, cands, 0, 0, ids), len(lin))
    got = [(int(r["tgt"]), int(r["beg"]), int(r["end"]), int(r["query"]), int(r["hits"])) for r in rec]
    assert got == [(0, 2, 2, big + 7, 3),
                   (1, 10, 12, 3, 6), (1, 10, 12, big - 1, 4), (1, 10, 12, 2 * big, 7),     # end 12 before end 14, whatever the query; queries as 64-bit numbers
                   (1, 10, 14, big + 7, 5),
                   (4, 0, 1, 3, 2)]
    assert off.tolist() == [0, 1, 5, 5, 5, 6] and hit == 3


def test_model_qualification_is_the_votes_tax_rule():
    lin = hand_lineages()
    cands = rows([[(2, 9, 0, 0), (0, 9, 1, 1)],                           # target 2: nothing on rank 0; the walk goes on to the next entry
                  [(3, 9, 0, 0)],                                          # no taxon at all
                  [(7, 9, 0, 0), (1, 1, 4, 4)],                            # beyond the table; then hits below hits_min = 2
                  [(1, 2, 5, 5), (0, 0, 6, 6), (4, 9, 7, 7)]], 3)          # hits == 0 ends the row: the entry behind it is not seen
    r0 = ref.records_of(lin, cands, 2, 0, first_query_id=100)
    assert [(int(r["tgt"]), int(r["query"])) for r in r0] == [(0, 100), (1, 103)]
    r3 = ref.records_of(lin, cands, 2, 3)                                  # lowest = 3: target 2 has its rank-3 taxon, the others nothing from rank 3 up
    assert [(int(r["tgt"]), int(r["query"])) for r in r3] == [(2, 0)]
    rng = np.random.default_rng(5)
    lin2 = rng.integers(0, 3, size=(40, ref.NUM_RANKS)).astype(np.uint32)
    tg = rng.integers(0, 45, size=200)
    for lowest in (0, 1, 7, 20):
        assert ref.tax_all(lin2, tg, lowest).tolist() == [ref.tax(lin2, t, lowest) for t in tg]
        for t in tg[:40]:                                                  # the vote classifies a single candidate exactly when it has a taxon
            v = classify_ref.vote(lin2, [t], [5], 0, 1.0, lowest, ref.NUM_RANKS - 1)
            assert (v[0] != 0) == (ref.tax(lin2, t, lowest) != 0)
