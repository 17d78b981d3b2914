"""CPU: the inputs of tests/test_gpu_builder_lists.py are proved here, before any kernel sees them -- from the model alone every case
sits on the border it is named for: lists of exactly cap - 1, cap and cap + 1 locations, every key shard owning keys of every list
class, features of exactly max_ambig and max_ambig + 1 taxa, kept lists that do not ascend, runs that begin on both sides of a block
edge, key counts on both sides of the scan's and the grids' limits, chunk and file-batch borders.  The mirror of key_owner is held
against literal rows."""
import numpy as np
import pytest

import builder_lists as bl

CAPS = [0, 1, 2, 7, 254, 1000]


def test_the_mirror_of_key_owner_against_literal_rows():
    """the rows were printed once by a host program that includes table_rules.h: the mirror is not held against the header it reads"""
    assert (bl.SH1, bl.MUL1, bl.SH2, bl.MUL2, bl.SH3, bl.OWNER_XOR) == (16, 0x85ebca6b, 13, 0xc2b2ae35, 16, 0x9E3779B9)
    for row in bl.OWNER_ROWS:
        for n, want in zip(bl.OWNER_SHARDS, row[1:]):
            assert int(bl.key_owner(row[0], n)) == want, (hex(row[0]), n)
    keys = np.array([r[0] for r in bl.OWNER_ROWS], dtype=np.uint32)
    assert bl.key_owner(keys, 3).tolist() == [r[3] for r in bl.OWNER_ROWS]
    assert {r[3] for r in bl.OWNER_ROWS} == {0, 1, 2}


def descends_somewhere(table):
    """kept lists that are not ascending in (target, window) order"""
    v = bl.vals64(table).astype(np.int64)
    inside = np.ones(len(v), dtype=bool)
    inside[table.first] = False
    falls = np.flatnonzero(inside[1:] & (v[1:] < v[:-1]))
    return len(falls)


@pytest.mark.parametrize("rm_over", [0, 1])
@pytest.mark.parametrize("m", CAPS)
def test_cap_cases_sit_on_the_cap(m, rm_over):
    case = bl.cap_case(m, rm_over=rm_over)
    M = {0: 254, 1: 1, 2: 2, 7: 7, 254: 254, 1000: 254}[m]
    assert case.cap == M and case.rule_on == (bool(rm_over) and M > 1)
    t = bl.held(case)
    arrived = dict(zip(t.keys.tolist(), t.arrived.tolist()))
    kept = dict(zip(t.keys.tolist(), t.sizes.tolist()))
    want = {"one": 1, "m-2": M - 2, "m-1": M - 1, "m": M, "m+1": M + 1, "3m+1": 3 * M + 1, "entry255": 255}
    for cname, n in want.items():
        if n < 1:
            assert cname not in case.classes
            continue
        keys = case.classes[cname]
        assert len(keys) == bl.PER_CLASS
        assert [arrived[k] for k in keys] == [n] * len(keys) and [kept[k] for k in keys] == [min(n, M)] * len(keys), cname
        for shards in (3,):                                                  # every shard owns at least one key of every list class
            assert set(bl.key_owner(keys, shards).tolist()) == set(range(shards)), cname
    assert all(k not in kept for k in case.classes["empty"])
    assert len(t.keys) == sum(len(v) for c, v in case.classes.items() if c != "empty")
    sizes = [int(s) for _, s, _ in case.batches for s in s]
    assert 255 in sizes and 0 in sizes and max(len(k) for k, _, _ in case.batches) > 1
    # the same key in several batches and more than once inside one batch
    per_batch = [np.unique(k, return_counts=True) for k, _, _ in case.batches]
    assert any(c.max() > 1 for _, c in per_batch if len(c))
    assert max(np.unique(np.concatenate([u for u, _ in per_batch]), return_counts=True)[1]) > 1
    if M > 1:
        assert descends_somewhere(t) > 0
        # "first M in arrival order" differs from "the M smallest" for some key: a sort that also orders the values is seen
        k, v = case.pairs()
        differs = 0
        for key in case.classes["m+1"] + case.classes["3m+1"]:
            mine = v[k == key]
            differs += not np.array_equal(np.sort(mine)[:M], np.sort(mine[:M]))
        assert differs > 0
    # the overpopulation rule: M - 2 and M - 1 stay, M and longer go
    f = bl.written(t, case)
    infile = set(f.keys.tolist())
    for cname in ("one", "m-2", "m-1", "m", "m+1", "3m+1", "entry255"):
        if cname in case.classes:
            stays = not case.rule_on or want[cname] <= M - 1
            assert all((k in infile) == stays for k in case.classes[cname]), cname
    if case.rule_on:
        assert 0 < len(f.keys) < len(t.keys)
    else:
        assert len(f.keys) == len(t.keys)
    # three shards hold the whole between them, each a part
    parts = [bl.held(case, i, 3) for i in range(3)]
    assert all(0 < len(p.keys) < len(t.keys) for p in parts)
    w = bl.whole(parts)
    assert np.array_equal(w.keys, t.keys) and np.array_equal(w.sizes, t.sizes) and np.array_equal(w.vals, t.vals)


def test_both_packings_describe_the_same_lists():
    a, b = bl.cap_case(7, tb=4, pack=2), bl.cap_case(7, tb=2, pack=4)
    assert a.pack == 2 and b.pack == 4 and bl.pack(a.batches[0][2], 2).dtype.itemsize == 6 and bl.pack(a.batches[0][2], 4).dtype.itemsize == 8
    assert np.array_equal(bl.held(a).vals, bl.held(b).vals)
    v = bl.pack(np.array([[5, 0xFFFE], [0xFFFFFFFF, 3]]), 2)
    assert v.tobytes() == bytes([5, 0, 0, 0, 0xFE, 0xFF, 0xFF, 0xFF, 0xFF, 0xFF, 3, 0])


def test_key_cases():
    case = bl.key_case()
    t = bl.held(case)
    assert set(t.keys.tolist()) == set(case.classes["edge"]) | set(case.classes["bits"]) and bl.NO_KEY not in t.keys
    assert t.nokey_pairs == 3 and t.pairs == len(t.vals) + 3
    base = case.classes["bits"][0]
    assert sorted((k ^ base).bit_length() - 1 for k in case.classes["bits"][1:]) == [0, 7, 8, 15, 16, 23, 24, 31]
    only = bl.held(bl.nokey_only_case())
    assert len(only.keys) == 0 and only.pairs == 5 and len(bl.held(bl.no_pairs_case()).keys) == 0 and bl.held(bl.no_pairs_case()).pairs == 0


def test_run_cases():
    for n in (1, 255, 256, 257, 16384, 16385):
        t = bl.held(bl.runs_case(n, every=0 if n > 1 else 1))
        assert len(t.keys) == n
    assert bl.held(bl.runs_case(257, every=1)).arrived.tolist() == [1] * 257
    assert bl.held(bl.runs_case(257, every=2)).arrived.min() == 2
    assert bl.held(bl.runs_case(16385, every=0)).arrived.max() > 1
    t = bl.held(bl.run_edge_case())
    assert t.run_start.tolist() == [0, 255, 256, 257] and t.sizes.tolist() == [254, 1, 1, 2] and descends_somewhere(t) > 0


@pytest.mark.parametrize("tb", [2, 4])
def test_id_cases(tb):
    case = bl.id_case(tb)
    t = bl.held(case)
    tg, win = t.vals[:, 1], t.vals[:, 0]
    assert np.all(win < case.windows[tg])
    if tb == 2:
        assert len(case.windows) == 0xFFFF and set(tg.tolist()) == {0, 255, 256, 0xFFFE}
    else:
        assert {65535, 65536, 65537} <= set(tg.tolist()) and int(case.windows[65536]) == (1 << 24) + 10 and int(win.max()) == (1 << 24) + 9
        assert t.sizes[t.keys == 300].tolist() == [1] and t.sizes[t.keys == 301].tolist() == [5]
        assert all((1 << 24) + 5 in win[t.first[i]:t.first[i] + t.sizes[i]] for i in np.flatnonzero((t.keys == 300) | (t.keys == 301)))
    for t_ in set(tg.tolist()):
        assert {0, int(case.windows[t_]) - 1} <= set(win[tg == t_].tolist())


def test_existing_lists_stand_in_front_of_sketched_ones():
    case = bl.existing_case(7)
    t = bl.held(case)
    n_old = len(case.windows)
    for cname, n in (("m-2", 5), ("m-1", 6), ("m", 7)):
        for key in case.classes[cname]:
            i = int(np.flatnonzero(t.keys == key)[0])
            tg = t.vals[t.first[i]:t.first[i] + t.sizes[i], 1]
            assert t.arrived[i] > n and t.sizes[i] == 7                     # the sketched ones are cut at the cap
            assert np.all(tg[:n] < n_old) and np.all(tg[n:] >= n_old), cname
    assert int((t.vals[:, 1] >= n_old).sum()) > 300 and case.n_targets == n_old + 2
    both = [i for i in range(len(t.keys)) if {n_old, n_old + 1} <= set(t.vals[t.first[i]:t.first[i] + t.sizes[i], 1].tolist())]
    assert both                                                              # features of both new targets: (target, window) order among the sketched


@pytest.mark.parametrize("max_ambig,nkeys", [(0, 256), (1, 257), (2, 256), (5, 257)])
def test_ambiguity_cases(max_ambig, nkeys):
    case = bl.ambig_case([max_ambig], nkeys)
    t = bl.held(case)
    lim = max(max_ambig, 1)
    assert len(t.keys) == nkeys and case.cap == bl.AMBIG_CAP
    taxa = dict(zip(t.keys.tolist(), bl.taxa_of(t, case.anc).tolist()))
    kept = set(bl.without_ambiguous(t, case.anc, max_ambig).keys.tolist())
    name = lambda c: f"{c}@{max_ambig}"
    assert all(taxa[k] == lim for k in case.classes[name("exact")]) and all(taxa[k] == lim + 1 for k in case.classes[name("plus1")])
    assert all(taxa[k] == lim + 1 for k in case.classes[name("anc0plus")]) and all(taxa[k] == 1 for k in case.classes[name("anc0")] + case.classes[name("repeat")])
    assert all(taxa[k] == 2 for k in case.classes[name("aba")])
    assert all(taxa[k] == lim for k in case.classes[name("behind")]) and all(taxa[k] == lim + 1 for k in case.classes[name("at_cap")])
    arrived = dict(zip(t.keys.tolist(), t.arrived.tolist()))
    assert all(arrived[k] == bl.AMBIG_CAP + 1 for k in case.classes[name("behind")]) and all(arrived[k] == bl.AMBIG_CAP for k in case.classes[name("at_cap")])
    for cname, keys in case.classes.items():
        assert all((k in kept) == case.stays[cname] for k in keys), cname
        assert set(bl.key_owner(keys, 3).tolist()) == {0, 1, 2}, cname
    assert 0 < len(kept) < nkeys


def test_ambiguity_sequences():
    case = bl.ambig_case([3, 1], 257)
    t = bl.held(case)
    a3 = bl.without_ambiguous(t, case.anc, 3)
    a31 = bl.without_ambiguous(a3, case.anc, 1)
    a1 = bl.without_ambiguous(t, case.anc, 1)
    assert len(t.keys) > len(a3.keys) > len(a31.keys) > 0                   # both calls compact
    assert np.array_equal(a31.keys, a1.keys) and np.array_equal(a31.vals, a1.vals)
    assert a31.sizes.max() >= 2                                             # lists that the second call's compaction moves
    one = np.full(len(bl.ANC), 5)                                            # every target in one taxon: nothing goes
    assert len(bl.without_ambiguous(t, one, 1).keys) == len(t.keys)
    gone = bl.ambig_all_go_case()
    g = bl.held(gone)
    assert len(g.keys) == 40 and len(bl.without_ambiguous(g, gone.anc, 1).keys) == 0 and len(bl.without_ambiguous(g, gone.anc, 2).keys) == 40


def test_chunk_and_batch_borders():
    big = bl.singleton_case(bl.TABLE_CHUNK + 257, "chunk")
    k = big.batches[0][0]
    assert len(np.unique(k)) == len(k) == (1 << 22) + 257 and bl.NO_KEY not in k
    assert -(-len(k) // bl.FILE_BATCH) == 5 and len(k) > bl.TABLE_CHUNK
    assert np.all(big.batches[0][2][:, 0] < big.windows[big.batches[0][2][:, 1]])
    three = bl.singleton_case(bl.FILE_BATCH + 1, "batch")
    k = three.batches[0][0]
    own = np.bincount(bl.key_owner(k, 3), minlength=3)
    assert len(np.unique(k)) == len(k) == (1 << 20) + 1 and own.min() > 0 and own[0] + own[1] < bl.FILE_BATCH < own.sum()      # the first file batch runs through shards 0 and 1 and ends inside shard 2
