"""GPU: the database builder's device stages (csrc/builder.hip: stable sort, run count, cap, compaction, the ambiguity kernels, the
build-time overpopulation rule, the key-shard filter, the chunked hand-over to the table, the file writer's batches) on location lists
chosen in tests/builder_lists.py and proved on their borders by tests/test_builder_lists_cpu.py.  The lists go in through
mc_build_add_existing_target / mc_build_add_locations; each case is checked (a) by mc_build_counts and the `removed` of
mc_build_remove_ambiguous, (b) by the written files read back with the oracle's reader, (c) by the table loaded from the builders and
by the table opened from the files, all against the plain model of builder_lists.py.  The tables here are never queried: their lists
are in orders no sketcher produces.

Not tested here: mc_build_write_add's host slice of 2^24 keys (a second slice needs about 200 MB of pairs); see the docstring of
builder_lists.py for everything the model leaves open."""
import ctypes as C

import numpy as np
import pytest

import builder_lists as bl

pytestmark = pytest.mark.gpu


# ---- 1. the cap ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,tb,pack", [(0, 4, 4), (1, 4, 4), (2, 2, 2), (7, 4, 2), (7, 2, 4), (254, 4, 4), (1000, 2, 2)])
def test_cap_border(tmp_path, m, tb, pack):
    """lists of 1, M - 2 .. M + 1 and 3M + 1 locations, an entry of 255, empty entries, arrival orders that do not ascend: the first M in
    arrival order stay"""
    held, _ = bl.run_case(bl.cap_case(m, tb=tb, pack=pack), tmp_path)
    assert held.sizes.max() == min(m or 254, 254)


# ---- 2. keys ------------------------------------------------------------------------------------------------------------------------
def test_key_border(tmp_path):
    held, _ = bl.run_case(bl.key_case(), tmp_path)
    assert bl.NO_KEY not in held.keys and {0, 0xFFFFFFFE} <= set(held.keys.tolist())


@pytest.mark.parametrize("make", [bl.nokey_only_case, bl.no_pairs_case])
def test_builders_without_features(tmp_path, make):
    """only pairs of key 0xFFFFFFFF, and no pairs at all: a readable database with zero features, a table that answers nothing"""
    held, in_file = bl.run_case(make(), tmp_path)
    assert len(held.keys) == 0 and len(in_file.keys) == 0


# ---- 3. runs and grids --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nkeys,every", [(1, 1), (255, 0), (256, 0), (257, 0), (16384, 0), (16385, 0), (257, 1), (257, 2)])
def test_run_and_grid_borders(tmp_path, nkeys, every):
    """distinct keys on both sides of a block of one-thread-per-run grids and of the single-block scan's limit; every = 1: singletons
    only, 2: no singleton"""
    held, _ = bl.run_case(bl.runs_case(nkeys, every), tmp_path)
    assert len(held.keys) == nkeys


def test_runs_that_begin_at_a_block_edge(tmp_path):
    """after sorting, runs begin at pair 255, 256 and 257: count_runs_kernel compares with the pair before, across the block's edge"""
    case = bl.run_edge_case()
    assert bl.held(case).run_start.tolist() == [0, 255, 256, 257]
    held, _ = bl.run_case(case, tmp_path)
    assert held.sizes.tolist() == [254, 1, 1, 2]


# ---- 4. mc_build_reserve ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", [8, 1 << 21])
def test_reserve(tmp_path, first):
    """reserve(8), 8 pairs, then a batch that makes grow_pairs copy the 8: all stay, in order; a reserve larger than ever needed;
    reserve after finish is refused"""
    rng = np.random.default_rng(4)
    lists = [(77, bl.some_locations(rng, bl.SMALL_WINDOWS, 8, "desc"), [8])]
    more = [(77, bl.some_locations(rng, bl.SMALL_WINDOWS, 40, "shuffled"), [40]), (5, bl.some_locations(rng, bl.SMALL_WINDOWS, 60, "desc"), [60])]
    case = bl.Case(f"reserve{first}", bl.SMALL_WINDOWS, bl.batches_of(rng, lists, 1) + bl.batches_of(rng, more, 1))
    assert len(case.batches[0][2]) == 8
    b = bl.make_builder(case)
    try:
        b.reserve(first)
        bl.add_batches(b, case)
        model = bl.held(case)
        assert bl.finish(b) == (2, 108) == (len(model.keys), len(model.vals))
        assert bl.L().mc_build_reserve(b.h, 1 << 22) == bl.MC_ERR_STATE
        name = str(tmp_path / case.name)
        bl.write([b], name)
        bl.check_file(name, model, case)
        bl.check_tables([b], name, model, model, case, np.array([77, 5, 6], dtype=np.uint32))
    finally:
        b.free()


# ---- 5. target ids and packing ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tb", [2, 4])
def test_target_ids_and_windows(tmp_path, tb):
    """the largest target ids of both packings, first and last windows, and (4 bytes) a location at window 2^24 + 5, which the table's
    direct index cannot hold"""
    held, _ = bl.run_case(bl.id_case(tb), tmp_path)
    assert int(held.vals[:, 1].max()) == (0xFFFE if tb == 2 else 65537)


# ---- 6. existing lists in front of sketched ones --------------------------------------------------------------------------------------
def test_existing_lists_in_front_of_sketched_ones(tmp_path):
    held, _ = bl.run_case(bl.existing_case(7), tmp_path)
    assert held.sizes.max() == 7 and int(held.vals[:, 1].max()) == len(bl.SMALL_WINDOWS) + 1


# ---- 7. key shards ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [7, 0])
def test_three_key_shards(tmp_path, m):
    """the same batches into shards 0, 1, 2 of 3: each keeps the model's keys, together they write the whole file and load the whole table;
    one shard alone is no database"""
    case = bl.cap_case(m, tb=4)
    bl.run_case(case, tmp_path, shards=3)
    b = bl.make_builder(case, 1, 3)
    try:
        bl.add_batches(b, case)
        bl.finish(b)
        assert bl.L().mc_build_write(b.h, str(tmp_path / "alone").encode(), None, 0) == bl.MC_ERR_UNSUPPORTED
        arr = (C.c_void_p * 1)(b.h)
        assert bl.L().mc_build_write_shards(arr, 1, str(tmp_path / "alone").encode(), None, 0) < 0
        assert not (tmp_path / "alone.meta").exists() and not (tmp_path / "alone.cache0").exists()
    finally:
        b.free()


# ---- 8. the build-time overpopulation rule ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shards", [1, 3])
@pytest.mark.parametrize("m", [1, 2, 7, 254])
def test_overpopulated_features_leave_at_build_time(tmp_path, m, shards):
    """remove_overpopulated: lists of M - 2 and M - 1 stay, lists of M and longer are absent from the file and dead in the loaded table
    (the counts still include them: the builder holds them until it writes or loads); with a cap of 1 the rule is off"""
    case = bl.cap_case(m, rm_over=1, tb=4 if m != 2 else 2)
    held, in_file = bl.run_case(case, tmp_path, shards=shards)
    if m == 1:
        assert len(in_file.keys) == len(held.keys)
    else:
        assert 0 < len(in_file.keys) < len(held.keys) and in_file.sizes.max() == m - 1


# ---- 9. ambiguity -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_ambig,nkeys", [(0, 256), (1, 257), (2, 256), (5, 257)])
def test_ambiguity_on_chosen_taxa(tmp_path, max_ambig, nkeys):
    case = bl.ambig_case([max_ambig], nkeys)
    held, _ = bl.run_case(case, tmp_path, ambig=[max_ambig])
    gone = [k for c, keys in case.classes.items() if not case.stays[c] for k in keys]
    assert gone and not set(gone) & set(held.keys.tolist()) and len(held.keys) == nkeys - len(gone)


def test_ambiguity_removes_nothing_or_everything(tmp_path):
    case = bl.ambig_case([1], 256)
    case.anc = np.full(len(bl.ANC), 5, dtype=np.uint32)                     # one taxon for all: the call without compaction
    held, _ = bl.run_case(case, tmp_path, ambig=[1])
    assert len(held.keys) == 256
    held, in_file = bl.run_case(bl.ambig_all_go_case(), tmp_path, ambig=[2, 1])
    assert len(held.keys) == 0 and len(in_file.keys) == 0


@pytest.mark.parametrize("shards", [1, 3])
def test_ambiguity_twice_is_the_stricter_call(tmp_path, shards):
    """max_ambig = 3, then 1, on the same builder: what one call with 1 gives.  The second call is the only reader of the interior of the
    list offsets the first one rewrote."""
    case = bl.ambig_case([3, 1], 257)
    twice, _ = bl.run_case(case, tmp_path, shards=shards, ambig=[3, 1])
    once = bl.without_ambiguous(bl.held(case), case.anc, 1)
    assert np.array_equal(twice.keys, once.keys) and np.array_equal(twice.vals, once.vals) and 0 < len(once.keys) < 257


# ---- 10. chunk and batch borders ------------------------------------------------------------------------------------------------------
def big_sample(model, rng):
    """a strided sample, both ends of every hand-over chunk and file batch, and keys the table does not hold"""
    n = len(model.keys)
    at = np.concatenate([np.arange(0, n, 4099), [0, n - 1], [i + d for i in range(bl.FILE_BATCH, n, bl.FILE_BATCH) for d in (-1, 0, 1) if i + d < n]])
    return np.concatenate([model.keys[at], rng.integers(0, 1 << 32, size=100, dtype=np.uint64).astype(np.uint32)])


def run_big(case, tmp_path, shards):
    rng = np.random.default_rng(10)
    bs = [bl.make_builder(case, i, shards) for i in range(shards)]
    try:
        models = []
        for i, b in enumerate(bs):
            bl.add_batches(b, case)
            m = bl.held(case, i, shards)
            assert bl.finish(b) == (len(m.keys), len(m.vals))
            models.append(m)
        model = bl.whole(models) if shards > 1 else models[0]
        sample = big_sample(model, rng)
        name = str(tmp_path / case.name)
        bl.write(bs, name)
        bl.check_file(name, model, case)
        for make in (lambda: bl.load(bs), lambda: bl.open_file(name)):
            db = make()
            try:
                bl.check_sampled(db, model, sample)
                assert db.n_locations == len(model.vals)
            finally:
                db.close()
    finally:
        for b in bs:
            b.free()


def test_second_table_chunk_and_five_file_batches(tmp_path):
    """2^22 + 257 singleton keys in one builder: mc_build_table_add's second chunk begins at key 2^22, the writer makes five batches"""
    run_big(bl.singleton_case(bl.TABLE_CHUNK + 257, "chunk"), tmp_path, 1)


def test_a_file_batch_runs_on_across_shards(tmp_path):
    """2^20 + 1 keys over three shards: the first file batch takes keys of all three"""
    run_big(bl.singleton_case(bl.FILE_BATCH + 1, "batch"), tmp_path, 3)


# ---- 11. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_builder_as_it_was(tmp_path):
    rng = np.random.default_rng(11)
    case = bl.cap_case(7)
    L = bl.L()
    b = bl.make_builder(case)
    try:
        anc = np.arange(1, case.n_targets + 2, dtype=np.uint32)
        one = (np.array([9], np.uint32), np.array([2], np.uint8))
        bl.add_batches(b, case)
        # a location of a target the builder does not know: nothing of the batch is taken
        assert bl.add_locations(b, *one, [[0, 1], [0, len(case.windows)]], 4) == bl.MC_ERR_INVALID
        assert bl.add_locations(b, *one, [[0, 1], [0, 2]], 3) == bl.MC_ERR_INVALID               # target_bytes 3
        assert L.mc_build_remove_ambiguous(b.h, anc.ctypes.data, case.n_targets, 1, None) == bl.MC_ERR_STATE      # before finish
        model = bl.held(case)
        assert bl.finish(b) == (len(model.keys), len(model.vals))
        assert L.mc_build_remove_ambiguous(b.h, anc.ctypes.data, case.n_targets + 1, 1, None) == bl.MC_ERR_INVALID
        assert L.mc_build_remove_ambiguous(b.h, anc.ctypes.data, case.n_targets - 1, 1, None) == bl.MC_ERR_INVALID
        assert bl.add_locations(b, *one, [[0, 1], [0, 2]], 4) == bl.MC_ERR_STATE                  # after finish
        assert bl.add_existing_target(b, 99, 5) == bl.MC_ERR_STATE
        assert b.counts() == (len(model.keys), len(model.vals))
        name = str(tmp_path / "refused")
        bl.write([b], name)
        bl.check_file(name, model, case)
        bl.check_tables([b], name, model, model, case, bl.queries_for(rng, model, [9]))
    finally:
        b.free()
    # existing lists go in before new targets
    g = bl.random_genome(rng, 500)
    late = bl.Case("late", bl.SMALL_WINDOWS, [], real=[g])
    b = bl.make_builder(late)
    try:
        bl.add_batches(b, late)
        assert bl.add_locations(b, *one, [[0, 1], [0, 2]], 4) == bl.MC_ERR_STATE
        model = bl.held(late)
        assert bl.finish(b) == (len(model.keys), len(model.vals)) and len(model.keys) > 16
        name = str(tmp_path / "late")
        bl.write([b], name)
        bl.check_file(name, model, late)
    finally:
        b.free()
