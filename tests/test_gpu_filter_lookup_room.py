"""GPU: what gw_filter_count_kernel<LOOKUP> asks and sets once per read instead of once per place:

  * phase B into LDS asks the WAVE whether the four stores of a load register fit the 384 places -- reads that keep a little under and a
    little over 384 numbers, one of them crossing 384 inside such a group;
  * the list loads set of the places without a number only the register phase A asks -- lists whose last round holds 1, 3, 4, 5, 15 and
    16 numbers, reads of exactly 16, 17, 112 and 128 rounds (where the number of loads steps, and the full batch), one of 129 (deferred),
    reads without a list, of one list, of one list and one singleton, and a read of one load behind a read of eight on the same wave.

The collection is groups of IDENTICAL strains: every feature of a group's genome has a list of as many locations as the group has
strains, so a read's lists follow from where it is cut -- each shape is asserted from the oracle's sketch, lists and hit counts.
`filter_lookup` 1 against 0 on one context and every read against the C oracle, with and without taxon merging (both LOOKUP instances)."""
import numpy as np
import pytest

import cpuref
import scale_util
from metacache_amd import synth, synthdb
from test_gpu_filter_lookup_entries import KEEP, ROUNDS, STRIDE, W_, gw_bases, shape_of
from test_gpu_filter_lookup_pipeline import _both_orders, _compare, _open

pytestmark = pytest.mark.gpu
K = 2
LEN = 36 * STRIDE                                                # a group's genome: 36 windows
COPIES = (1, 10, 16, 17, 19, 20, 21, 22, 23, 24, 25, 31, 32, 100, 120)   # strains per group = locations per list
ENDS = {17: 1, 19: 3, 20: 4, 21: 5, 31: 15, 16: 16, 32: 16}     # group -> numbers in a list's last round
EXACT_ROUNDS = (16, 17, 112, 128, 129)
WAVES = 1024                                                     # filter_bpc 1: wave w walks the reads w, w + 1 024, ...


class World:
    pass


def collection():
    parts = [synthdb.phylogeny(1, 1, m, LEN, LEN, seed=7100 + m, div_strain=(0.0, 0.0)) for m in COPIES]
    group = np.concatenate([np.full(len(p.targets), i, dtype=np.int64) for i, p in enumerate(parts)])
    first = np.cumsum([0] + [len(p.targets) for p in parts])
    spec = synthdb.Phylogeny(np.concatenate([p.targets for p in parts]), group, group.copy(), len(parts), len(parts))
    return spec, {m: int(first[i]) for i, m in enumerate(COPIES)}


@pytest.fixture(scope="module")
def world():
    w = World()
    w.spec, first = collection()
    cs = synthdb.CpuSynth()
    genome = {m: cs.target(w.spec, t) for m, t in first.items()}
    for m, t in first.items():                                   # the strains of a group ARE one sequence
        assert m == 1 or np.array_equal(cs.target(w.spec, t + m - 1), genome[m]), m
    orc = cpuref.oracle()
    odb = scale_util.oracle_database(w.spec, None, threads=8, with_lineages=True)
    bases = gw_bases([range(LEN)] * len(w.spec.targets))
    w.memo, shapes = {}, {}

    def oracle(read, lowest=0):
        if (read, lowest) not in w.memo:
            w.memo[read, lowest] = odb.query(read, b"", K, lowest, 0)
        return w.memo[read, lowest]

    def shape(read):
        """the read's lists in lane order (found features only), its locations, rounds and loads, and the numbers the filter keeps
        (shape_of: without the filter's false positives -- a lower bound; H is the upper one)"""
        if read not in shapes:
            feats, counts = orc.sketch(read)
            sizes = [len(odb.lookup(int(f))) for i in range(len(feats)) for f in feats[i, :counts[i]]]
            sizes = [n for n in sizes if n]
            rounds = sum((n + 15) // 16 for n in sizes if n > 1)
            kept = shape_of(orc, odb, bases, read, b"", 2 + len(read) // STRIDE)["kept"] if sizes else 0
            shapes[read] = dict(sizes=sizes, H=sum(sizes), nent=len(sizes), rounds=rounds, loads=(rounds + 15) // 16, kept=kept)
        return shapes[read]

    def cut(m, start, n):
        return bytes(genome[m][start:start + n])

    def find(candidates, ok, what):
        for r in candidates:
            if ok(shape(r)):
                return r
        raise AssertionError(f"no read for: {what}")

    rng = np.random.default_rng(384)
    # ---- kept numbers around kKeep: reads of up to 150 bp of the groups of 16 .. 25 strains (a read cut anywhere finds 8 .. 19 of its
    # features, one that begins with a window of the genome 16 and more), some with substitutions
    w.around = []
    for m in (16, 19, 20, 21, 22, 23, 24, 25):
        for i in range(12):
            n = 150 - 3 * (i % 6)
            st = int(rng.integers(0, LEN - n)) if i % 2 else STRIDE * int(rng.integers(0, LEN // STRIDE - 2))
            w.around.append(bytes(synth.mutate(rng, genome[m][st:st + n], 0.01 * (i % 3 == 2))))
    # ---- every way a list can end, in reads of two to four loads
    w.ends = {m: [cut(m, int(rng.integers(0, LEN - 150)), 150) for _ in range(6)] for m in ENDS}
    # ---- exact numbers of rounds: one whole window of a group (16 lists of 1, 7 or 8 rounds), for 17 and 129 with a piece of the group of
    # ten strains behind it that brings exactly one more list of one round
    one_window = {16: 16, 17: 16, 112: 100, 128: 120, 129: 120}
    w.exact = {}
    for want, m in one_window.items():
        whole = [cut(m, j * STRIDE, W_) for j in range(LEN // STRIDE - 1)]
        tail = [b""] if want in (16, 112, 128) else [cut(10, o, n) for o in range(0, LEN - 48, 37) for n in (17, 22, 27, 32)]
        w.exact[want] = find((a + b for a in whole for b in tail), lambda s, want=want: s["rounds"] == want and s["H"] <= 2048 and s["nent"] <= 64, f"{want} rounds")
    # ---- degenerate reads
    w.singles = find((cut(1, o, 150) for o in range(0, LEN - 150, 50)), lambda s: s["nent"] >= 8 and set(s["sizes"]) == {1}, "singletons only")
    short100 = [cut(100, o, n) for o in range(0, LEN - 40, 11) for n in (18, 22, 26)]
    w.one_list = find(short100, lambda s: s["sizes"] == [100], "one list and no singleton")
    short1 = [cut(1, o, 24) for o in range(0, LEN - 24, 13)]
    w.list_and_single = find((a + b for a in short100[:120] for b in short1[:40]), lambda s: sorted(s["sizes"]) == [1, 100], "one singleton and one list")
    w.oracle, w.shape = oracle, shape
    yield w
    odb.close()


LOWEST = pytest.mark.parametrize("lowest", [0, 4])               # 4: candidates merged at a taxon rank -- the kernel's other instance


def _run_and_compare(world, reads, lowest, reverse_too=False):
    import torch
    dev = torch.device("cuda", 0)
    db = _open(world)
    for order in (reads, reads[::-1]) if reverse_too else (reads,):
        got, gstat, want, wstat = _both_orders(db, order, dev, lowest)
        _compare(world, order, got, gstat, want, wstat, lowest)
    db.close()


@LOWEST
def test_kept_numbers_around_the_room_in_lds(world, lowest):
    """reads that keep at most 320, 321 .. 384 and 385 .. 448 numbers: the last group of four stores that fits, the first that does not
    (left out as a whole: the read is filtered again into the pool), and a count that passes 384 inside a group"""
    sh = [world.shape(r) for r in world.around]
    own = [s for s in sh if s["H"] > 64 and s["rounds"] <= ROUNDS]
    print("kept (lower bound) / locations:", sorted((s["kept"], s["H"]) for s in own))
    assert any(s["H"] <= KEEP - 64 for s in own)
    assert any(KEEP - 64 < s["kept"] and s["H"] <= KEEP for s in own)
    assert any(KEEP < s["kept"] and s["H"] <= KEEP + 64 for s in own)
    # passes 384 inside a group of stores: a store holds 64 numbers at most and the count does not end on 384
    assert any(KEEP < s["kept"] and s["H"] < KEEP + 64 for s in own)
    assert sum(s["kept"] > KEEP for s in own) >= 8 and sum(s["H"] <= KEEP for s in own) >= 8
    _run_and_compare(world, world.around, lowest, reverse_too=True)


def _special_reads(world):
    reads = [r for m in ENDS for r in world.ends[m]] + [world.exact[n] for n in EXACT_ROUNDS]
    return reads + [world.singles, world.one_list, world.list_and_single]


@LOWEST
def test_list_ends_round_counts_and_degenerate_reads(world, lowest):
    for m, last in ENDS.items():                                 # every list of the read ends this way, in its first load and in its last
        full = [s for s in map(world.shape, world.ends[m]) if set(s["sizes"]) == {m} and s["loads"] >= 2 and s["rounds"] <= ROUNDS]
        assert full and (m - 1) % 16 + 1 == last, (m, last)
    for n in EXACT_ROUNDS:
        assert world.shape(world.exact[n])["rounds"] == n
    assert [world.shape(world.exact[n])["loads"] for n in (16, 17, 112, 128)] == [1, 2, 7, 8]
    assert world.shape(world.exact[129])["rounds"] > ROUNDS       # deferred by its rounds alone
    assert world.shape(world.one_list)["H"] > 64 and world.shape(world.list_and_single)["H"] > 64   # the filter's class
    _run_and_compare(world, _special_reads(world), lowest, reverse_too=True)


@LOWEST
def test_a_read_of_one_load_on_the_wave_of_a_read_of_eight(world, lowest):
    """2 048 reads: wave w walks the reads w and w + 1 024.  Every fourth wave takes a read that fills all eight load registers and then
    one that uses a single register; the other waves walk the rest of this file's reads.  Then the batch reversed: the other order"""
    shape = world.shape
    specials = _special_reads(world) + world.around
    eight = [r for r in specials if shape(r)["loads"] == 8 and shape(r)["rounds"] <= ROUNDS and shape(r)["H"] <= 2048]
    one = [r for r in specials if shape(r)["loads"] == 1 and shape(r)["H"] > 64]
    assert eight and len(one) >= 2, (len(eight), len(one))
    first = [eight[(i // 4) % len(eight)] if i % 4 == 0 else specials[i % len(specials)] for i in range(WAVES)]
    second = [one[(i // 4) % len(one)] if i % 4 == 0 else specials[(i * 7 + 3) % len(specials)] for i in range(WAVES)]
    reads = first + second
    pairs = sum(shape(reads[i])["loads"] == 8 and shape(reads[i + WAVES])["loads"] == 1 for i in range(WAVES))
    assert pairs >= WAVES // 4, pairs
    _run_and_compare(world, reads, lowest, reverse_too=True)
