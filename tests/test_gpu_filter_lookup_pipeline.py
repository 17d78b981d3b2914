"""GPU: order and depth of the per-wave pipeline of gw_filter_count_kernel<LOOKUP> (raw metadata three reads ahead, features
two, index entries one).  What test_gpu_filter_lookup.py and test_gpu_filter_lookup_entries.py do not reach: waves with one to six reads
(every stage falls behind the end of the batch at some depth for some wave), and every way out of a read in front of a read the kernel
finishes -- the stages a read skips have to be run for the reads behind it all the same.

One species of 48 strains of 20 kbp, `filter_bpc` 1 (a grid of min(256, ceil(n / 4)) blocks of four waves: wave w walks the reads
w, w + 1 024, ...), mc_query_device(MC_DEFER_TAIL) + mc_query_finish with `direct_index` 1: `filter_lookup` 1 against `filter_lookup` 0 on
the same context (candidates, all four statistics words) and against the C oracle."""
import numpy as np
import pytest

import scale_util
from metacache_amd import synth, synthdb
from test_gpu_filter_lookup import TIMERS, _as_cands, _device_batch, _run, _same_rows
from test_gpu_parity import cands_equal

pytestmark = pytest.mark.gpu
K = 2
WAVES = 1024                                                     # filter_bpc 1: 256 blocks of four waves once the batch has 1 021 reads
ENDS = (1, 3, 4, 5, 1023, 1024, 1025, 2 * 1024 + 1, 3 * 1024 + 1, 4 * 1024 + 1, 5 * 1024 + 3)
# what one wave sees, in order (own: a read of the filter's class, which the kernel finishes)
WALK = ("own", "long", "nowin", "own", "nohit", "other", "own", "long", "nowin", "own")


class World:
    pass


@pytest.fixture(scope="module")
def world():
    w = World()
    rng = np.random.default_rng(909)
    w.spec = synthdb.phylogeny(1, 1, 48, 20_000, 20_000, seed=9048, div_strain=(0.002, 0.01))
    cs = synthdb.CpuSynth()

    def draw(seed, length, sub, count):
        P = synthdb.read_params(w.spec, seed, read_len=length, sub_rate=sub)
        return [bytes(r[:length]) for r in cs.reads(w.spec, P, 0, count)]

    odb = scale_util.oracle_database(w.spec, None, threads=8, with_lineages=True)
    w.memo = {}

    def oracle(read, lowest=0):
        if (read, lowest) not in w.memo:
            w.memo[read, lowest] = odb.query(read, b"", K, lowest, 0)
        return w.memo[read, lowest]

    def hits(read):
        return len(oracle(read)[0])

    own = [r for r in draw(31, 150, 0.01, 48) + draw(32, 150, 0.04, 16) if hits(r) > 64]
    other = [r for sub in (0.10, 0.15, 0.20, 0.25) for r in draw(40 + int(sub * 100), 150, sub, 48) if 1 <= hits(r) <= 64]
    nohit = [r for r in (bytes(synth.random_genome(rng, 150)) for _ in range(8)) if hits(r) == 0]
    long_ = draw(51, 512, 0.01, 8)                                # 80 features: more than a wave has lanes -- not this kernel's
    nowin = [r[:15] for r in draw(52, 150, 0.01, 8)]             # shorter than a k-mer: no window, no feature
    assert len(own) >= 32 and len(other) >= 4 and len(nohit) >= 4, (len(own), len(other), len(nohit))
    assert all(hits(r) == 0 for r in nowin)
    w.kinds = {"own": own, "other": other, "nohit": nohit, "long": long_, "nowin": nowin}
    w.oracle = oracle
    w.hits = hits
    yield w
    odb.close()


def _open(world):
    db, _ = synthdb.build_database(world.spec, shards=1, max_candidates=K)
    assert db.table_layout()["location_bytes"] == 4
    db.set_lineages(world.spec.lineages())
    db.set_tuning("direct_index", 1)
    assert db.table_layout()["direct_index"]
    db.set_tuning("big_min", 0)
    db.set_tuning("filter_bpc", 1)
    return db


def _both_orders(db, reads, dev, lowest):
    """the batch with the default order of the kernels and with the lookups in the filter kernel, on the same context"""
    batch = _device_batch(reads, None, 0, dev)
    db.set_tuning("filter_lookup", 0)
    want, wstat = _run(db, batch, K, lowest)
    db.set_tuning("filter_lookup", 1)
    db.timing(True); db.timing_reset()
    got, gstat = _run(db, batch, K, lowest)
    ran = {k: db.timing_get(k)[1] for k in TIMERS}
    db.timing(False)
    assert ran["sketch_lane"] > 0 and ran["gw_filter_count"] > 0 and ran["sketch_probe"] == 0, ran
    return got, gstat, want, wstat


def _compare(world, reads, got, gstat, want, wstat, lowest):
    """every read against the other order of the kernels and against the oracle (memoised: the batches repeat some 130 reads)"""
    assert np.array_equal(gstat, wstat), np.flatnonzero((gstat != wstat).any(axis=1))[:8]
    used = want[:, :, 1] > 0                                     # (an entry with hits == 0 is unused: its other fields are not part of the result)
    same = np.array_equal(got[:, :, 1], want[:, :, 1]) and np.array_equal(got[used], want[used])
    if not same:
        for i in range(len(reads)):
            assert _same_rows(got[i], want[i]), (i, len(reads[i]), got[i], want[i])
    for i in range(len(reads)):
        h, e = world.oracle(reads[i], lowest)
        assert int(gstat[i, 0]) == len(h), (i, len(reads[i]), gstat[i], len(h))
        assert cands_equal(_as_cands(got[i]), e), (i, len(reads[i]), got[i], e)


LOWEST = pytest.mark.parametrize("lowest", [0, 4])               # 4: candidates merged at a taxon rank -- the kernel's other instance


@LOWEST
def test_waves_with_one_to_six_reads(world, lowest):
    """batches whose last reads leave every stage of the pipeline without a read at some depth: 1 .. 5 reads (waves with one read, most
    waves of the grid's blocks with none), 1 023 .. 1 025 (the second read of wave 0 only), k x 1 024 + 1 or 3 (one or three waves with
    k + 1 reads, the others with k).  Nearly all reads are the filter's own, so the stages run at full depth; every 13th is of another kind."""
    import torch
    dev = torch.device("cuda", 0)
    own = world.kinds["own"]
    rest = [world.kinds[k][0] for k in ("long", "nowin", "nohit", "other")]
    db = _open(world)
    for n in ENDS:
        reads = [rest[(i // 13) % 4] if i % 13 == 12 else own[(i * 7 + n) % len(own)] for i in range(n)]
        got, gstat, want, wstat = _both_orders(db, reads, dev, lowest)
        _compare(world, reads, got, gstat, want, wstat, lowest)
    db.close()


def _walk_batch(world):
    """ten reads per wave; wave 0 and wave 517 see WALK, the other waves the filter's own reads with a read of another kind now and then"""
    kinds = world.kinds
    n = len(WALK) * WAVES
    reads, marked = [None] * n, {}
    for i in range(n):
        wave, step = i % WAVES, i // WAVES
        if wave in (0, 517):
            kind = WALK[step]
            reads[i] = kinds[kind][(step + wave) % len(kinds[kind])]
            marked[i] = kind
        else:
            reads[i] = kinds["own"][(i * 5 + step) % len(kinds["own"])] if i % 29 else kinds["other"][i % len(kinds["other"])]
    # each kind is where it is meant to be, by the oracle's hit counts and the reads' lengths
    for i, kind in marked.items():
        h, length = world.hits(reads[i]), len(reads[i])
        ok = {"own": h > 64 and length == 150, "other": 1 <= h <= 64 and length == 150, "nohit": h == 0 and length == 150,
              "long": length == 512 and h > 0, "nowin": length == 15 and h == 0}[kind]
        assert ok, (i, kind, h, length)
    return reads, marked


@LOWEST
def test_every_way_out_of_a_read_in_front_of_an_own_read(world, lowest):
    """wave 0 and a wave in the middle walk: own, more than 64 features, no window, own, no hit, another class, own, two reads that are
    not the kernel's, own as the wave's last -- then the same batch in reverse order on the same context, so that nothing the first run
    left behind can stand in for work the second fails to do"""
    import torch
    dev = torch.device("cuda", 0)
    reads, marked = _walk_batch(world)
    db = _open(world)
    for order in (reads, reads[::-1]):
        got, gstat, want, wstat = _both_orders(db, order, dev, lowest)
        _compare(world, order, got, gstat, want, wstat, lowest)
    db.close()
