"""GPU: gw_filter_count_kernel<LOOKUP> writes a read's hand-over entries (ws.psize / ws.ppay) only when the read leaves the kernel;
a read it finishes has none, and step D takes its entries from the index again.  Every exit that now re-derives the entries from the
read's number has to be reached, so the collection is made for the routes, and a NumPy classifier of the oracle's all-hits lists says
which route a read takes -- a case that does not reach one of its routes with at least 8 reads fails:

  1  finished, K candidates of two or more hits              5  early deferral (more than 2 048 locations or 128 rounds)
  2  finished through step D (places left for single hits)   6  late deferral (at most 384 kept numbers, more than 256 distinct)
  3  taxon merging with places left -> exact wave kernel     7  more than 384 kept numbers -> pool, gw_count_kernel
  4  two best ranges in one target -> exact wave kernel      8  other classes: no hit, up to 24 locations, 25 .. 64

Candidates and all four statistics words against `filter_lookup` 0 on the same context, candidates and hit counts against the C oracle."""
import numpy as np
import pytest

import cpuref
from metacache_amd import api, synth
from test_gpu_filter_lookup import _device_batch, _run, _as_cands, _same_rows
from test_gpu_parity import cands_equal

pytestmark = pytest.mark.gpu

GAP = 1024                                                      # kernels.h: kGwGap
K_, S_, W_, STRIDE = 16, 16, 127, 112
SMALL_H, ROUNDS, KEEP, DISTINCT, LANE_HITS = 2048, 128, 384, 256, 24   # gw_kernels.hip: kGwSmallH, kGwRounds, kKeep, kList of the fused counting; kernels.hip: MC_LANE_HITS
MIN_PER_ROUTE = 8


def windows_of(length):
    """windows of a target (hash_dna.hpp:54-75)"""
    if length <= W_:
        return 1 if length >= K_ else 0
    nw = (length - W_) // STRIDE + 1
    if nw * STRIDE < length and length - nw * STRIDE >= K_:
        nw += 1
    return nw


def chimera(rng, base, L):
    """a random genome that carries L characters of `base` in every stretch of 112, at a place of its own: it shares a feature with a
    window of base now and then, hardly ever two"""
    g = synth.random_genome(rng, len(base))
    for s0 in range(0, len(base) - STRIDE, STRIDE):
        o = s0 + int(rng.integers(0, STRIDE - L))
        g[o:o + L] = base[o:o + L]
    return g


def collection(seed=20250, three_n=6, three_L=17, far_n=380, far_L=17):
    """one species; groups of targets of 20 kbp made for the routes (and three targets of 230 kbp that carry a segment twice,
    1 786 windows apart: farther than the gap between two targets' window numbers, which is what makes two regions of one target)
    -> (targets, {group: the genomes its reads are drawn from})"""
    rng = np.random.default_rng(seed)
    genomes, groups = [], {}

    def add(name, base, rates, chimeras=0, L=0):
        strains = [synth.mutate(rng, base, r) if r else base.copy() for r in rates]
        groups[name] = strains if strains else [base]
        genomes.extend(strains)
        for _ in range(chimeras):
            genomes.append(chimera(rng, base, L))

    add("few", synth.random_genome(rng, 20_000), [0, 0.002])                                       # 8: lists of up to 64 locations
    add("eight", synth.random_genome(rng, 20_000), [0] + [0.002] * 7)                               # 1: eight candidates of many hits
    add("three", synth.random_genome(rng, 20_000), [0, 0.002, 0.002], three_n, three_L)             # 2: three strong ones, single hits beside them
    twice = synth.random_genome(rng, 230_000)
    twice[201_000:201_400] = twice[1_000:1_400]
    add("twice", twice, [0, 0.004, 0.004])                                                          # 4
    add("sixty", synth.random_genome(rng, 20_000), [0] + [0.002] * 59)                              # 5 (300 bp), 7 (150 bp)
    add("far", synth.random_genome(rng, 20_000), [], far_n, far_L)                                  # 6: hundreds of targets with a hit in two or three windows each (their common source is no target)
    return genomes, groups


def make_reads(genomes, groups, seed=7):
    rng = np.random.default_rng(seed)
    out = []

    def draw(group, n, length, sub, lo=0, hi=None):
        src = groups[group]
        for _ in range(n):
            g = src[int(rng.integers(0, len(src)))]
            st = int(rng.integers(lo, (hi if hi is not None else len(g) - length)))
            r = synth.mutate(rng, g[st:st + length], sub, 0.001 if sub else 0.0)
            if rng.random() < 0.5:
                r = synth.revcomp(r)
            out.append(bytes(r))

    draw("eight", 30, 150, 0.01)
    draw("three", 40, 239, 0.01)
    draw("twice", 20, 150, 0.01, 1_000, 1_250)
    draw("twice", 20, 150, 0.01, 201_000, 201_250)
    draw("twice", 10, 150, 0.01)
    draw("sixty", 30, 150, 0.01)
    draw("sixty", 30, 330, 0.01)
    draw("sixty", 10, 351, 0.06)
    draw("far", 60, 463, 0.0)
    draw("few", 20, 150, 0.01)
    draw("few", 20, 100, 0.01)
    draw("few", 20, 60, 0.03)
    out += [bytes(synth.random_genome(rng, L)) for L in (150,) * 10 + (240, 351)]
    return [out[i] for i in rng.permutation(len(out))]


def make_pairs(genomes, groups, seed=11):
    """mates of 120 bp, 150 .. 200 bp apart: one window each, a window range of 4"""
    rng = np.random.default_rng(seed)
    a, b = [], []
    for group, n in (("eight", 30), ("three", 30), ("sixty", 30), ("few", 30), ("far", 20), ("twice", 10)):
        src = groups[group]
        for _ in range(n):
            g = src[int(rng.integers(0, len(src)))]
            st = int(rng.integers(0, len(g) - 400)); d = int(rng.integers(150, 200))
            a.append(bytes(synth.mutate(rng, g[st:st + 120], 0.01, 0.001)))
            b.append(bytes(synth.revcomp(synth.mutate(rng, g[st + d:st + d + 120], 0.01, 0.001))))
    a += [bytes(synth.random_genome(rng, 120)) for _ in range(10)]
    b += [bytes(synth.random_genome(rng, 120)) for _ in range(10)]
    p = rng.permutation(len(a))
    return [a[i] for i in p], [b[i] for i in p]


def gw_bases(genomes):
    base = np.zeros(len(genomes) + 1, dtype=np.int64)
    base[0] = GAP
    for t, g in enumerate(genomes):
        base[t + 1] = base[t] + windows_of(len(g)) + GAP
    return base


def shape_of(orc, odb, bases, read, mate, max_win):
    """what the kernels' decisions depend on, from the oracle's sketch, lists and all-hits: locations, found features, rounds, the kept
    numbers of the filter (without its few false positives) and the distinct ones among them, and the counting's K rounds on them"""
    nent = rounds = H = 0
    for s in (read, mate):
        if not s:
            continue
        feats, counts = orc.sketch(s)
        for w in range(len(feats)):
            for f in feats[w, :counts[w]]:
                n = len(odb.lookup(int(f)))
                H += n; nent += n > 0; rounds += (n + 15) // 16 if n > 1 else 0
    h, _ = odb.query(read, mate or b"", 1, 0, 0)
    assert len(h) == H, (len(h), H)
    gw = np.sort(bases[h["tgt"].astype(np.int64)] + h["win"].astype(np.int64))
    D = max(max_win - 1, 1)
    A = max(8, int(64 * D - 1).bit_length())
    blk, cnt = np.unique(gw >> A, return_counts=True)
    twice = cnt[np.searchsorted(blk, gw >> A)] >= 2
    edge = ((gw + (max_win - 1 if max_win > 1 else 0)) & ((1 << A) - 1)) < 2 * (max_win - 1 if max_win > 1 else 0)
    kept = gw[twice | edge]
    nums, c = np.unique(kept, return_counts=True)
    # hits of the window range that ends in each number
    R = np.array([c[(nums <= g) & (nums > g - max_win)].sum() for g in nums], dtype=np.int64)
    return dict(H=H, nent=int(nent), rounds=int(rounds), kept=len(kept), distinct=len(nums), nums=nums, R=R)


def route_of(sh, bases, K, tax, max_win):
    H = sh["H"]
    if H == 0:
        return "8-none"
    if H <= 64:
        return "8-lane" if H <= LANE_HITS else "8-mid"
    if H > SMALL_H or sh["rounds"] > ROUNDS or sh["nent"] > 64:
        return "5"
    if max_win > 8:
        return "other"
    if sh["kept"] > KEEP:
        return "7"
    if sh["kept"] > KEEP - 24:                                  # (the filter's false positives decide)
        return "border"
    if sh["distinct"] > DISTINCT:
        return "6"
    if sh["distinct"] > DISTINCT - 12:
        return "border"
    # the K rounds: the most hits, the smallest number among them; its region (taxon merging: everything, one species) is struck
    nums, R = sh["nums"], sh["R"].copy()
    live = np.ones(len(nums), dtype=bool)
    targets, strong = [], 0
    for _ in range(K):
        if not live.any() or R[live].max() == 0:
            break
        m = R[live].max()
        g = nums[live & (R == m)].min()
        strong += m >= 2
        targets.append(int(np.searchsorted(bases, g, side="right") - 1))
        live &= False if tax else (np.abs(nums - g) > GAP)
    if not tax and len(set(targets)) < len(targets):
        return "4"
    if strong >= K:
        return "1"
    return "3" if tax else "2"


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    import os
    old = os.environ.get("MC_COMPACT_LOCATIONS")
    os.environ["MC_COMPACT_LOCATIONS"] = "1"
    genomes, groups = collection()
    name = str(tmp_path_factory.mktemp("entries") / "routes")
    bld = api.Builder(target_id_bytes=4, max_candidates=4)
    for i, g in enumerate(genomes):
        bld.add_target(g, f"E{i:04d}.1", parent_taxid=1000)
    bld.finish(load=False)
    bld.write(name, [(1, 1, 20, "root"), (1000, 1, 4, "sp0")])
    bld.free()
    orc = cpuref.oracle()
    odb = orc.open(name)
    bases = gw_bases(genomes)
    singles = make_reads(genomes, groups)
    p1, p2 = make_pairs(genomes, groups)
    shapes = {}

    def shape(read, mate, max_win):                             # (computed once per read and window range, shared by the cases)
        key = (read, mate, max_win)
        if key not in shapes:
            shapes[key] = shape_of(orc, odb, bases, read, mate, max_win)
        return shapes[key]
    yield dict(name=name, odb=odb, bases=bases, singles=singles, pairs=(p1, p2), shape=shape)
    odb.close()
    if old is None:
        os.environ.pop("MC_COMPACT_LOCATIONS", None)
    else:
        os.environ["MC_COMPACT_LOCATIONS"] = old


def _check(world, reads, mates, K, lowest, want_routes, repeat=1, filter_bpc=0):
    import torch
    dev = torch.device("cuda", 0)
    odb, bases = world["odb"], world["bases"]
    reads = list(reads) * repeat
    mates = None if mates is None else list(mates) * repeat
    db = api.Database.open(world["name"], max_candidates=K, copy_allhits=0)
    try:
        assert db.table_layout()["location_bytes"] == 4
        db.set_tuning("direct_index", 1)
        assert db.table_layout()["direct_index"]
        db.set_tuning("big_min", 0)
        if filter_bpc:
            db.set_tuning("filter_bpc", filter_bpc)
        batch = _device_batch(reads, mates, 0, dev)
        db.set_tuning("filter_lookup", 0)
        want, wstat = _run(db, batch, K, lowest)
        # the same reads in reverse order: the entries that run left in ws.psize / ws.ppay, which would stand in for entries the new
        # kernel fails to write, now lie in other reads' slots
        _run(db, _device_batch(reads[::-1], None if mates is None else mates[::-1], 0, dev), K, lowest)
        db.set_tuning("filter_lookup", 1)
        db.timing(True); db.timing_reset()
        got, gstat = _run(db, batch, K, lowest)
        ran = {k: db.timing_get(k)[1] for k in ("sketch_probe", "sketch_lane", "gw_filter_count")}
        db.timing(False)
        assert ran["sketch_lane"] > 0 and ran["gw_filter_count"] > 0 and ran["sketch_probe"] == 0, ran
    finally:
        db.close()
    reached, single_hit_rows, routes = {}, 0, []
    expected = {}
    for i, r in enumerate(reads):
        m = mates[i] if mates is not None else b""
        mw = 2 + (len(r) + len(m)) // STRIDE
        if (r, m) not in expected:
            expected[(r, m)] = odb.query(r, m, K, lowest, 0)
        h, e = expected[(r, m)]
        route = route_of(world["shape"](r, m, mw), bases, K, lowest != 0, mw)
        reached[route] = reached.get(route, 0) + 1
        routes.append(route)
        single_hit_rows += route == "2" and bool((e["hits"] == 1).any())
        assert int(gstat[i, 0]) == len(h), (route, i, len(r), gstat[i], len(h))
        assert cands_equal(_as_cands(got[i]), e[:K]), (route, i, len(r), got[i], e)
        assert _same_rows(got[i], want[i]), (route, i, len(r), got[i], want[i])
        assert np.array_equal(gstat[i], wstat[i]), (route, i, len(r), gstat[i], wstat[i])
    print("routes reached:", dict(sorted(reached.items())), "rows with a single-hit entry on route 2:", single_hit_rows)
    for route in want_routes:
        assert reached.get(route, 0) >= MIN_PER_ROUTE * repeat, (route, reached)
    if "2" in want_routes:
        assert single_hit_rows >= MIN_PER_ROUTE, single_hit_rows
    return routes


OTHER = ["8-none", "8-lane", "8-mid"]


@pytest.mark.parametrize("K,lowest,routes", [(2, 0, ["1", "4", "5", "6", "7"]), (3, 0, ["1", "4", "5", "6", "7"]),
                                             (4, 0, ["1", "2", "4", "5", "6", "7"]), (3, 4, ["3", "5", "6", "7"])])
def test_single_reads_on_every_exit_that_rederives_the_entries(world, K, lowest, routes):
    _check(world, world["singles"], None, K, lowest, routes + OTHER)


def test_two_ranges_of_one_target_last_of_a_walk_and_followed_by_other_reads(world):
    """the grid cut to 256 blocks of four waves and the reads four times over (more than 1 024): a wave walks reads w and w + 1 024 --
    the candidates of a read wait for the wave's next one (GwPend), where `two winners of one target` turns up for the read BEFORE
    the current one, and behind the loop for the last one.  Route 4 reads must stand in both places: as the first read of a walk whose
    second read enters the counting (routes 1, 4, 6: it finishes the waiting read), and as the last read of a walk."""
    n = len(world["singles"])
    waves = 1024
    assert 3 * n < waves < 4 * n, n
    routes = _check(world, world["singles"], None, 2, 0, ["1", "4", "5", "6", "7"] + OTHER, repeat=4, filter_bpc=1)
    followed = sum(routes[i] == "4" and routes[i + waves] in ("1", "4", "6") for i in range(4 * n - waves))
    last = sum(routes[i] == "4" for i in range(4 * n - waves, 4 * n))
    print("route 4 reads followed by a counted read of their wave:", followed, "last of their wave's walk:", last)
    assert followed >= 2 and last >= MIN_PER_ROUTE, (followed, last)


def test_pairs_with_a_window_range_of_four(world):
    p1, p2 = world["pairs"]
    _check(world, p1, p2, 2, 0, ["1", "7", "8-none"])
