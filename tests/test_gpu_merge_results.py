"""GPU: mc_merge_results_* (merge_results.hip), the device form and MC_MERGE_HOST, against the witness (merge_results_ref), which
test_merge_results_witness_cpu.py holds to the reference's own `metacache merge`.

  * the four golden part files and the generated ones, two and three files in both orders: lists, header places, list count, status and
    assignments (hitmin 5 / 3, hitdiff 1 / 0.5, lowest species / genus, highest family / domain);
  * files built around the tile T = api.merge_results_tile(); the same file in two and three pieces (MC_MERGE_CONTINUE) cut at every line start;
  * one irregular range per clause of the line rule and a duplicate across pieces: verdict and offence as the witness's, the store
    bit-identical to what it was; MC_MERGE_OVERFLOW one query short; two mergers on two streams at once.
Every device output sits between guard zones.  A regular input that the device refuses FAILS here: there is no skip and no fall-back."""
import numpy as np
import pytest

import merge_results_cases as cases
import merge_results_ref as ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
FILL64 = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])
OPTIONS = [dict(hitmin=5, hitdiff=1.0, lowest=4, highest=19), dict(hitmin=3, hitdiff=0.5, lowest=6, highest=10)]   # (lowest is checked and not used)


@pytest.fixture(scope="module")
def toy():
    return cases.toy_table()


@pytest.fixture(scope="module")
def rm(toy):
    ids, lin, rank, _ = toy
    m = api.ResultMerger()
    m.set_taxa(lin, rank, ids)
    yield m
    m.close()


@pytest.fixture(scope="module")
def files(toy):
    ids, _, rank, _ = toy
    out = {"g_" + k: v for k, v in cases.generated_files(ids, rank).items()}
    for name in ("part0.txt", "part1.txt", "part0_genus.txt", "part1_genus.txt"):
        out[name] = cases.golden_part(name)
    return out


def column(data):
    return cases.tophits_column(data)


class Guarded:
    """a device array of `elems` 8-byte words between two guard zones"""

    def __init__(self, elems):
        import torch
        self.torch, self.elems = torch, elems
        self.t = torch.full((GUARD + elems + GUARD,), FILL64, dtype=torch.int64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()                               # (the fill runs on torch's stream, the library on the context's)

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * GUARD

    def get(self, dtype=np.uint64):
        self.torch.cuda.synchronize()
        raw = self.t.cpu().numpy().view(np.uint8)
        assert np.all(raw[:8 * GUARD] == FILL) and np.all(raw[8 * (GUARD + self.elems):] == FILL), "bytes outside the array were written"
        return raw[8 * GUARD:8 * (GUARD + self.elems)].view(dtype).copy()


def to_device(data):
    import torch
    t = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(torch.device("cuda", 0))
    assert t.data_ptr() % 16 == 0
    return t


def stage(data):
    """a range, its workspace and its Guarded status on the device, filled and waited for -> (status, (bytes, workspace, its size))"""
    import torch
    d = to_device(data)
    wsb = api.merge_results_scratch_bytes(len(data))
    ws = torch.full((wsb + GUARD,), FILL, dtype=torch.uint8, device=d.device)
    st = Guarded(8)
    torch.cuda.synchronize()
    return st, (d, ws, wsb)


def enqueue(rm, staged, col, file_lines=0, cont=False, stream=0):
    """mc_merge_results_add on what stage() made: nothing is waited for"""
    st, (d, ws, wsb) = staged
    rm.add_device(d.data_ptr(), d.numel(), col, status_ptr=st.ptr, workspace_ptr=ws.data_ptr(), workspace_bytes=wsb, file_lines=file_lines, cont=cont, stream=stream)


def add_on_device(rm, data, col, file_lines=0, cont=False, stream=0):
    """-> the Guarded status and what has to stay alive until the stream is through"""
    staged = stage(data)
    enqueue(rm, staged, col, file_lines, cont, stream)
    return staged


def check_workspace(keep):
    d, ws, wsb = keep
    assert np.all(ws.cpu().numpy()[wsb:] == FILL), "bytes behind the workspace were written"


def store_on_device(rm, stream=0):
    """lists, header places and the count through the device form of mc_merge_results_lists, between guards"""
    cap, K = rm.capacity, rm.max_candidates
    L, P, N = Guarded(cap * K), Guarded((3 * cap + 1) // 2), Guarded(1)
    rm.lists_device(0, cap, lists_ptr=L.ptr, places_ptr=P.ptr, num_ptr=N.ptr, stream=stream)
    return L.get(np.uint32).reshape(cap, K, 2), P.get(np.uint32)[:3 * cap].reshape(cap, 3), int(N.get()[0])


def assert_store(rm, want, what, device=True):
    if device:
        lists, places, count = store_on_device(rm)
    else:
        lists, places, count = rm.lists()
    assert count == want.count, what
    assert np.array_equal(lists, want.lists_array()), what
    assert np.array_equal(places, want.header_places()), what


def assert_votes(rm, want, what, device=True):
    for o in OPTIONS:
        exp = want.classify(o["hitmin"], o["hitdiff"], o["highest"])
        opt = api.classify_options(hitmin=o["hitmin"], hitdiff=o["hitdiff"], lowest=o["lowest"], highest=o["highest"])
        if device:
            out = Guarded(rm.capacity)
            rm.classify_device(opt, 0, rm.capacity, out.ptr)
            got = out.get(np.uint32).reshape(rm.capacity, 2)
        else:
            got = rm.classify(opt)
        assert np.array_equal(got[:, 0], exp[:, 0]), (what, o)
        assert np.array_equal(got[:, 1] & 0xFF, exp[:, 1]) and np.array_equal(got[:, 1] >> 8, exp[:, 2]), (what, o)


SETS = [(("part0.txt", "part1.txt"), 4, 4), (("part1.txt", "part0.txt"), 3, 4), (("part0_genus.txt", "part1_genus.txt"), 2, 6),
        (("part1_genus.txt", "part0_genus.txt"), 2, 6), (("g_a", "g_b"), 8, 4), (("g_b", "g_a"), 1, 4), (("g_a", "g_b", "g_c"), 8, 4),
        (("g_c", "g_b", "g_a"), 8, 4), (("g_a", "g_b", "g_c"), 1, 0), (("g_c", "g_a", "g_b"), 3, 0)]


@pytest.mark.parametrize("device", [True, False], ids=["device", "host"])
@pytest.mark.parametrize("names,max_cand,merge_below", SETS, ids=lambda v: "+".join(v) if isinstance(v, tuple) else str(v))
def test_files_equal_the_witness(rm, toy, files, names, max_cand, merge_below, device):
    ids, lin, rank, _ = toy
    want = ref.Merger(ids, lin, rank, 700, max_cand, merge_below)
    rm.begin(700, max_cand, merge_below)
    for name in names:
        data = files[name]
        exp = want.add(data, column(data))
        assert exp[5] == ref.OK
        if device:
            st, keep = add_on_device(rm, data, column(data))
            got = [int(x) for x in st.get()]
            check_workspace(keep)
        else:
            got = rm.add(data, column(data))
        assert got[5] == api.MERGE_OK, f"{name}: a regular file was refused: verdict {got[5]}, offence {got[6]}"
        assert got == exp, name
    assert_store(rm, want, names, device)
    assert_votes(rm, want, names, device)


def test_file_lines_given_by_the_caller(rm, toy, files):
    ids, lin, rank, _ = toy
    want = ref.Merger(ids, lin, rank, 100, 4, 4)
    rm.begin(100, 4, 4)
    for name, lines in (("g_a", 0), ("g_b", 70), ("g_c", 20)):       # more than the file holds, fewer than its largest id
        exp = want.add(files[name], cases.COL, file_lines=lines)
        assert rm.add(files[name], cases.COL, file_lines=lines) == exp and exp[5] == ref.OK
    assert_store(rm, want, "file_lines", device=False)


def test_files_around_the_tile(rm, toy):
    ids, lin, rank, _ = toy
    T = api.merge_results_tile()
    for name, data in cases.tile_files(T, ids, rank).items():
        want = ref.Merger(ids, lin, rank, 12400 if name == "id_straddles_T" else 2600, 2, 4)
        exp = want.add(data, cases.COL)
        assert exp[5] == ref.OK, name
        for device in (True, False):
            rm.begin(want.capacity, 2, 4)
            if device:
                st, keep = add_on_device(rm, data, cases.COL)
                got = [int(x) for x in st.get()]
                check_workspace(keep)
            else:
                got = rm.add(data, cases.COL)
            assert got[5] == api.MERGE_OK, f"{name}: a regular file was refused: verdict {got[5]}, offence {got[6]}"
            assert got == exp, name
            assert_store(rm, want, name, device)
    assert_votes(rm, want, "tile files")


def test_pieces_equal_the_whole(rm, toy, files):
    ids, lin, rank, _ = toy
    first, data = files["g_b"], files["g_a"]
    starts = [s for s, _ in ref.line_spans(data)][1:]
    assert len(starts) >= 40
    rm.begin(64, 8, 4)
    rm.add(first, cases.COL)
    assert rm.add(data, cases.COL)[5] == api.MERGE_OK
    whole = rm.lists()
    lines = ref.judge(data, cases.COL)[0]
    cuts = [(a,) for a in starts] + [(a, b) for i, a in enumerate(starts) for b in starts[i + 1:]]
    for cut in cuts:
        want = ref.Merger(ids, lin, rank, 64, 8, 4)
        want.add(first, cases.COL)
        rm.begin(64, 8, 4)
        rm.add(first, cases.COL)
        edges = (0,) + cut + (len(data),)
        for k in range(len(edges) - 1):
            piece = data[edges[k]:edges[k + 1]]
            exp = want.add(piece, cases.COL, file_lines=lines, cont=k > 0)
            assert rm.add(piece, cases.COL, file_lines=lines, cont=k > 0) == exp and exp[5] == ref.OK, cut
        lists, places, count = rm.lists()
        assert count == whole[2] and np.array_equal(lists, whole[0]), cut
        assert np.array_equal(places, want.header_places()), cut
    # the device form: the pieces of a cut enqueued back to back on one stream, nothing waited for in between
    for cut in [c for c in cuts if len(c) == 1][::5] + [c for c in cuts if len(c) == 2][::97]:
        want = ref.Merger(ids, lin, rank, 64, 8, 4)
        want.add(first, cases.COL)
        rm.begin(64, 8, 4)
        rm.add(first, cases.COL)
        edges = (0,) + cut + (len(data),)
        pieces = [data[edges[k]:edges[k + 1]] for k in range(len(edges) - 1)]
        staged = [stage(p) for p in pieces]
        for k, sd in enumerate(staged):
            enqueue(rm, sd, cases.COL, file_lines=lines, cont=k > 0)
        for k, (st, keep) in enumerate(staged):
            assert [int(x) for x in st.get()] == want.add(pieces[k], cases.COL, file_lines=lines, cont=k > 0), cut
        lists, places, count = store_on_device(rm)
        assert count == whole[2] and np.array_equal(lists, whole[0]) and np.array_equal(places, want.header_places()), cut


def test_irregular_ranges_change_nothing(rm, toy, files):
    ids, lin, rank, _ = toy
    want = ref.Merger(ids, lin, rank, 64, 4, 4)
    rm.begin(64, 4, 4)
    want.add(files["g_a"], cases.COL)
    rm.add(files["g_a"], cases.COL)
    before = store_on_device(rm)
    for name, (data, at) in cases.irregular_files(ids, rank).items():
        exp = want.add(data, cases.COL)
        assert exp[5] == ref.IRREGULAR and exp[6] == at, name
        st, keep = add_on_device(rm, data, cases.COL)
        assert [int(x) for x in st.get()] == exp, name
        assert rm.add(data, cases.COL) == want.add(data, cases.COL), name
        after = store_on_device(rm)
        assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2])) and before[2] == after[2], name
    # a duplicate across pieces: the second piece names a query of the first
    sp = [int(i) for i, r in zip(ids, rank) if r == 4]
    one = cases.line(3, b"r2", [(sp[0], 9)]) + cases.line(5, b"r4", [])
    two = cases.line(6, b"r5", [(sp[1], 4)]) + cases.line(3, b"r2", [(sp[1], 2)])
    for m in (want, rm):
        assert m.add(one, cases.COL, file_lines=4)[5] == ref.OK
    before = store_on_device(rm)
    exp = want.add(two, cases.COL, cont=True)
    assert exp[5] == ref.IRREGULAR and exp[6] == len(cases.line(6, b"r5", [(sp[1], 4)]))
    st, keep = add_on_device(rm, two, cases.COL, cont=True)
    assert [int(x) for x in st.get()] == exp
    after = store_on_device(rm)
    assert all(np.array_equal(a, b) for a, b in zip(before[:2], after[:2])) and before[2] == after[2]
    # ... and the refusal left no claim behind: the same piece without the duplicate is folded
    ok = cases.line(6, b"r5", [(sp[1], 4)])
    assert rm.add(ok, cases.COL, cont=True) == want.add(ok, cases.COL, cont=True)
    assert_store(rm, want, "after the refusals")


def test_overflow_one_query_short(rm, toy, files):
    ids, lin, rank, _ = toy
    data = files["g_a"]                                              # ids up to 60
    want = ref.Merger(ids, lin, rank, 59, 4, 4)
    rm.begin(59, 4, 4)
    exp = want.add(data, cases.COL)
    assert exp[5] == ref.OVERFLOW and exp[7] == 60
    st, keep = add_on_device(rm, data, cases.COL)
    assert [int(x) for x in st.get()] == exp
    lists, places, count = store_on_device(rm)
    assert count == 0 and not lists.any() and not places.any()
    rm.reserve(exp[7]); want.reserve(exp[7])
    assert rm.add(data, cases.COL) == want.add(data, cases.COL)
    assert_store(rm, want, "after reserve")
    # reserve keeps the content
    rm.reserve(90); want.reserve(90)
    assert rm.add(files["g_c"], cases.COL) == want.add(files["g_c"], cases.COL)
    assert_store(rm, want, "after a second reserve")


def test_two_mergers_on_two_streams(toy, files):
    """two contexts, two streams, work queued on both at once: everything is staged and waited for FIRST, then the adds of both mergers are
    enqueued interleaved, then the copies of the stores and the votes on the same streams; one synchronisation at the end"""
    import torch
    ids, lin, rank, _ = toy
    cap, K = 2600, 4
    big = cases.tile_files(api.merge_results_tile(), ids, rank)["many_tiles"]          # (more than 256 tiles: the streams have work to overlap)
    jobs = []
    for datas in ([big, files["g_a"], files["g_b"], files["g_c"]], [files["part0.txt"], big, files["part1.txt"]]):
        m = api.ResultMerger()
        m.set_taxa(lin, rank, ids)
        m.begin(cap, K, 4)
        want = ref.Merger(ids, lin, rank, cap, K, 4)
        exp = [want.add(d, cases.COL) for d in datas]                                   # (every file here has its top hits in column 2)
        assert all(e[5] == ref.OK for e in exp)
        opts = [api.classify_options(hitmin=o["hitmin"], hitdiff=o["hitdiff"], lowest=o["lowest"], highest=o["highest"]) for o in OPTIONS]
        jobs.append(dict(m=m, want=want, datas=datas, exp=exp, staged=[stage(d) for d in datas], stream=torch.cuda.Stream(), opts=opts,
                         L=Guarded(cap * K), P=Guarded((3 * cap + 1) // 2), N=Guarded(1), votes=[Guarded(cap) for _ in OPTIONS]))
    torch.cuda.synchronize()
    # from here to the end nothing synchronises
    for k in range(max(len(j["datas"]) for j in jobs)):
        for j in jobs:
            if k < len(j["datas"]):
                enqueue(j["m"], j["staged"][k], cases.COL, stream=j["stream"].cuda_stream)
    for j in jobs:
        j["m"].lists_device(0, cap, lists_ptr=j["L"].ptr, places_ptr=j["P"].ptr, num_ptr=j["N"].ptr, stream=j["stream"].cuda_stream)
    for i in range(len(OPTIONS)):
        for j in jobs:
            j["m"].classify_device(j["opts"][i], 0, cap, j["votes"][i].ptr, stream=j["stream"].cuda_stream)
    torch.cuda.synchronize()
    for j in jobs:
        want = j["want"]
        for (st, keep), exp in zip(j["staged"], j["exp"]):
            assert [int(x) for x in st.get()] == exp
            check_workspace(keep)
        assert int(j["N"].get()[0]) == want.count
        assert np.array_equal(j["L"].get(np.uint32).reshape(cap, K, 2), want.lists_array())
        assert np.array_equal(j["P"].get(np.uint32)[:3 * cap].reshape(cap, 3), want.header_places())
        for o, g in zip(OPTIONS, j["votes"]):
            exp = want.classify(o["hitmin"], o["hitdiff"], o["highest"])
            got = g.get(np.uint32).reshape(cap, 2)
            assert np.array_equal(got[:, 0], exp[:, 0]) and np.array_equal(got[:, 1] & 0xFF, exp[:, 1]) and np.array_equal(got[:, 1] >> 8, exp[:, 2]), o
        j["m"].close()


def test_tally_adds_to_the_classify_counters(toy, files):
    ids, lin, rank, _ = toy
    m = api.ResultMerger()                                           # (a context without lineages: the tallies are sized by the taxon table)
    m.set_taxa(lin, rank, ids)
    m.begin(64, 8, 4)
    want = ref.Merger(ids, lin, rank, 64, 8, 4)
    for k in ("g_a", "g_b", "g_c"):
        assert m.add(files[k], cases.COL) == want.add(files[k], cases.COL)
    assigned = np.zeros(ref.NUM_RANKS + 1, dtype=np.uint64)
    per_taxon = np.zeros(len(ids) + 1, dtype=np.uint64)
    for o, n in ((OPTIONS[0], want.count), (OPTIONS[1], 64)):
        exp = want.classify(o["hitmin"], o["hitdiff"], o["highest"])[:n]
        opt = api.classify_options(hitmin=o["hitmin"], hitdiff=o["hitdiff"], lowest=o["lowest"], highest=o["highest"])
        got = m.classify(opt, tally=True, count=n)
        assert np.array_equal(got[:, 0], exp[:, 0]) and np.array_equal(got[:, 1] & 0xFF, exp[:, 1])
        np.add.at(assigned, exp[:, 1], 1)
        np.add.at(per_taxon, exp[exp[:, 0] != 0, 0], 1)
    got_assigned, got_taxa = m.tally(reset=True)
    assert np.array_equal(got_assigned, assigned) and np.array_equal(got_taxa, per_taxon) and per_taxon.sum() > 10
    assert not m.tally()[0].any()
    m.close()


def test_stats_count_the_calls(toy, files):
    ids, lin, rank, _ = toy
    m = api.ResultMerger()
    m.set_taxa(lin, rank, ids)
    m.begin(64, 4, 4)
    a = m.add(files["g_a"], cases.COL)
    bad = cases.irregular_files(ids, rank)["crlf"][0]
    m.add(bad, cases.COL)
    assert m.stats() == [2, len(files["g_a"]) + len(bad), a[0], a[3], a[4], 1]
    m.close()
