"""CPU: the plain sketch model (sketch_ref.py) pinned to the reference's own output and to the C oracle on everything the device
tests feed the sketchers, and the coverage conditions of those inputs, decided by the model alone -- a seed that loses a branch
fails here, without a GPU."""
import numpy as np
import pytest

import cpuref
import sketch_cases as sc
import sketch_ref
from conftest import split


def test_model_matches_reference_sketch_vectors(golden):
    z = golden.npz("sketch_vectors")
    strings = [x.tobytes() for x in split(z["strings"], z["strings_off"])]
    assert len(z["params"]) == 7
    for pi, (k, s, w, st) in enumerate(z["params"]):
        feats, counts, nwin = z[f"p{pi}_feats"], z[f"p{pi}_counts"], z[f"p{pi}_nwin"]
        fo = co = 0
        for x, nw in zip(strings, nwin):
            f, c = sketch_ref.sketch(x, int(k), int(s), int(w), int(st))
            assert len(c) == nw
            assert np.array_equal(c, counts[co:co + nw])
            assert np.array_equal(f.reshape(-1), feats[fo:fo + nw * int(s)])
            fo += nw * int(s); co += nw


@pytest.mark.parametrize("L", [0, 1, 15, 16, 99, 100, 101, 129, 130, 131, 145, 146, 229, 230, 231, 260, 261, 400])
def test_window_rule(L):
    """windows(): against the closed form of windows_of (kernels.h) and, tail suppressed, the full windows alone"""
    for k, w, stride in ((16, 127, 112), (16, 100, 130), (1, 20, 20), (16, 16, 1), (7, 100, 94), (16, 127, 40)):
        ws = sketch_ref.windows(L, k, w, stride)
        if L <= w:
            want = 1 if L >= k else 0
        else:
            nf = (L - w) // stride + 1
            want = nf + (1 if nf * stride < L and L - nf * stride >= k else 0)
        assert len(ws) == want, (L, k, w, stride)
        assert all(n >= k and f + n <= L and (n == w or f + n == L) for f, n in ws)
        assert [f for f, _ in ws] == [i * stride for i in range(len(ws))]
        nt = sketch_ref.windows(L, k, w, stride, no_tail=True)
        assert nt == (ws if L <= w else [x for x in ws if x[1] == w]), (L, k, w, stride)


def test_encoding_table():
    valid = {c: v for letters, v in (("Aa", 0), ("Cc", 1), ("Gg", 2), ("TtUu", 3)) for c in map(ord, letters)}
    for b in range(256):
        assert sketch_ref.CODE[b] == valid.get(b, 4), b


@pytest.mark.parametrize("params", sc.QUERY_PARAMS, ids=str)
def test_model_matches_oracle_on_query_inputs(params):
    orc = cpuref.oracle()
    reads, model = sc.query_reads(params), sc.query_model(params)
    assert 300 <= len(reads) <= 400
    for (name, a, b), m in zip(reads, model):
        f, c = orc.sketch(a, *params)
        if b:
            f2, c2 = orc.sketch(b, *params)
            f, c = np.concatenate([f, f2]), np.concatenate([c, c2])
        assert np.array_equal(c, m.counts), (params, name)
        assert np.array_equal(f, m.feats), (params, name)


@pytest.mark.parametrize("params", sc.BUILD_PARAMS, ids=str)
def test_model_matches_oracle_on_builder_targets(params):
    orc = cpuref.oracle()
    for (name, t), m in zip(sc.build_targets(params), sc.build_model(params)):
        f, c = orc.sketch(t, *params)
        assert np.array_equal(c, m.counts) and np.array_equal(f, m.feats), (params, name)


def test_model_matches_oracle_on_plan_switch_reads():
    orc = cpuref.oracle()
    pool = sc.plan_pool()
    assert sorted({len(r) for r in pool}) == list(range(41))
    for r in pool:
        f, c = orc.sketch(r, 16, 16, 127, 112)
        mf, mc = sketch_ref.sketch(r, 16, 16, 127, 112)
        assert np.array_equal(c, mc) and np.array_equal(f, mf)
    reads = sc.plan_switch_reads(sc.SMALL_PLAN + 1)
    assert len({len(r) for r in reads[-41:]}) > 30 and len(reads[0]) != len(reads[1])


def test_query_inputs_reach_the_branches():
    """Summed over the grid the inputs hold every situation the device tests are there for (the conditions of the device tests,
    asserted here on the model alone)."""
    cov = sc.coverage()
    for cond, witnesses in cov.items():
        assert witnesses, cond


def test_each_parameter_set_does_what_it_is_there_for():
    facts = {p: sc.query_model(p) for p in sc.QUERY_PARAMS}
    reads = {p: sc.query_reads(p) for p in sc.QUERY_PARAMS}

    def windows_where(p, pred):
        return sum(int(pred(m).sum()) for m in facts[p])

    # random reads alone bring the wave sketcher's rare branches at the sets chosen for them
    assert windows_where((16, 32, 1024, 1009), lambda m: m.below > 64) >= 1
    assert windows_where((16, 1, 1024, 1009), lambda m: (m.below < np.minimum(1, m.nk)) & (m.valid >= 1)) >= 1
    assert windows_where((16, 32, 1024, 1009), lambda m: (m.nk == 1009) & (m.counts == 32)) >= 1       # 8 rounds of 128 k-mers
    # k = 1 has two canonical k-mers: every window of three valid k-mers or more repeats one among its smallest
    for m in facts[(1, 4, 20, 20)]:
        assert m.dup[m.valid >= 3].all()
    assert windows_where((1, 4, 20, 20), lambda m: m.dup) > 1000
    assert windows_where((7, 32, 100, 94), lambda m: m.dup) >= 1
    # w == k: one k-mer per window
    assert all((m.nk == 1).all() for m in facts[(16, 1, 16, 1)])
    # stride > w: characters between two windows belong to none
    assert any(len(m.first) > 1 and (np.diff(m.first) == 130).all() for m in facts[(16, 16, 100, 130)])
    # lengths on both sides of every kernel choice, at the sets with chunk lanes; the tandem read's repeat stays inside one chunk
    for p in ((16, 16, 127, 112), (12, 16, 123, 112), (15, 16, 126, 112)):
        ls = {len(a) for _, a, b in reads[p] if not b}
        assert {511, 512, 513, 1024, 1025, 3001} <= ls
        (m,) = [m for (name, _, _), m in zip(reads[p], facts[p]) if name == "long_tandem_in_one_window"]
        assert int(m.dup.sum()) == 1 and len(m.dup) > 20
    # a single repeat at the last pair of the sketch and at the first, at every set whose lanes look for repeats themselves
    for p in sc.QUERY_PARAMS:
        if sc.lane_path_supported(*p) and p[0] >= 8 and p[1] >= 3:
            by = {name: m for (name, _, _), m in zip(reads[p], facts[p])}
            last, first = by["dup_only_in_last_pair"], by["dup_only_in_first_pair"]
            assert last.dup_pairs.tolist() == [1] and last.dup_first.tolist() == [p[1] - 2] and last.counts.tolist() == [p[1]], p
            assert first.dup_pairs.tolist() == [1] and first.dup_first.tolist() == [0], p
    # the serial minimum with a sketch carried in from the first round that the second round's equal hashes do not replace
    for p in ((16, 1, 1024, 1009), (16, 32, 1024, 1009), (16, 32, 255, 240)):
        (m,) = [m for (name, _, _), m in zip(reads[p], facts[p]) if name == "random_then_poly_a"]
        assert m.below256[0] > 64 and m.feats[0, 0] == 0
    for p in ((16, 32, 1024, 1009), (16, 32, 255, 240)):
        (m,) = [m for (name, _, _), m in zip(reads[p], facts[p]) if name == "random_then_poly_a"]
        assert m.below128[0] > 0 and m.counts[0] > 1
    assert not sc.chunked(16, 16, 125, 110, 3001, 0) and sc.chunked(16, 16, 127, 112, 513, 0) and not sc.chunked(16, 16, 127, 112, 512, 0)
    # every byte value stands in a read of its own
    for p in sc.QUERY_PARAMS:
        assert sorted(a[20] for name, a, _ in reads[p] if name.startswith("byte_")) == list(range(256))


@pytest.mark.parametrize("params", sc.QUERY_PARAMS, ids=str)
def test_content_reads_hold_what_their_names_say(params):
    """every named content case, at every set: the N characters stand where the name puts them (none dropped at the read's end), the
    run across a window end spans one, the emptied window lies between windows that keep k-mers"""
    k, s, w, stride = params
    by = {name: (a, m) for (name, a, _), m in zip(sc.query_reads(params), sc.query_model(params))}
    base, _ = by["random"]
    L = len(base)
    j = sc.emptied_window(k, w, stride)
    assert L > j * stride + w and len(by["random"][1].nk) >= 3 and b"N" not in base
    if sc.lane_path_supported(*params) and w <= 256:
        assert L <= sc.LANE_MAX_LEN                                   # (short windows: the lanes take the content cases)

    def n_at(name):
        a, _ = by[name]
        assert len(a) == L
        at = [i for i in range(L) if a[i] == ord("N")]
        assert all(a[i] == base[i] for i in range(L) if i not in at), name
        return at

    assert n_at("n_at_0") == [0] and n_at("n_at_k-1") == [k - 1] and n_at("n_at_last") == [L - 1]
    run = n_at("n_run_across_window_end")
    assert len(run) == max(k, 2) and run == list(range(run[0], run[0] + len(run))) and run[0] < w <= run[-1]     # window 0 ends at w
    m = by["n_run_across_window_end"][1]
    assert m.valid[0] < by["random"][1].valid[0]                    # the window that ends there loses k-mers, and so does the next one
    assert stride > w or (m.valid[1:] < by["random"][1].valid[1:]).any()     # (stride > w: the characters behind the end belong to no window)
    assert n_at("n_run_over_whole_window") == list(range(j * stride, j * stride + w))
    m = by["n_run_over_whole_window"][1]
    assert m.valid[j] == 0 and m.valid[0] > 0 and (m.valid[j + 1:] > 0).any(), params
    if w > 512:                                                       # ambiguous characters on both sides of the 1024-character segment border
        assert run[0] < 1024 <= run[-1] and max(n_at("n_run_over_whole_window")) >= 1024
    # the other cases
    assert by["lower"][0] == base.lower() and by["poly_a"][0] == b"A" * L and by["at_repeat"][0][:4] == b"ATAT" and by["acg_repeat"][0][:6] == b"ACGACG"
    u = by["mixed_case_u"][0]
    assert u.upper().replace(b"U", b"T") == base and any(c in u for c in b"acgt") and (b"U" in u)
    rep = by["20mer_repeated"][0]
    assert rep[20:] == rep[:-20]
    assert ("16mer_and_revcomp" in by) == (w >= 40)
    if w >= 40:
        a = by["16mer_and_revcomp"][0]
        assert a[22:38] == a[2:18].translate(sc.COMPLEMENT)[::-1]
    assert ("long_tandem_in_one_window" in by) == (w >= 60 and stride >= 40)


@pytest.mark.parametrize("params", sc.BUILD_PARAMS, ids=str)
def test_builder_targets_reach_the_record_borders(params):
    k, s, w, stride = params
    targets, model = sc.build_targets(params), sc.build_model(params)
    by = {name: (t, m) for (name, t), m in zip(targets, model)}
    want = {"full1_tailk-1": 1, "full3_tailk": 4, "full4_tailk-1": 4, "full5_tailk": 6, "full255_tailk-1": 255, "full256_tailk": 257,
            "full257_tailk-1": 257, "full512_tailk": 513, "full513_tailk-1": 513, "all_n": len(sketch_ref.windows(300, k, w, stride)),
            "shorter_than_k": 0, "tandem_in_one_window": sc.TANDEM_TARGET_WINDOWS}
    assert {n: len(m.nk) for n, (t, m) in by.items()} == want
    for n, (t, m) in by.items():
        if n.endswith("_tailk"):
            assert m.nk[-1] == 1 and m.nk[-2] == stride                     # a tail window of one k-mer
        if n.endswith("_tailk-1"):
            assert (m.nk == stride).all()
    assert (by["all_n"][1].counts == 0).all() and len(by["all_n"][1].counts) > 0
    # the tandem target: exactly the intended window repeats a hash -- its record (windows 0 .. 255) is flagged, the next one is not
    dups = np.flatnonzero(by["tandem_in_one_window"][1].dup)
    assert dups.tolist() == [sc.TANDEM_WINDOW] and sc.TANDEM_WINDOW < sc.BUILD_RECORD_WINDOWS < sc.TANDEM_TARGET_WINDOWS
    assert max(len(t) for _, t in targets) <= 513 * stride + w
