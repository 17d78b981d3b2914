"""GPU: mc_align_semiglobal through api.align_semiglobal -- (a) every alignment the reference program printed
(tests/golden/align_expected.json.gz: the recorded score and both strings, for the record the reference read), (b) the plain model
(tests/align_ref.py, pinned to the reference by tests/test_align_witness_cpu.py) on problems the goldens cannot reach, (c) the call's
edges: no problems, a context without a table, a database's context."""
import gzip
import json
import os

import numpy as np
import pytest

import align_ref

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")


def _cases():
    with gzip.open(os.path.join(GOLD, "align_expected.json.gz"), "rt") as f:
        return json.load(f)["cases"]


def _golden_problems():
    """[(tag, read, mate, subject, score, aligned query, aligned target)] of every alignment in the goldens"""
    out = []
    records = align_ref.Records(GOLD)
    for case, c in sorted(_cases().items()):
        comment, sep = align_ref.option(c["args"], "-comment", "# "), align_ref.option(c["args"], "-separator", "\t|\t")
        winlen, stride = align_ref.SKETCHING[c["db"]]
        reads = align_ref.queries(os.path.join(GOLD, c["reads"]), "-pairseq" in c["args"])
        name_col = align_ref.columns(c["lines"], comment, sep).index("query_header")
        for i, line, aln in align_ref.parse_output(c["lines"], comment):
            if aln is None:
                continue
            read, mate = reads[line.split(sep)[name_col]]
            if "-cov-percentile" in c["args"]:
                read, mate = b"", None
            score, filename, index, beg, end = align_ref.parse_head(aln[0], comment, stride)
            rec = records.get(filename, align_ref.record_number(index, "reference"))
            out.append(((case, i), read, mate, align_ref.cut(rec, beg, end, winlen, stride), score,
                        aln[1][len(comment) + 9:].encode("latin-1"), aln[2][len(comment) + 9:].encode("latin-1")))
    return out


@pytest.mark.gpu
def test_every_alignment_of_the_goldens():
    from metacache_amd import api
    P = _golden_problems()
    assert len(P) > 400 and any(len(p[1]) > 3000 for p in P) and any(p[2] for p in P)
    got, raw = api.align_semiglobal([p[1] for p in P], [p[3] for p in P], [p[2] for p in P])
    for p, g in zip(P, got):
        assert (g[0], g[2], g[3]) == (p[4], p[5], p[6]), (p[0], g[0], p[4], g[2][:60], p[5][:60])


def _random_problems(rng):
    P = []
    A4, A2 = b"ACGT", b"AC"

    def rnd(n, alphabet=A4):
        return bytes(rng.choice(np.frombuffer(alphabet, dtype=np.uint8), size=n)) if n else b""

    def related(s, n, rate=0.08):
        """n characters read off s somewhere, with substitutions, insertions and deletions"""
        if not s or not n:
            return rnd(n)
        p = int(rng.integers(0, max(1, len(s) - n + 1)))
        out = bytearray()
        for ch in s[p:p + n]:
            u = rng.random()
            if u < rate / 3:
                continue
            if u < 2 * rate / 3:
                out.append(int(rng.choice(np.frombuffer(A4, dtype=np.uint8))))
            out.append(ch if u > rate else int(rng.choice(np.frombuffer(A4, dtype=np.uint8))))
        return bytes(out[:n]) + rnd(max(0, n - len(out)))

    # lengths on both sides of the tiers (256 x 512), the strips (multiples of 64 columns), the row chunks (64) and the panels (512)
    for lq in (0, 1, 2, 63, 64, 65, 128, 129, 255, 256, 257):
        for ls in (0, 1, 2, 63, 64, 65, 127, 128, 129, 255, 256, 257, 320, 321, 511, 512, 513, 1023, 1024, 1025):
            s = rnd(ls)
            q = related(s, lq) if (lq + ls) % 3 else rnd(lq)
            if (lq + ls) % 2:
                q = align_ref.reverse_complement(q)
            P.append((q, None if (lq + ls) % 5 else related(s, 70), s))
    s = rnd(300)
    P += [(s, None, s), (s[50:200], s[120:260], s), (align_ref.reverse_complement(s[50:200]), s[10:100], s)]                       # identical strings
    P += [(b"A" * 90, None, b"C" * 200), (b"A" * 90, b"G" * 50, b"C" * 200), (b"A" * 3, b"T", b"C" * 300), (b"G", b"G", b"C")]    # nothing in common: negative sums wrap
    P += [(b"A" * 100, b"T" * 80, b"A" * 40 + b"C" * 200)]                       # forward wins on read 1, the mate's negative score wraps the sum
    P += [(b"N" * 80, None, b"N" * 150), (b"N" * 80, b"N" * 30, b"ACGT" * 40)]    # N == N matches
    P += [(s[20:150].lower(), None, s), (s[20:150], None, s.lower()), (s[20:80] + s[80:150].lower(), s[100:180].lower(), s)]     # case is kept, never folded
    P += [(b"ACGUUGCA" * 10, None, b"ACGTTGCA" * 20), (b"UGCAACGU" * 10, b"uuuu", b"ACGTTGCA" * 20), (b"acgu" * 20, None, b"acgt" * 30)]   # U: complement A, equal only to U
    for _ in range(150):                                                         # two letters: ties between diag / above / left and between end cells
        ls = int(rng.integers(1, 90)); lq = int(rng.integers(1, 60))
        P.append((rnd(lq, A2), rnd(int(rng.integers(0, 40)), A2) if rng.random() < 0.5 else None, rnd(ls, A2)))
    for _ in range(40):                                                          # periodic sequences: equal scores along the last row and column
        u = rnd(int(rng.integers(1, 5)))
        P.append((u * int(rng.integers(1, 40)), None, u * int(rng.integers(1, 80))))
    for _ in range(6):                                                           # the long tier: several panels, several row chunks
        ls = int(rng.integers(1500, 4000)); s = rnd(ls)
        P.append((related(s, int(rng.integers(300, 1500))), related(s, 200) if rng.random() < 0.5 else None, s))
    return P


def _check_against_model(got, raw, P):
    for i, ((q, m, s), g) in enumerate(zip(P, got)):
        score, rev, aq, at, four = align_ref.align_pair(q, m, s)
        assert list(map(int, raw[i])) == four, (i, len(q), len(m or b""), len(s), list(raw[i]), four)
        assert g == (score, rev, aq, at), (i, len(q), len(s), g[:2], (score, rev), g[2][:50], aq[:50])


@pytest.mark.gpu
def test_against_the_model_where_the_goldens_do_not_reach():
    from metacache_amd import api
    P = _random_problems(np.random.default_rng(7))
    got, raw = api.align_semiglobal([p[0] for p in P], [p[2] for p in P], [p[1] for p in P])
    _check_against_model(got, raw, P)
    # without any mate (NULL mates) the same reads give the same first two scores
    got2, raw2 = api.align_semiglobal([p[0] for p in P[:60]], [p[2] for p in P[:60]])
    for i in range(60):
        assert list(raw2[i][:2]) == list(raw[i][:2]) and list(raw2[i][2:]) == [0, 0]


@pytest.mark.gpu
def test_thousands_of_problems_in_sub_batches():
    """a small budget: the call goes to the device in many sub-batches, short and long tier mixed in each"""
    from metacache_amd import api
    rng = np.random.default_rng(11)
    base = _random_problems(rng)
    P = [base[int(i)] for i in rng.integers(0, len(base), size=3000)]
    A = api.Aligner()
    try:
        A.set_tuning("align_scratch_mb", 1)
        got, raw = A.align([p[0] for p in P], [p[2] for p in P], [p[1] for p in P])
        st = A.stats()
    finally:
        A.close()
    assert st[0] == len(P) and st[3] > 3, st
    memo = {}
    for i, (p, g) in enumerate(zip(P, got)):
        k = id(p)
        if k not in memo:
            memo[k] = align_ref.align_pair(p[0], p[1], p[2])
        score, rev, aq, at, four = memo[k]
        assert g == (score, rev, aq, at) and list(map(int, raw[i])) == four, (i, g[:2], score, rev)


@pytest.mark.gpu
def test_no_problems_and_contexts_with_and_without_a_table(golden):
    from metacache_amd import api
    got, raw = api.align_semiglobal([], [])
    assert got == [] and raw.shape == (0, 4)
    db = api.Database.open(golden.db_path("toy32"))
    try:
        got, raw = api.align_semiglobal([b"ACGTACGTAC"], [b"TTACGTACGTACTT"], handle=db.h.value)
        assert got[0] == (20, False, b"ACGTACGTAC", b"ACGTACGTAC")
        exp = align_ref.align_pair(b"ACGTACGTAC", None, b"TTACGTACGTACTT")
        assert got[0] == exp[:4] and list(map(int, raw[0])) == exp[4]
    finally:
        db.close()
    with pytest.raises(ValueError):
        api.align_semiglobal([b"A"], [])
