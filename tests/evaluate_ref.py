"""A plain Python / numpy model of the evaluation against a ground truth (include/metacache_amd.h: mc_set_taxon_table,
mc_evaluate_assignments, mc_evaluate_tally) -- written from the rule in the header, not from the library's code.

    taxon_table(taxa)         the table of every taxon from (id, parent, rank) triples: make_ranks, the rank, covers
    evaluate_plain(...)       the verdicts and the per-rank bins of a list of (assigned, truth) pairs, read by read
    evaluate(...)             the same through the distinct pairs of the list (what long lists are modelled with)
    synthetic_taxa(rng)       a random taxonomy for the tests: ranks skipped, taxa without a rank, taxa no target covers
    random_pairs(...)         a mix of (assigned, truth) pairs over a table
"""
import numpy as np

NUM_RANKS = 21
NONE = NUM_RANKS


def parent_chain(taxa, by_id, i):
    """indices of taxon i and of its ancestors, lowest first: until an unknown id, a self-parent (or an id that is no taxon's: <= 0)"""
    chain = [i]
    pid = taxa[i][1]
    while pid > 0 and pid in by_id:
        j = by_id[pid]
        chain.append(j)
        if taxa[j][1] == pid:
            break
        pid = taxa[j][1]
    return chain


def taxon_table(taxa):
    """taxa: [(id, parent, rank, ...)] in table order; targets are the taxa with negative ids.
    -> lin[n, 21] uint32 (index + 1, 0 = none), rank[n] uint8 (21 = none), covered[n] uint8"""
    n = len(taxa)
    by_id = {t[0]: i for i, t in enumerate(taxa)}
    lin = np.zeros((n, NUM_RANKS), dtype=np.uint32)
    rank = np.array([min(int(t[2]), NONE) for t in taxa], dtype=np.uint8).reshape(n)
    covered = np.zeros(n, dtype=np.uint8)
    for i in range(n):
        chain = parent_chain(taxa, by_id, i)
        for j in chain:                                  # a later (higher) taxon of the same rank overwrites
            if rank[j] < NONE:
                lin[i, rank[j]] = j + 1
        if taxa[i][0] < 0:
            covered[chain] = 1
    return lin, rank, covered


def derived_rank(lin):
    """the rank where none is given: the slot that names the taxon itself"""
    rank = np.full(len(lin), NONE, dtype=np.uint8)
    for x in range(len(lin)):
        own = np.nonzero(lin[x] == x + 1)[0]
        if len(own):
            rank[x] = own[0]
    return rank


def evaluate_plain(lin, rank, covered, assigned, truth, coverage=False):
    """-> verdicts [n, 3] (known, correct, counted wrong) and a dict of the bins: assigned, known, correct, wrong [22],
    coverage [22, 4] (true_pos, false_pos, true_neg, false_neg), reads, out_of_table"""
    n_taxa = len(lin)
    bins = {k: np.zeros(NUM_RANKS + 1, dtype=np.uint64) for k in ("assigned", "known", "correct", "wrong")}
    conf = np.zeros((NUM_RANKS + 1, 4), dtype=np.uint64)
    verdicts = np.zeros((len(truth), 3), dtype=np.uint8)
    out_of_table = 0
    for i, (a, t) in enumerate(zip(map(int, assigned), map(int, truth))):
        if a > n_taxa:
            a = 0; out_of_table += 1
        if t > n_taxa:
            t = 0; out_of_table += 1
        ar = int(rank[a - 1]) if a else NONE
        kr = int(rank[t - 1]) if t else NONE
        cr = NONE
        if a and t:
            for r in range(NUM_RANKS):
                if lin[a - 1, r] != 0 and lin[a - 1, r] == lin[t - 1, r]:
                    cr = int(rank[lin[a - 1, r] - 1])
                    break
        cr = max(cr, ar, kr)
        bins["assigned"][ar] += 1
        bins["known"][kr] += 1
        wrong = False
        if kr != NONE:
            bins["correct"][cr] += 1
            if cr > kr and cr > ar:
                bins["wrong"][cr - 1] += 1
                wrong = True
        verdicts[i] = (kr, cr, int(wrong))
        if coverage and t:
            for r in range(NUM_RANKS):
                x = int(lin[t - 1, r])
                if not x:
                    continue
                rr = int(rank[x - 1])
                on = a != 0 and rr >= ar
                cov = bool(covered[x - 1])
                conf[rr, (0 if on else 3) if cov else (1 if on else 2)] += 1
    return verdicts, dict(bins, coverage=conf, reads=len(truth), out_of_table=out_of_table)


def evaluate(lin, rank, covered, assigned, truth, coverage=False):
    """evaluate_plain on every DISTINCT pair once, each weighted by how often the list holds it: the counters are sums over reads and a
    verdict depends on its pair alone"""
    assigned = np.asarray(assigned, dtype=np.uint64)
    truth = np.asarray(truth, dtype=np.uint64)
    pairs, inverse, counts = np.unique((assigned << np.uint64(32)) | truth, return_inverse=True, return_counts=True)
    verdicts = np.zeros((len(pairs), 3), dtype=np.uint8)
    total = None
    for k, (p, c) in enumerate(zip(pairs, counts)):
        v, one = evaluate_plain(lin, rank, covered, [int(p) >> 32], [int(p) & 0xFFFFFFFF], coverage)
        verdicts[k] = v[0]
        if total is None:
            total = {key: np.zeros_like(val) if isinstance(val, np.ndarray) else 0 for key, val in one.items()}
        for key, val in one.items():
            total[key] = total[key] + val * (np.uint64(c) if isinstance(val, np.ndarray) else int(c))
    if total is None:
        return evaluate_plain(lin, rank, covered, [], [], coverage)
    return verdicts[inverse.reshape(-1)], total


def synthetic_taxa(rng, nodes=2400, targets=560):
    """(id, parent, rank) triples: a root, a chain with a taxon of EVERY rank 20 .. 1 and two targets under each of its taxa (siblings
    under every rank), then random inner taxa (a rank below the parent's next ranked one, or none) and random targets"""
    taxa = [(1, 1, 20)]
    eff = {1: 20}                              # id -> the rank of the taxon or of its next ranked ancestor
    nxt, tgt = 2, 0
    for r in range(19, 0, -1):
        taxa.append((nxt, nxt - 1, r)); eff[nxt] = r; nxt += 1
    chain = [t[0] for t in taxa]
    for pid in chain:
        for _ in range(2):
            taxa.append((-(tgt + 1), pid, 0)); tgt += 1
    inner = list(chain)
    while nxt < nodes:
        pid = inner[int(rng.integers(len(inner)))]
        if eff[pid] <= 1:
            continue
        rank = NONE if rng.random() < 0.15 else int(rng.integers(1, eff[pid]))
        taxa.append((nxt, pid, rank)); eff[nxt] = eff[pid] if rank == NUM_RANKS else rank
        inner.append(nxt); nxt += 1
    for _ in range(targets):
        taxa.append((-(tgt + 1), inner[int(rng.integers(len(inner) // 2))], 0)); tgt += 1      # (the later half of the taxa stays uncovered)
    order = rng.permutation(len(taxa))
    return [taxa[i] for i in order]


def random_pairs(rng, n, n_taxa, lin):
    """a mix: any two taxa, the truth's own ancestors, the same taxon, nothing, entries beyond the table"""
    a = rng.integers(1, n_taxa + 1, n).astype(np.uint32)
    t = rng.integers(1, n_taxa + 1, n).astype(np.uint32)
    kind = rng.integers(0, 10, n)
    slot = lin[t - 1, rng.integers(0, NUM_RANKS, n)]
    a = np.where((kind == 0) | (kind == 1), np.where(slot != 0, slot, a), a)      # an ancestor of the truth (or the truth itself)
    a = np.where(kind == 2, t, a)
    a = np.where(kind == 3, 0, a)
    t = np.where(kind == 4, 0, t)
    a = np.where(kind == 5, n_taxa + 1 + (a % 3), a)
    return a.astype(np.uint32), t.astype(np.uint32)


def same_counters(ev, want):
    """an api.Evaluation against the model's bins -> list of the counters that differ"""
    bad = [k for j, k in enumerate(("assigned", "known", "correct", "wrong")) if not np.array_equal(ev.bins[j], want[k])]
    if not np.array_equal(ev.confusion, want["coverage"]):
        bad.append("coverage")
    bad += [k for k in ("reads", "out_of_table") if getattr(ev, k) != want[k]]
    return bad
