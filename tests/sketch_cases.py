"""Inputs of the sketcher tests (TEST INFRASTRUCTURE): the parameter grid, the generated reads and builder targets, and the model's
answers for them (sketch_ref), computed once per process.  test_sketch_ref_cpu.py pins the model and asserts the coverage conditions
on it; test_gpu_sketchers.py and test_gpu_builder_sketchers.py run the same inputs through the device."""
from __future__ import annotations

import functools

import numpy as np

import sketch_ref

# (k, s, w, stride): what each set is there for
QUERY_PARAMS = [
    (16, 16, 127, 112),    # batched lanes, uint4 emit; chunks for long reads
    (16, 8, 127, 112),     # batched lanes, s != 16 emit
    (16, 16, 63, 48),      # batched lanes, stride 48: many window ends per read
    (12, 16, 123, 112),    # generic lanes, even k; chunks
    (15, 16, 126, 112),    # generic lanes, odd k; chunks
    (16, 16, 125, 110),    # generic lanes (stride % 16 != 0); stride % 4 != 0 sends long reads to the wave kernel
    (1, 4, 20, 20),        # k = 1: every window has duplicates, every read is handed over
    (16, 1, 16, 1),        # w == k, one k-mer per window, s = 1
    (16, 1, 1024, 1009),   # threshold raised and restarted (wave); reads up to 512 go through the generic lanes, one window each
    (16, 32, 1024, 1009),  # w == kMaxWinLen: one window per staged segment, 8 rounds with carried sketch, serial-minimum branch
    (16, 32, 255, 240),    # s > 16: wave only; two windows per probe group
    (7, 32, 100, 94),      # the same at a small odd k: duplicates
    (16, 12, 127, 40),     # overlapping windows; s does not divide 64
    (16, 16, 100, 130),    # stride > w
]
BUILD_PARAMS = [
    (16, 16, 127, 112),    # batched build lanes
    (12, 16, 123, 112),    # generic build lanes
    (16, 16, 125, 110),    # stride % 4 != 0: sketch_only_kernel<false>
    (16, 32, 255, 240),    # s > 16: wave
    (8, 8, 35, 28),
]
LANE_MAX_LEN = 512         # kLaneMaxLen: longest mate one lane takes; longer single reads are cut into chunks
BUILD_RECORD_WINDOWS = 256 # kBuildRecWins: windows per builder record
ACGT = np.frombuffer(b"ACGT", dtype=np.uint8)
COMPLEMENT = bytes.maketrans(b"ACGT", b"TGCA")


def lane_path_supported(k, s, w, stride):
    """kernels.hip lane_path_supported: the k-mers of a sequence partition into its windows, the sketch fits a lane's registers"""
    return s <= 16 and stride == w - k + 1 and k <= 16


def chunked(k, s, w, stride, l1, l2):
    """the lane path cuts this read into chunks (lane_chunk_records): a single read beyond a lane's length, chunk starts 4-byte aligned"""
    return lane_path_supported(k, s, w, stride) and stride % 4 == 0 and l2 == 0 and l1 > LANE_MAX_LEN


def random_bases(rng, n):
    return ACGT[rng.integers(0, 4, size=n)].tobytes()


def single_lengths(k, s, w, stride):
    ls = [0, k - 1, k, k + s - 2, k + s - 1, w - 1, w, w + 1, stride + k - 2, stride + k - 1, stride + k, w + stride - 1, w + stride,
          w + stride + 1, 511, 512, 513, 1024, 1025, 3001]
    if (k, s, w, stride) == (16, 1, 16, 1):
        ls = [min(x, 600) for x in ls]            # one window per character: keep the window count small
    return sorted({x for x in ls if x >= 0})


def mate_lengths(k, s, w, stride):
    return sorted({0, k - 1, k, w, w + 1, 512, 513})


def tandem_read(rng, k, w, stride, L, window):
    """random bases with a 20-mer repeated over the inside of ONE window, 8 characters away from both of its ends"""
    r = bytearray(random_bases(rng, L))
    a, b = window * stride + 8, window * stride + w - 8
    unit = random_bases(rng, 20)
    r[a:b] = (unit * (w // 20 + 1))[:b - a]
    return bytes(r)


def emptied_window(k, w, stride):
    """the window content_reads fills with N: the first one behind window 0 that leaves window 0 its first k-mer"""
    return max(1, -(-k // stride))


def content_reads(rng, k, s, w, stride):
    """-> [(name, bytes)]: the content cases, each long enough for full windows before and behind the emptied one and a tail (two full
    windows and a tail wherever stride >= k).  No cap at a lane's length: where the windows are short these reads stay below it, where
    they are long (w > 512) the wave kernel takes them with N on both sides of its 1024-character segment border."""
    j = emptied_window(k, w, stride)
    L = w + j * stride + max(k, stride // 2)
    base = random_bases(rng, L)

    def with_n(positions):
        r = bytearray(base)
        for p in positions:
            assert 0 <= p < L, (p, L)
            r[p] = ord("N")
        return bytes(r)

    out = [("random", base)]
    # one window whose smallest hashes repeat at ONE place only: the last pair a sketch holds, and the first
    for name, rank in (("dup_only_in_last_pair", "last"), ("dup_only_in_first_pair", 0)):
        r = planted_repeat(rng, k, s, w, stride, rank)
        if r is not None:
            out.append((name, r))
    # a window whose first 128 k-mers are random and whose next ones bring more than 64 equal small hashes: the serial minimum
    # has to keep what the first round carried
    if w >= 240:
        out.append(("random_then_poly_a", random_bases(rng, 140) + b"A" * (w - 140)))
    run = max(k, 2)                                # (a run of k, of two at k = 1: it has to stand on both sides of the end)
    out += [("lower", base.lower()),
           ("mixed_case_u", bytes(c + 32 if i % 3 == 0 else (ord("U") if c == ord("T") and i % 2 else c) for i, c in enumerate(base))),
           ("n_at_0", with_n([0])), ("n_at_k-1", with_n([k - 1])), ("n_at_last", with_n([L - 1])),
           ("n_run_across_window_end", with_n(range(w - run // 2, w - run // 2 + run))),
           ("n_run_over_whole_window", with_n(range(j * stride, j * stride + w))),
           ("poly_a", b"A" * L), ("at_repeat", (b"AT" * L)[:L]), ("acg_repeat", (b"ACG" * L)[:L]),
           ("20mer_repeated", (random_bases(rng, 20) * (L // 20 + 1))[:L])]
    # a 16-mer and its reverse complement inside the first window (where a window has room for both)
    if w >= 40:
        r = bytearray(base)
        m = random_bases(rng, 16)
        r[2:18] = m
        r[22:38] = m.translate(COMPLEMENT)[::-1]
        out.append(("16mer_and_revcomp", bytes(r)))
    # long reads (the chunk lanes where the set has them): a tandem repeat inside a single window away from both ends
    Ll = 600 if (k, s, w, stride) == (16, 1, 16, 1) else 3001
    if w >= 60 and stride >= 40:
        nfull = (Ll - w) // stride + 1
        out.append(("long_tandem_in_one_window", tandem_read(rng, k, w, stride, Ll, nfull // 2)))
    out.append(("long_poly_a", b"A" * Ll))
    return out


def planted_repeat(rng, k, s, w, stride, rank):
    """w random bases (one window) in which one k-mer stands a second time, so that -- by the model's facts -- the sl smallest hashes
    hold exactly ONE repeat, at the pair (rank, rank + 1); "last": the last pair a sketch holds.  Found by trial: a copy of a k-mer
    with a small hash is written elsewhere (which removes up to 2k - 1 other k-mers) until the model sees the wanted window.
    None where the set has no room for it."""
    nk = w - k + 1
    sl = min(s, nk)
    if sl < 3 or k < 8 or nk < 3 * k:
        return None
    rank = sl - 2 if rank == "last" else rank
    for _ in range(5000):
        r = bytearray(random_bases(rng, w))
        h, _ = sketch_ref.kmer_hashes(bytes(r), k)
        src = int(np.argsort(h, kind="stable")[rank + int(rng.integers(0, 6))])
        p = int(rng.integers(0, nk))
        if abs(p - src) < k:
            continue
        r[p:p + k] = r[src:src + k]
        m = sketch_ref.facts(bytes(r), k, s, w, stride)
        if len(m.dup) == 1 and m.dup_pairs[0] == 1 and m.dup_first[0] == rank:
            return bytes(r)
    raise AssertionError("no window with a single planted repeat")


@functools.lru_cache(maxsize=None)
def query_reads(params):
    """-> [(name, mate1, mate2)] for one parameter set; mate2 = b"" for single reads.  Seeded by the set."""
    k, s, w, stride = params
    rng = np.random.default_rng([20240611, k, s, w, stride])
    out = []
    for L in single_lengths(*params):
        out.append((f"single_{L}", random_bases(rng, L), b""))
    for name, r in content_reads(rng, *params):
        out.append((name, r, b""))
    for l1 in mate_lengths(*params):
        for l2 in mate_lengths(*params):
            out.append((f"pair_{l1}_{l2}", random_bases(rng, l1), random_bases(rng, l2)))
    for b in range(256):                           # every byte value at the centre of 40 random bases: both encoders on every byte
        r = bytearray(random_bases(rng, 40))
        r[20] = b
        out.append((f"byte_{b}", bytes(r), b""))
    return out


@functools.lru_cache(maxsize=None)
def query_model(params):
    """the model's answer for query_reads(params): per read the Sketch of mate 1 followed by mate 2 (sketch_ref.Sketch of the
    concatenated windows), in read order"""
    out = []
    for _, a, b in query_reads(params):
        fa = sketch_ref.facts(a, *params)
        if b:
            fb = sketch_ref.facts(b, *params)
            fa = sketch_ref.Sketch(*[np.concatenate([x, y]) for x, y in zip(fa, fb)])
        out.append(fa)
    return out


# ---- the two plans of a batch's windows: plan_scan_small_kernel up to kSmallPlan reads, plan_kernel + three-kernel scan beyond ----
SMALL_PLAN = 32768


PLAN_POOL = 41 * 8


@functools.lru_cache(maxsize=None)
def plan_pool():
    """41 * 8 distinct reads of 0 .. 40 random bases: read i has i % 41 bases"""
    rng = np.random.default_rng(77)
    return [random_bases(rng, i % 41) for i in range(PLAN_POOL)]


def plan_switch_reads(n):
    """n reads: read i is plan_pool()[(i * 7 + i // PLAN_POOL) % PLAN_POOL] -- neighbours differ in length, no two tiles of the scan agree"""
    pool = plan_pool()
    return [pool[(i * 7 + i // PLAN_POOL) % PLAN_POOL] for i in range(n)]


# ---- builder targets --------------------------------------------------------------------------------------------------------------
TANDEM_TARGET_WINDOWS = 300
TANDEM_WINDOW = 130         # inside the first record (windows 0 .. 255), far from its ends; the second record holds windows 256 ..


@functools.lru_cache(maxsize=None)
def build_targets(params):
    """-> [(name, bytes)]: targets by their number of full windows, with a rest behind the last full window's stride of k - 1
    characters (no tail window) or k (a tail window of one k-mer), alternating -- for 256 and 512 full windows the tail is the one
    the last lane of a full record takes too"""
    k, s, w, stride = params
    rng = np.random.default_rng([20240612, k, s, w, stride])
    out = []
    for i, nfull in enumerate((1, 3, 4, 5, 255, 256, 257, 512, 513)):
        tail = k if i % 2 else k - 1                             # 256 and 512 full windows get the tail window
        L = (nfull - 1) * stride + w + tail - (k - 1)            # (= nfull * stride + tail where stride = w - k + 1)
        out.append((f"full{nfull}_tail{'k' if tail == k else 'k-1'}", random_bases(rng, L)))
    out.append(("all_n", b"N" * 300))
    out.append(("shorter_than_k", random_bases(rng, k - 1)))
    L = (TANDEM_TARGET_WINDOWS - 1) * stride + w
    t = tandem_read(rng, k, w, stride, L, TANDEM_WINDOW) if w >= 60 else tandem_small(rng, k, w, stride, L, TANDEM_WINDOW)
    out.append(("tandem_in_one_window", only_dup_window(rng, t, params, TANDEM_WINDOW)))
    return out


def only_dup_window(rng, t, params, window):
    """At a small k random sequence repeats k-mers by itself.  The characters [j * stride + k - 1, (j + 1) * stride) belong to the
    k-mers of window j alone (stride = w - k + 1): they are drawn again for every other window the model finds a repeat in."""
    k, s, w, stride = params
    assert stride == w - k + 1
    t = bytearray(t)
    for _ in range(100):
        others = [int(j) for j in np.flatnonzero(sketch_ref.facts(bytes(t), *params).dup) if j != window]
        if not others:
            return bytes(t)
        for j in others:
            t[j * stride + k - 1:(j + 1) * stride] = random_bases(rng, stride - k + 1)
    raise AssertionError("no target whose only window with a repeated hash is the intended one")


def tandem_small(rng, k, w, stride, L, window):
    """the same for short windows: a 5-mer repeated over the inside of one window, 4 characters away from both ends"""
    r = bytearray(random_bases(rng, L))
    a, b = window * stride + 4, window * stride + w - 4
    r[a:b] = (random_bases(rng, 5) * w)[:b - a]
    return bytes(r)


@functools.lru_cache(maxsize=None)
def build_model(params):
    return [sketch_ref.facts(t, *params) for _, t in build_targets(params)]


# ---- coverage: what the inputs must contain, decided by the model's facts alone ---------------------------------------------------
@functools.lru_cache(maxsize=None)
def coverage(params_list=None):
    """-> {condition: [(params, read name, window), ...]} over the query grid (first few witnesses each); params_list: a tuple of sets"""
    found = {c: [] for c in ("below_over_64", "below_under_sl_unsaturated", "carried_rounds_full_sketch", "dup_in_lane_read",
                             "dup_in_one_chunk_of_many", "empty_window_between_others", "serial_minimum_first_round",
                             "serial_minimum_with_carried_sketch", "lane_dup_only_in_last_pair", "lane_dup_only_in_first_pair")}

    def note(c, *w):
        if len(found[c]) < 4:
            found[c].append(w)

    for params in (params_list or QUERY_PARAMS):
        k, s, w, stride = params
        lanes = lane_path_supported(*params)
        for (name, a, b), m in zip(query_reads(params), query_model(params)):
            sl = np.minimum(s, m.nk)
            for i in np.flatnonzero(m.below > 64):
                note("below_over_64", params, name, int(i))
            unsat = np.array([sketch_ref.first_threshold(s, int(x)) < sketch_ref.NONE for x in m.nk], dtype=bool)
            for i in np.flatnonzero((m.below < sl) & unsat & (m.valid >= sl)):
                note("below_under_sl_unsaturated", params, name, int(i))
            # (stricter than `below`: one round of 128 k-mers alone brings more than 64 candidates, whatever was carried into it)
            for i in np.flatnonzero(m.below128 > 64):
                note("serial_minimum_first_round", params, name, int(i))
            if lanes and len(a) <= LANE_MAX_LEN and not b:
                for i in np.flatnonzero((m.dup_pairs == 1) & (m.dup_first == sl - 2)):
                    note("lane_dup_only_in_last_pair", params, name, int(i))
                for i in np.flatnonzero((m.dup_pairs == 1) & (m.dup_first == 0) & (sl > 2)):
                    note("lane_dup_only_in_first_pair", params, name, int(i))
            # (the second round's candidates alone exceed 64 and the first round left others to carry: more than one feature)
            for i in np.flatnonzero((m.below128 > 0) & (m.below256 > 64) & (m.counts > 1)):
                note("serial_minimum_with_carried_sketch", params, name, int(i))
            for i in np.flatnonzero((m.nk > 128) & (m.counts == sl)):
                note("carried_rounds_full_sketch", params, name, int(i))
            if lanes and len(a) <= LANE_MAX_LEN and len(b) <= LANE_MAX_LEN and m.dup.any():
                note("dup_in_lane_read", params, name, int(np.flatnonzero(m.dup)[0]))
            if chunked(*params, len(a), len(b)) and m.dup.any() and not m.dup.all():
                note("dup_in_one_chunk_of_many", params, name, int(np.flatnonzero(m.dup)[0]))
            if len(m.nk) > 1 and (m.valid == 0).any() and (m.valid > 0).any():
                note("empty_window_between_others", params, name, int(np.flatnonzero(m.valid == 0)[0]))
    return found
