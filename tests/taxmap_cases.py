"""Inputs of the taxmap tests: the records and the table the witness test gives to the reference, and the name tables and ranges the
device tests run (cases()), built around the tile T and the longest line M of the library.  Data only: what is expected comes from
taxmap_ref."""
import os
import random

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# ---- the witness: a dozen records for the reference's `build`, and the table of its ranking pass ------------------------------------
WITNESS_HEADERS = [
    "AA_000001.1 exact accession.version",
    "AB_000002.1 a similar accession beats a later exact row",
    "AC_000003 a name equal to an accession",
    "AC_000003.1 the next longer name",
    "AD_000004.1 first use of the id",
    "AD_000004.1 second use of the id",
    "gi|77777|gb|whatever found by its gi",
    "AE_000005.1 ranked by a row of three tokens",
    "AF_000006.1 behind the shifted tokens",
    "AG_000007.1 behind the end of the loop",
    "AH_000008.1 ranked by its header taxid=562 ",
    "AI_000009.1 no row at all",
]
WITNESS_TABLE = (b"accession\taccession.version\ttaxid\tgi\n"
                 b"AA_000001\tAA_000001.1\t100\t1\n"
                 b"AB_000002\tAB_000002.9\t200\t2\n"
                 b"AB_000002\tAB_000002.1\t201\t3\n"
                 b"AC_000003\tAC_000003.5\t300\t4\n"
                 b"AD_000004\tAD_000004.1\t400\t5\n"
                 b"AD_000004\tAD_000004.7\t401\t6\n"
                 b"XX_000001\tXX_000001.1\t500\t77777\n"
                 b"AH_000008\tAH_000008.1\t999\t7\n"
                 b"AE_000005\tAE_000005.1\t600\n"
                 b"AF_000006\tAF_000006.1\t700\tna\n"
                 b"AG_000007\tAG_000007.1\t800\t8\n")


def witness_fasta():
    x, out = 12345, []
    for h in WITNESS_HEADERS:
        seq = []
        for _ in range(400):
            x = (x * 1103515245 + 12345) % (1 << 31)
            seq.append("ACGT"[(x >> 16) & 3])
        s = "".join(seq)
        out.append(">" + h + "\n" + "\n".join(s[i:i + 80] for i in range(0, 400, 80)) + "\n")
    return "".join(out)


# ---- the device tests' inputs ------------------------------------------------------------------------------------------------------
def filler(length, k=0):
    """a regular line of exactly `length` bytes, its '\\n' included, that names no target (9 <= length)"""
    assert length >= 9
    return b"~" + b"%d" % (k % 10) + b"x" * (length - 9) + b" ~ 1 ~\n"


def fill_to(buf, offset, piece=500):
    """filler lines behind buf so that the next line starts at `offset`"""
    out = bytearray(buf)
    k = 0
    while len(out) < offset:
        left = offset - len(out)
        n = left if left < piece + 9 else piece
        out += filler(n, k)
        k += 1
    assert len(out) == offset
    return bytes(out)


def row(acc, accver, taxid, gi, sep=b"\t"):
    return sep.join([acc, accver, b"%d" % taxid if isinstance(taxid, int) else taxid, gi]) + b"\n"


def numbered(n):
    return [b"N%06d.1" % i for i in range(n)]


def cases(T=4096, M=1024):
    """-> {case: (names ascending, wanted flags or None, [range, ...])}"""
    out = {}
    three = [b"P_000001.1", b"P_000002.1", b"P_000003.1", b"P_000004.1"]
    hit = lambda i, taxid: row(three[i][:-2], three[i], taxid, b"9")

    # line starts at T - 1, 2 T and 3 T + 1, and a line across the border of tiles 4 and 5
    b = fill_to(b"", T - 1) + hit(0, 11)
    b = fill_to(b, 2 * T) + hit(1, 12)
    b = fill_to(b, 3 * T + 1) + hit(2, 13)
    b = fill_to(b, 5 * T - 10) + hit(3, 14)
    out["tile_borders"] = (three, None, [fill_to(b, 6 * T + 100)])

    # the longest line, by blanks and by a token; one byte more is refused
    head = row(b"P_000001", b"P_000001.1", 5, b"1")
    long_blank = b"P_000002" + b" " * (M - 8 - 15) + b"\tP_000002.1\t6\t1\n"
    long_token = b"P_000003\tP_000003.1\t7\t" + b"g" * (M - 22) + b"\n"
    assert len(long_blank) == M + 1 and len(long_token) == M + 1
    out["max_line"] = (three, None, [head + long_blank + long_token + hit(3, 8)])
    out["max_line_plus_one_blank"] = (three, None, [head + long_blank[:8] + b" " + long_blank[8:] + hit(3, 8)])
    out["max_line_plus_one_token"] = (three, None, [head + long_token[:-1] + b"g\n" + hit(3, 8)])
    out["max_line_plus_one_no_newline"] = (three, None, [head + long_token[:-1] + b"g"])
    out["max_line_no_newline"] = (three, None, [head + long_token[:-1]])
    out["much_too_long"] = (three, None, [head + b"P_000002 " + b"z" * (3 * T) + b" 5 1\n" + hit(3, 8)])

    out["one_line"] = (three, None, [hit(1, 21)])
    out["one_line_no_newline"] = (three, None, [hit(1, 21)[:-1]])
    out["one_byte_lines"] = (three, None, [b"a"])
    out["blanks_at_both_ends"] = (three, None, [b"  \tP_000001 \t P_000001.1\t31  7 \t\n" + b" P_000002.5 P_000002.1 32 7 " + b"\n\t" + hit(2, 33)[:-1] + b"\t"])

    high = sorted([b"\xc3\xa9_000001.1", b"\xff\xfe", b"\xff\xfe\x80", b"\x80", b"A\xe4.2", b"zz"])
    rows = (row(b"\xc3\xa9_000001", b"\xc3\xa9_000001.1", 41, b"\xff") + row(b"\xff", b"\xff\x80", 42, b"1") + row(b"\xff\xfe", b"q", 43, b"1")
            + row(b"q", b"q.1", 44, b"\x80") + row(b"A\xe4", b"A\xe4.1", 45, b"zz") + row(b"q", b"q.1", 46, b"zz"))
    out["high_bytes"] = (high, None, [rows])

    # names that are prefixes of each other and of tokens
    pre = sorted([b"AB", b"AB.1", b"AB.1!1", b"AB.10", b"ABC", b"A", b"AB.1!1!2", b"B"])
    rows = b"".join([row(b"AB", b"AB.2", 51, b"0"), row(b"AB.1", b"zz", 52, b"0"), row(b"A", b"AB.1!1", 53, b"0"), row(b"AB.10", b"AB.100", 54, b"A"),
                     row(b"AB.1!1!", b"q", 55, b"0"), row(b"ABCD", b"ABCD.1", 56, b"ABC"), row(b"B", b"B", 57, b"0"), row(b"AB.", b"q", 58, b"AB"),
                     row(b"ABC", b"ABC.1", 59, b"AB"), row(b"C", b"C", 60, b"C"), row(b"@", b"@", 61, b"B")])
    out["prefix_names"] = (pre, None, [rows])
    out["prefix_names_some_wanted"] = (pre, [i % 2 for i in range(len(pre))], [rows])

    # name counts around a wave, and many
    for n in (0, 1, 2, 63, 64, 65, 5000):
        names = numbered(n)
        rng = random.Random(100 + n)
        rows = []
        for j in range(max(40, min(n, 400))):
            i = rng.randrange(max(n, 1) + 2) - 1                      # -1 and n: no such name
            kind = rng.randrange(3)
            nm = b"N%06d" % i if i >= 0 else b"M999999"
            if kind == 0:
                rows.append(row(nm, nm + b".1", 1000 + j, b"0"))
            elif kind == 1:
                rows.append(row(nm, nm + b".7", 2000 + j, b"0"))
            else:
                rows.append(row(b"q", b"q.1", 3000 + j, nm + b".1"))
        out["names_%d" % n] = (names, [rng.randrange(4) != 0 for _ in names], [b"".join(rows)])

    # the same target named in two tiles and in two calls: the first row wins
    b = fill_to(hit(0, 71), T + 7) + hit(0, 72) + hit(1, 73)
    out["two_tiles_two_calls"] = (three, None, [fill_to(b, 2 * T + 50), hit(1, 74) + hit(0, 75) + hit(2, 76)])
    # a refused call between two accepted ones changes nothing and still takes its call number
    out["refused_between"] = (three, None, [hit(0, 81), hit(1, 82) + b"\n" + hit(2, 83), hit(2, 84) + hit(0, 85)])
    out["all_ranked_then_more"] = (three[:2], None, [hit(0, 91) + hit(1, 92), hit(0, 93) + hit(1, 94)])
    out["nothing_wanted"] = (three, [0, 0, 0, 0], [hit(0, 95) + hit(1, 96)])
    out["taxid_0_and_18_digits"] = (three, None, [hit(0, 0) + hit(1, 999999999999999999) + hit(2, b"000000000000000007")])
    out["taxid_19_digits"] = (three, None, [hit(0, 1) + hit(1, b"1000000000000000000") + hit(2, 3)])

    # every irregular kind between regular lines; the first of two offending lines is the offence
    good = hit(0, 1) + filler(300) + hit(1, 2)
    kinds = {"empty_line": b"\n", "blank_line": b" \t \n", "cr": b"P_000003\tP_000003.1\t3\t1\r\n", "cr_inside": b"P_000003\tP_0\r00003.1\t3\t1\n",
             "vt": b"P_000003\tP_000003.1\t3\x0b1\n", "ff": b"\x0cP_000003\tP_000003.1\t3\t1\n", "nul": b"P_000003\tP_000003.1\t3\t1\0\n",
             "three_tokens": b"P_000003\tP_000003.1\t3\n", "five_tokens": b"P_000003\tP_000003.1\t3\t1\t2\n", "one_token": b"P_000003\n",
             "taxid_letters": b"P_000003\tP_000003.1\t3x\t1\n", "taxid_sign": b"P_000003\tP_000003.1\t+3\t1\n", "taxid_minus": b"P_000003\tP_000003.1\t-3\t1\n",
             "taxid_19": b"P_000003\tP_000003.1\t1234567890123456789\t1\n"}
    for k, bad in kinds.items():
        out["irregular_" + k] = (three, None, [good + bad + hit(2, 4)])
    out["irregular_first_line"] = (three, None, [b"\n" + good])
    out["irregular_last_line"] = (three, None, [good + b"P_000003 P_000003.1 3"])
    out["irregular_twice"] = (three, None, [fill_to(good, T + 3) + kinds["cr"] + fill_to(b"", 2 * T) + kinds["three_tokens"] + hit(2, 4)])

    # a range that ends inside a thread's 16 bytes: every length L .. L + 15 inside one tile and around the tile border, the last line whole
    # and without its '\n' (a call and a name each), and a line that starts in the range's last byte (refused there)
    sweep = numbered(32)
    for zone, L in (("one_tile", 208), ("tile_border", T - 8)):
        ends, last_byte = [], []
        for i in range(16):
            for j, cut in ((2 * i, 0), (2 * i + 1, 1)):
                last = row(sweep[j][:-2], sweep[j], 500 + j, b"9")
                r = fill_to(b"", L + i + cut - len(last)) + last
                ends.append(r[:len(r) - cut])
            last_byte.append(fill_to(b"", L + i - 1) + b"x")
        assert [len(r) for r in ends[0::2]] == [len(r) for r in ends[1::2]] == [len(r) for r in last_byte] == list(range(L, L + 16))
        out["tail_sweep_" + zone] = (sweep, None, ends)
        out["irregular_last_byte_" + zone] = (sweep, None, last_byte)

    # random rows
    rng = random.Random(20261021)
    names = sorted({b"R%05d" % rng.randrange(3000) + (b".%d" % rng.randrange(1, 4) if rng.randrange(5) else b"") for _ in range(340)})[:300]
    assert len(names) == 300
    wanted = [rng.randrange(5) != 0 for _ in names]
    rows = []
    for j in range(20000):
        base = b"R%05d" % rng.randrange(3000) if rng.randrange(3) else rng.choice(names).split(b".")[0]
        ver = base + b".%d" % rng.randrange(1, 4)
        gi = rng.choice(names) if rng.randrange(50) == 0 else b"%d" % rng.randrange(10 ** 6)
        rows.append(row(base, ver, rng.randrange(10 ** 7), gi, sep=rng.choice([b"\t", b" ", b"\t "])))
    cut = len(rows) // 2
    out["random_20000x300"] = (names, wanted, [b"".join(rows[:cut]), b"".join(rows[cut:])])
    return out


def read_targets(name):
    """{target name: parent} of the sequence-level taxa in <name>.meta (database.cpp:247-290)"""
    import struct
    b = open(name + ".meta", "rb").read()
    p = 8
    widths = struct.unpack_from("<7B", b, p); p += 7
    p += 8 * 9                                                    # two sketchers, the location limit
    p += (2 if widths[1] == 2 else 4) + 4                         # targets, parts
    ntaxa = struct.unpack_from("<Q", b, p)[0]; p += 8
    out = {}
    for _ in range(ntaxa):
        tid, parent, rank = struct.unpack_from("<qqB", b, p); p += 17
        strs = []
        for _ in range(2):
            n = struct.unpack_from("<Q", b, p)[0]; p += 8
            strs.append(b[p:p + n]); p += n
        p += 16
        if tid < 0 and rank == 0:
            out[strs[0]] = parent
    assert p == len(b)
    return out


def run_witness(ref_binary, workdir):
    """the reference's `build` over the witness records with the witness table as -taxpostmap -> {target name: parent}"""
    import subprocess
    fa, table, db = os.path.join(workdir, "witness.fa"), os.path.join(workdir, "witness.accession2taxid"), os.path.join(workdir, "witness_db")
    with open(fa, "w") as f:
        f.write(witness_fasta())
    with open(table, "wb") as f:
        f.write(WITNESS_TABLE)
    r = subprocess.run([ref_binary, "build", db, fa, "-taxpostmap", table, "-threads", "1"], cwd=workdir, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    return read_targets(db)
