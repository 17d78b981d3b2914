"""A plain model of the ranking pass over accession2taxid tables (try_to_rank_unranked_targets), in two forms:

  * rank_stream: the reference's own loop (building.cpp:85-149) over its token stream `is >> acc >> accver >> taxid >> gi`, the dropped
    first line and the `break` included, for ANY bytes; test_taxmap_witness_cpu.py pins it to the compiled reference;
  * Model: mc_taxmap_begin / _add / _result as include/metacache_amd.h states them -- the line rule's verdict and offence, the target of
    a row, the winner as the smallest {call, line start} -- which the device is compared with bit for bit.
Both find names as std::map<std::string, ...> does: Python orders bytes as std::string::compare does."""
from bisect import bisect_left, bisect_right

WS = b" \t\n\r\v\f"                       # std::isspace in the "C" locale
MAX_LINE = 1024
OK, IRREGULAR = 0, 1
NOT_FOUND = 0xFFFFFFFFFFFFFFFF


def target_of(names, acc, accver, gi):
    """the index of the name a row names in the ascending list `names`, or None (taxon_with_name / taxon_with_similar_name)"""
    def with_name(n):
        if not n:
            return None
        i = bisect_left(names, n)
        return i if i < len(names) and names[i] == n else None

    def with_similar(n):
        if not n:
            return None
        i = bisect_right(names, n)           # upper_bound: a name equal to n is skipped
        return i if i < len(names) and names[i][:len(n)] == n else None

    t = with_name(accver)
    if t is None:
        t = with_similar(acc)
        if t is None:
            t = with_name(gi)
    return t


class _Stream:
    """std::istream's formatted extraction, as far as the loop uses it"""

    def __init__(self, data):
        self.d, self.p, self.ok = data, 0, True

    def getline(self):
        nl = self.d.find(b"\n", self.p)
        self.p = len(self.d) if nl < 0 else nl + 1

    def _skip(self):
        while self.p < len(self.d) and self.d[self.p] in WS:
            self.p += 1

    def word(self):
        if not self.ok:
            return b""
        self._skip()
        b = self.p
        while self.p < len(self.d) and self.d[self.p] not in WS:
            self.p += 1
        if self.p == b:
            self.ok = False
        return self.d[b:self.p]

    def uint64(self):
        """num_get for an unsigned type: an optional sign, decimal digits up to the first other byte; a '-' negates modulo 2^64"""
        if not self.ok:
            return 0
        self._skip()
        neg = False
        if self.p < len(self.d) and self.d[self.p] in b"+-":
            neg = self.d[self.p] == ord("-")
            self.p += 1
        b = self.p
        while self.p < len(self.d) and 48 <= self.d[self.p] <= 57:
            self.p += 1
        if self.p == b:
            self.ok = False
            return 0
        v = int(self.d[b:self.p])
        if v >= 1 << 64:
            self.ok = False
            return 0
        return (-v) % (1 << 64) if neg else v


def as_parent(taxid):
    """the uint64 the stream read, as the signed 64-bit parent it is stored as"""
    return taxid - (1 << 64) if taxid >= 1 << 63 else taxid


def rank_stream(names, wanted, files):
    """names ascending, wanted[i] flags, files = the whole bytes of each table in order (None: a file that cannot be opened)
    -> {name index: parent} of the names the loop ranked"""
    unranked = {i for i, w in enumerate(wanted) if w}
    parents = {}
    if not unranked:
        return parents
    for data in files:
        if data is None:
            continue
        s = _Stream(data)
        s.getline()
        while True:
            acc = s.word(); accver = s.word(); taxid = s.uint64(); gi = s.word()
            if not s.ok:
                break
            t = target_of(names, acc, accver, gi)
            if t is not None and t in unranked:
                parents[t] = as_parent(taxid)
                unranked.discard(t)
                if not unranked:
                    break
        if not unranked:
            break
    return parents


def line_starts(data):
    out, p = [], 0
    while p < len(data):
        out.append(p)
        nl = data.find(b"\n", p)
        p = len(data) if nl < 0 else nl + 1
    return out


def cut_line(data, s, max_line=MAX_LINE):
    """the line rule on the line that starts at s -> its four tokens, or None where the line is irregular"""
    nl = data.find(b"\n", s)
    line = data[s:len(data) if nl < 0 else nl]
    if len(line) > max_line or any(c in line for c in b"\r\v\f\0"):
        return None
    tok = line.replace(b"\t", b" ").split(b" ")
    tok = [t for t in tok if t]
    if len(tok) != 4 or not (1 <= len(tok[2]) <= 18) or not all(48 <= c <= 57 for c in tok[2]):
        return None
    return tok


def judge(data, max_line=MAX_LINE):
    """-> (verdict, offence, lines) of a range"""
    starts = line_starts(data)
    for s in starts:
        if cut_line(data, s, max_line) is None:
            return IRREGULAR, s, len(starts)
    return OK, 0, len(starts)


class Model:
    """mc_taxmap_begin / mc_taxmap_add / mc_taxmap_result"""

    def __init__(self, names, wanted=None, max_line=MAX_LINE):
        self.names = [bytes(n) for n in names]
        assert all(a < b for a, b in zip(self.names, self.names[1:])), "the names must ascend strictly"
        self.wanted = [True] * len(self.names) if wanted is None else [bool(w) for w in wanted]
        self.key = [NOT_FOUND] * len(self.names)
        self.taxid = [0] * len(self.names)
        self.call = 0
        self.max_line = max_line

    def still_wanted(self):
        return sum(1 for w, k in zip(self.wanted, self.key) if w and k == NOT_FOUND)

    def add(self, data):
        """-> status[8]"""
        call, self.call = self.call, self.call + 1
        verdict, offence, lines = judge(data, self.max_line)
        if verdict != OK:
            return [lines, 0, 0, 0, self.still_wanted(), verdict, offence, 0]
        targeted = hit = newly = 0
        for s in line_starts(data):
            acc, accver, taxid, gi = cut_line(data, s, self.max_line)
            t = target_of(self.names, acc, accver, gi)
            if t is None:
                continue
            targeted += 1
            if not self.wanted[t]:
                continue
            hit += 1
            if self.key[t] == NOT_FOUND:         # (rows come in ascending {call, line start}: the first one is the minimum)
                self.key[t] = (call << 32) | s
                self.taxid[t] = int(taxid)
                newly += 1
        return [lines, targeted, hit, newly, self.still_wanted(), OK, 0, 0]

    def result(self):
        return list(self.taxid), list(self.key), self.still_wanted()
