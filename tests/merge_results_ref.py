"""A plain Python model of the merge of per-part result files (include/metacache_amd.h: mc_merge_results_*) -- the witness, written from
the rules in the header, not from the library's code.

    judge(data, col)            the line rule on one range: (result lines, comment lines, offence or None, [(start, q, hoff, hlen, entries)])
    Merger(ids, lin, rank, ...) the store: add(data, col, file_lines=0, cont=False) -> status[8] as the library fills it; lists(), header
                                places, count; classify(hitmin, hitdiff, highest) -> [(taxon entry, rank, voters)]
    insert(top, c, ...)         the insert rule on one list
"""
import numpy as np

NUM_RANKS = 21
OK, IRREGULAR, OVERFLOW = 0, 1, 2
DIGITS = b"0123456789"


def parse_line(data: bytes, s: int, e: int, col: int):
    """the line data[s:e] (without its '\\n') -> (q, header offset, header length, [(taxid, hits)]) or None where it breaks the rule"""
    line = data[s:e]
    if any(c in line for c in b"\r\v\f\0"):
        return None
    p = 0
    while p < len(line) and line[p] in DIGITS:
        p += 1
    if p == 0 or int(line[:p]) > 2 ** 32 - 1:
        return None
    ident = int(line[:p])
    q = ident - 1 if ident > 0 else 0
    bar = line.find(b"|", p)
    if bar < 0:
        return None
    p = bar + 1
    while p < len(line) and line[p] in b" \t":
        p += 1
    h0 = p
    while p < len(line) and line[p] not in b" \t":
        if line[p] == ord("|"):
            return None
        p += 1
    if p == h0:
        return None
    hoff, hlen = s + h0, p - h0
    for _ in range(col - 1):
        bar = line.find(b"|", p)
        if bar < 0:
            return None
        p = bar + 1
    tab = line.find(b"\t", p)
    if tab < 0:
        return None
    p = tab + 1
    entries = []
    if p < len(line) and line[p] != ord("\t"):
        end = line.find(b"\t", p)
        text = line[p:] if end < 0 else line[p:end]
        for item in text.split(b","):
            tax, sep, hits = item.partition(b":")
            neg = tax.startswith(b"-")
            digits = tax[1:] if neg else tax
            if not sep or not (1 <= len(digits) <= 18) or not (1 <= len(hits) <= 10):
                return None
            if any(c not in DIGITS for c in digits) or any(c not in DIGITS for c in hits):
                return None
            h = int(hits)
            if h < 1 or h > 2 ** 32 - 1:
                return None
            entries.append((-int(digits) if neg else int(digits), h))
    return q, hoff, hlen, entries


def line_spans(data: bytes):
    """(start, end) of every line: end at its '\\n' or at the end of the range"""
    out, s, n = [], 0, len(data)
    while s < n:
        e = data.find(b"\n", s)
        if e < 0:
            e = n
        out.append((s, e))
        s = e + 1
    return out


def judge(data: bytes, col: int):
    lines = comments = 0
    offence = None
    parsed = []
    for s, e in line_spans(data):
        if data[s:s + 1] == b"#":
            comments += 1
            continue
        lines += 1
        r = parse_line(data, s, e, col)
        if r is None:
            offence = s if offence is None else min(offence, s)
        else:
            parsed.append((s,) + r)
    return lines, comments, offence, parsed


def insert(top, c, merge_below, max_cand):
    """insert_taxon_candidate: top is a list of [taxon entry, hits], hits descending"""
    if len(top) == max_cand and top[-1][1] >= c[1]:
        return

    def place():
        j = 0
        while j < len(top) and top[j][1] >= c[1]:
            j += 1
        if j != len(top) or len(top) < max_cand:
            top.insert(j, list(c))
            del top[max_cand:]

    if merge_below == 0:
        return place()
    for i, t in enumerate(top):
        if t[0] == c[0]:
            if c[1] > t[1]:
                top[i] = list(c)
                j = i
                while j > 0 and top[j][1] > top[j - 1][1]:
                    top[j], top[j - 1] = top[j - 1], top[j]
                    j -= 1
            return
    place()


class Merger:
    def __init__(self, ids, lin, rank, capacity, max_cand, merge_below):
        self.row_of = {int(t): i + 1 for i, t in enumerate(ids)}
        self.lin, self.rank = np.asarray(lin), np.asarray(rank)
        self.capacity, self.max_cand, self.merge_below = capacity, max_cand, merge_below
        self.lists = [[] for _ in range(capacity)]
        self.hdr = [(0, 0, 0)] * capacity
        self.count = 0
        self.calls = 0
        self.file_seen = set()

    def reserve(self, capacity):
        if capacity > self.capacity:
            self.lists += [[] for _ in range(capacity - self.capacity)]
            self.hdr += [(0, 0, 0)] * (capacity - self.capacity)
            self.capacity = capacity

    def add(self, data: bytes, col: int, file_lines: int = 0, cont: bool = False):
        call = self.calls
        self.calls += 1
        if not cont:
            self.file_seen = set()
        lines, comments, offence, parsed = judge(data, col)
        seen = set()
        for s, q, *_ in parsed:                              # a second line for q is an offending line (found below the capacity)
            if q < self.capacity and (q in seen or (cont and q in self.file_seen)):
                offence = s if offence is None else min(offence, s)
            seen.add(q)
        if offence is not None:
            return [lines, comments, self.count, 0, 0, IRREGULAR, offence, 0]
        base = self.count if cont else (file_lines if file_lines else lines)
        need = max([base] + [q + 1 for _, q, *_ in parsed])
        if need > self.capacity:
            return [lines, comments, self.count, 0, 0, OVERFLOW, 0, need]
        if not cont:
            for q in range(base, self.count):
                self.lists[q] = []
                self.hdr[q] = (0, 0, 0)
        self.count = need
        folded = unknown = 0
        for s, q, hoff, hlen, entries in parsed:
            self.file_seen.add(q)
            if self.hdr[q][2] == 0:
                self.hdr[q] = (call, hoff, hlen)
            for taxid, hits in entries:
                x = self.row_of.get(taxid, 0)
                if not x:
                    unknown += 1
                    continue
                folded += 1
                insert(self.lists[q], (x, hits), self.merge_below, self.max_cand)
        return [lines, comments, self.count, folded, unknown, OK, 0, need]

    def lists_array(self):
        out = np.zeros((self.capacity, self.max_cand, 2), dtype=np.uint32)
        for q, l in enumerate(self.lists):
            for j, (x, h) in enumerate(l):
                out[q, j] = (x, h)
        return out

    def header_places(self):
        return np.array(self.hdr, dtype=np.uint32).reshape(self.capacity, 3)

    def classify(self, hitmin: int, hitdiff: float, highest: int):
        """-> [capacity, 3]: taxon entry, rank (21 = unclassified), voters"""
        out = np.zeros((self.capacity, 3), dtype=np.uint32)
        out[:, 1] = NUM_RANKS
        f32 = np.float32
        for q, l in enumerate(self.lists):
            if not l or l[0][1] < hitmin:
                continue
            top = l[0][0]
            r, t, v = int(self.rank[top - 1]), top, 1
            threshold = f32(l[0][1] - hitmin) * f32(hitdiff) if l[0][1] > hitmin else f32(0)
            for x, h in l[1:]:
                if not f32(h) > threshold:
                    break
                v += 1
                found = 0
                while r < NUM_RANKS:
                    a = int(self.lin[top - 1, r])
                    if a and a == int(self.lin[x - 1, r]):
                        found = a
                        break
                    r += 1
                t = found
                if not t or r > highest:
                    t = 0
                    break
            if t and r <= highest:
                out[q] = (t, r, min(v, 255))
        return out
