"""What the table-content tests share: the reference's recorded `info <db> statistics | featurecounts | featuremap` output
(tests/golden/table_info_expected.json.gz, table_info_maps_expected.json.gz; made by tests/golden/make_golden_table_info.py), cut into
its sections, and the lines of the statistics block as the reference words them."""
import functools
import gzip
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = os.path.join(HERE, "golden")
RULE = "==================================================="
DBS = ["toy32", "toy16", "toy32p2", "toy32p4"]
MAP_DBS = ["toy32", "toy16", "toy32p2"]


@functools.lru_cache(maxsize=None)
def golden():
    out = {}
    for f in ("table_info_expected.json.gz", "table_info_maps_expected.json.gz"):
        with gzip.open(os.path.join(GOLD, f), "rt") as fh:
            out.update(json.load(fh))
    return out


def drop_version(lines):
    return [l for l in lines if not l.startswith("MetaCache version")]


def split_output(lines):
    """stdout lines -> (head: everything up to and including the first rule, parts: [(header or None, [lines])], tail: from the second rule)
    A `statistics` output has no rule: all of it is head."""
    if RULE not in lines:
        return lines, [], []
    a = lines.index(RULE)
    b = len(lines) - 1 - lines[::-1].index(RULE)
    assert b > a
    parts = []
    for l in lines[a + 1:b]:
        if l.startswith("database part "):
            parts.append((l, []))
        else:
            if not parts:
                parts.append((None, []))
            parts[-1][1].append(l)
    return lines[:a + 1], parts, lines[b:]


def canonical(lines):
    """the comparison of the command-line tests: lines between the rules sorted within their part (the reference walks its own hash
    slots), the part headers in place, every other line as it is"""
    head, parts, tail = split_output(drop_version(lines))
    body = []
    for header, ls in parts:
        if header is not None:
            body.append(header)
        body.extend(sorted(ls))
    return head + body + tail


@functools.lru_cache(maxsize=None)
def counts_of(db):
    """[per part: {feature: size}] from the recorded featurecounts lines"""
    _, parts, _ = split_output(golden()["featurecounts_" + db]["stdout"])
    out = []
    for _, ls in parts:
        d = {}
        for l in ls:
            k, v = l.split(" -> ")
            d[int(k)] = int(v)
        assert len(d) == len(ls)
        out.append(d)
    return out


@functools.lru_cache(maxsize=None)
def lists_of(db):
    """[per part: {feature: [(tgt, win), ...]}] from the recorded featuremap lines"""
    _, parts, _ = split_output(golden()["featuremap_" + db]["stdout"])
    out = []
    for _, ls in parts:
        d = {}
        for l in ls:
            k, v = l.split(" -> ")
            d[int(k)] = [tuple(int(x) for x in p.split(",")) for p in v.strip("()").split(")(")]
        assert len(d) == len(ls)
        out.append(d)
    return out


def size_blocks(db):
    """the recorded statistics blocks: [{'title': None | 'database part 1 / 2:' | 'complete database (all parts):', 'buckets': line, ...}]
    in the order printed (a database of several parts: its parts, then the complete database)"""
    lines = golden()["statistics_" + db]["stdout"]
    blocks = []
    for i, l in enumerate(lines):
        if l.startswith("buckets  "):
            title = lines[i - 1] if lines[i - 1].endswith(":") else None
            blk = {"title": title}
            for m in lines[i:i + 5]:
                blk[m[:19].strip()] = m
            blocks.append(blk)
    return blocks


def histogram(sizes):
    h = [0] * 256
    for s in sizes:
        h[s] += 1
    return h


def size_lines(st, buckets=None):
    """the lines of a statistics block from api.table_statistics' result, worded and formatted (%g: an ostream's six digits) as
    print_content_properties does"""
    return {"buckets": "buckets            %d" % (st["buckets"] if buckets is None else buckets),
            "bucket size": "bucket size        max: %g mean: %g +/- %g <> %g" % (st["max"], st["mean"], st["stddev"], st["skewness"]),
            "features": "features           %d" % st["features"],
            "locations": "locations          %d" % st["locations"]}
