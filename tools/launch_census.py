"""Which timed steps of the per-batch pipeline (csrc/query_pipe.cpp) run for which kind of batch: a fixed list of small batches, per case and
batch {timer name: count} from mc_timing_get.  The counts are decided by the host's batch plan (csrc/query_rules.h) and by the batch's
work-list counters -- not by the clock --, so a change of the host code that is meant to leave the launches alone must leave every one
of them as it is: tests/test_gpu_launch_census.py compares with tests/golden/launch_census.json.

    python tools/launch_census.py --commit <hash of the tree the library was built from> --out tests/golden/launch_census.json"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# every ScopedTimer name of the per-batch pipeline and the owner-side entry points
TIMERS = ("plan", "sketch_lane", "sketch_probe", "chunk_sketch", "mask_features", "chunk_probe", "probe_cands",
          "mid_cands_64", "mid_cands_128", "mid_cands_256", "hash_cands_256", "hash_cands_512", "hash_cands_1024",
          "query_wave", "scan", "gather_lists", "sort_candidates", "pack_numbers",
          "gw_filter_count", "gw_filter", "big_filter", "gw_filter2", "gw_compact", "gw_filter_stream_fine", "gw_filter_stream_mid", "gw_filter_stream",
          "big_filter_2", "gw_count", "big_count", "gw_count_512", "gw_count_1024", "big_count_2", "gw_sort", "gw_sorted_cands",
          "cands_from_hits", "owner_entries", "decode_union")
CASES = ("01_synchronous", "02_taxon_key", "03_deferred_tail", "04_all_hits", "05_partial_hits", "06_partial_numbers", "07_features",
         "08_lane_path_off", "09_lane_kernels_apart", "10_lane_kernels_fused", "11_counting_apart", "12_lane_candidates_unsupported",
         "13_wide_store", "14_filter_lookup", "15_slot_short_reads", "16_slot_long_read", "17_owner_partial_hits", "18_owner_partial_numbers")
SKIPPABLE = ("14_filter_lookup",)                                # only where the device had no room for the direct index
LENGTHS = ((150,), (150, 300, 512), (700, 1500, 4000, 150), (150, 9000))
SHORT, MIXED, LONG = 0, 2, 3                                     # the batches the one-batch cases use


def collection():
    """the collection and the four batches of tests/test_gpu_pipeline.py's deferred-tail test: they reach the sorted class, the reads the filtered
    path hands back and the reads with duplicate hashes"""
    from metacache_amd import synth, synthdb
    spec = synthdb.phylogeny(4, 2, 10, 30_000, 40_000, seed=4242, div_strain=(0.002, 0.01))
    cs = synthdb.CpuSynth()
    rng = np.random.default_rng(5)
    batches = []
    for b, lens in enumerate(LENGTHS):
        reads = []
        for j, L in enumerate(lens):
            P = synthdb.read_params(spec, 2000 + 10 * b + j, read_len=L, sub_rate=0.03 if L > 600 else 0.01)
            reads += [bytes(r[:L]) for r in cs.reads(spec, P, 0, 400 if L <= 512 else 60)]
        reads += [bytes(synth.random_genome(rng, 300)) for _ in range(20)]
        reads += [b"ACGT" * 60, b"A" * 200]
        batches.append([reads[i] for i in rng.permutation(len(reads))])
    return spec, batches


def golden_reads():
    z = np.load(os.path.join(ROOT, "tests", "golden", "toy_reads.npz"))
    off = z["single_off"]
    return [z["single"][int(off[i]):int(off[i + 1])].tobytes() for i in list(range(0, 300)) + list(range(1595, 1650))]


def device_batch(reads, dev):
    import torch
    pad = [len(r) + (-len(r)) % 4 for r in reads]
    offs = np.concatenate([[0], np.cumsum(pad)]).astype(np.int64)
    buf = np.zeros(int(offs[-1]) + 16, dtype=np.uint8)
    for r, o in zip(reads, offs[:-1]):
        buf[o:o + len(r)] = np.frombuffer(r, dtype=np.uint8)
    qinfo = np.zeros((len(reads), 4), dtype=np.uint32)
    qinfo[:, 0] = offs[:-1]; qinfo[:, 1] = [len(r) for r in reads]; qinfo[:, 2] = offs[:-1]
    mw = np.array([2 + len(r) // 112 for r in reads], dtype=np.int32)
    return (torch.from_numpy(buf).to(dev), torch.from_numpy(qinfo.view(np.int32)).to(dev), torch.from_numpy(mw).to(dev), int(offs[-1]), len(reads))


def counts(db):
    db.synchronize()
    return {k: int(db.timing_get(k)[1]) for k in TIMERS}


def run_batches(db, dbatch, which, finish=False, **kw):
    """one mc_query_device call per batch -> {batch: {timer: count}}"""
    out = {}
    for i in which:
        seq, qi, mw, nch, n = dbatch[i]
        db.timing_reset()
        db.query_device(seq.data_ptr(), qi.data_ptr(), n, nch, max_win_ptr=mw.data_ptr(), **kw)
        if finish:
            db.query_finish()
        out[f"batch{i}"] = counts(db)
    return out


def build(spec, env=None, **cfg):
    from metacache_amd import synthdb
    env = dict(env or {}, MC_BIG_MIN="0")                        # every list above 64 locations takes the filtered path
    before = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        db, _ = synthdb.build_database(spec, shards=1, **cfg)
    finally:
        for k, v in before.items():
            os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
    db.set_lineages(spec.lineages())
    db.timing(True)
    return db


def run(device: int = 0) -> dict:
    """-> {"cases": {case: {batch: {timer: count}}}, "skipped": [cases that could not run]}"""
    import torch
    dev = torch.device("cuda", device)
    spec, batches = collection()
    dbatch = [device_batch(r, dev) for r in batches]
    torch.cuda.synchronize()
    every = range(len(dbatch))
    cases, skipped = {}, []

    db = build(spec, max_candidates=2)
    assert db.table_layout()["location_bytes"] == 4
    cases["01_synchronous"] = run_batches(db, dbatch, every)
    cases["02_taxon_key"] = run_batches(db, dbatch, every, lowest=4)
    cases["03_deferred_tail"] = run_batches(db, dbatch, every, finish=True, defer_tail=True)
    cases["04_all_hits"] = run_batches(db, dbatch, every, want_allhits=True)
    cases["05_partial_hits"] = run_batches(db, dbatch, every, want_partial_hits=True)
    cases["06_partial_numbers"] = run_batches(db, dbatch, every, want_partial_numbers=True)
    cases["07_features"] = run_batches(db, dbatch, every, want_features=True)
    for case, name, value, back in (("08_lane_path_off", "lane_path", 0, 1), ("09_lane_kernels_apart", "lane_fusion", 0, -1),
                                    ("10_lane_kernels_fused", "lane_fusion", 1, -1), ("11_counting_apart", "gw_fuse", 0, 1)):
        db.set_tuning(name, value)
        cases[case] = run_batches(db, dbatch, every)
        db.set_tuning(name, back)
    # the slot path (mc_batch_submit on a pipe the slot borrows): no read beyond a lane's reach / one such read
    for case, i in (("15_slot_short_reads", SHORT), ("16_slot_long_read", LONG)):
        db.timing_reset()
        db.query(batches[i])
        cases[case] = {f"batch{i}": counts(db)}
    # the owner side of Mode K, one source: the shard side's lists of the same batch, 8-byte locations / 4-byte window numbers
    seq, qi, mw, nch, n = dbatch[MIXED]
    res = db.query_device(seq.data_ptr(), qi.data_ptr(), n, nch, max_win_ptr=mw.data_ptr(), want_partial_hits=True)
    off = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    db.copy_results(off.data_ptr(), res.hit_offsets, (n + 1) * 8); db.synchronize()
    hits = torch.zeros(int(off[-1]) + 2, dtype=torch.int64, device=dev)
    db.copy_results(hits.data_ptr(), res.hits, int(off[-1]) * 8); db.synchronize()
    cnt = (off[1:] - off[:-1]).to(torch.int32).contiguous()
    db.timing_reset()
    db.candidates_from_partial_hits(cnt.data_ptr(), hits.data_ptr(), int(off[-1]), n, 1, max_win_ptr=mw.data_ptr())
    cases["17_owner_partial_hits"] = {f"batch{MIXED}": counts(db)}
    res = db.query_device(seq.data_ptr(), qi.data_ptr(), n, nch, max_win_ptr=mw.data_ptr(), want_partial_numbers=True)
    db.timing_reset()
    part, _ = db.partial_numbers(res, n, [0, n])
    db.synchronize()
    db.candidates_from_partial_numbers(part.counts, part.numbers, [0, int(part.total)], n, max_win_ptr=mw.data_ptr())
    cases["18_owner_partial_numbers"] = {f"batch{MIXED}": counts(db)}
    # the lane path's lookups inside the filter kernel: needs the direct index
    db.set_tuning("direct_index", 1)
    if db.table_layout()["direct_index"]:
        db.set_tuning("filter_lookup", 1)
        cases["14_filter_lookup"] = run_batches(db, dbatch, (SHORT, MIXED))
    else:
        skipped.append("14_filter_lookup")
    db.close()

    db = build(spec, max_candidates=5)                           # more candidates than the lane path delivers: wave kernels only
    cases["12_lane_candidates_unsupported"] = run_batches(db, dbatch, every)
    db.close()

    db = build(spec, env={"MC_COMPACT_LOCATIONS": "0"}, max_candidates=2)
    assert db.table_layout()["location_bytes"] == 8
    cases["13_wide_store"] = run_batches(db, [device_batch(golden_reads(), dev)], (0,))
    db.close()
    return {"cases": cases, "skipped": skipped}


def write(res: dict, path: str):
    """one line per batch, the timers in TIMERS' order"""
    rows = []
    for case in sorted(res["cases"]):
        batches = res["cases"][case]
        inner = ",\n".join(f"   {json.dumps(b)}: {json.dumps({k: batches[b][k] for k in TIMERS})}" for b in sorted(batches))
        rows.append(f"  {json.dumps(case)}: {{\n{inner}\n  }}")
    os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
    with open(path, "w") as f:
        f.write("{\n" + f" \"commit\": {json.dumps(res['commit'])},\n \"timers\": {json.dumps(list(TIMERS))},\n \"skipped\": {json.dumps(res['skipped'])},\n"
                " \"cases\": {\n" + ",\n".join(rows) + "\n }\n}\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit whose csrc the library was built from")
    ap.add_argument("--out", required=True)
    args = ap.parse_args()
    res = {"commit": args.commit, **run()}
    write(res, args.out)
    print(json.dumps({"cases": len(res["cases"]), "skipped": res["skipped"]}))


if __name__ == "__main__":
    main()
