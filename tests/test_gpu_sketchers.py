"""GPU: every query-side sketcher against the plain model (sketch_ref.py) -- window offsets and every sketch row, padding included,
bit-exact -- on the parameter grid and the generated reads of sketch_cases.py, once per route:

    lanes apart    sketch_lane_kernel, chunk_sketch_kernel for the long single reads it cuts, what a lane flags redone by query_kernel
    lanes fused    sketch_probe_lane_kernel, the same chunks and hand-over
    wave           query_kernel<true>
    wave, allhits  query_kernel<false>

The inputs reach the rare branches (sketch_window_v3's serial minimum, raised threshold and carried sketch; the lanes' hand-over of a
read, of one chunk of a long read): sketch_cases.coverage(), asserted from the model before the device is touched.  The model itself is
pinned to the reference's vectors and to the oracle in test_sketch_ref_cpu.py."""
import numpy as np
import pytest

import sketch_cases as sc
from metacache_amd import api, synth

pytestmark = pytest.mark.gpu

WAVE_TIMER = "query_wave"
LANE_TIMERS = ("sketch_lane", "sketch_probe", "chunk_sketch")


def pack(reads):
    """[(mate1, mate2)] -> (characters with 16 slack bytes, qinfo[n, 4], characters used): every sequence starts 4-byte aligned"""
    chunks, info, pos = [], [], 0
    for a, b in reads:
        first = pos
        for x in (a, b):
            chunks.append(x + b"\0" * (-len(x) % 4))
            pos += len(chunks[-1])
        info.append((first, len(a), first + len(a) + (-len(a) % 4) if b else first, len(b)))
    buf = np.frombuffer(b"".join(chunks) + b"\0" * 16, dtype=np.uint8).copy()
    return buf, np.array(info, dtype=np.uint32).reshape(-1, 4), pos


def table_for(params):
    """three random 2 kbp targets under the set's sketching parameters (what is in the table does not matter)"""
    k, s, w, stride = params
    rng = np.random.default_rng(3)
    bld = api.Builder(kmerlen=k, sketchlen=s, winlen=w, winstride=stride, max_candidates=2)
    try:
        for i in range(3):
            bld.add_target(synth.random_genome(rng, 2000), f"T{i}.1", parent_taxid=0)
        db = bld.finish(load=True)
    finally:
        bld.free()
    assert (db.k, db.s, db.w, db.stride) == params
    return db


class Batch:
    """one packed batch on the device; run() -> (win_offsets[n + 1], features[windows, s]) of a query_device call"""

    def __init__(self, reads):
        import torch
        self.n = len(reads)
        buf, info, self.chars = pack(reads)
        self.dseq = torch.from_numpy(buf).cuda()
        self.dq = torch.from_numpy(info.view(np.int32).reshape(-1)).cuda()

    def run(self, db, s, **kw):
        res = db.query_device(self.dseq.data_ptr(), self.dq.data_ptr(), self.n, self.chars, max_win_uniform=3, want_features=True, **kw)
        db.synchronize()
        wo = np.zeros(self.n + 1, dtype=np.uint32)
        db.copy_results(wo.ctypes.data, res.win_offsets, wo.nbytes, to_host=True)
        db.synchronize()
        f = np.zeros((int(wo[-1]), s), dtype=np.uint32)
        if f.size:
            db.copy_results(f.ctypes.data, res.features, f.nbytes, to_host=True)
            db.synchronize()
        return wo.astype(np.int64), f


def assert_sketches(names, model_rows, wo, f, what):
    """win_offsets = scan of the model's window counts; every row = the model's row"""
    want_wo = np.concatenate(([0], np.cumsum([len(m) for m in model_rows]))).astype(np.int64)
    bad = np.flatnonzero(wo != want_wo)
    assert bad.size == 0, (what, "win_offsets", names[max(int(bad[0]) - 1, 0)] if bad.size else None)
    want = np.concatenate(model_rows) if len(model_rows) else np.zeros((0, f.shape[1]), dtype=np.uint32)
    assert f.shape == want.shape, (what, f.shape, want.shape)
    rows = np.flatnonzero((f != want).any(axis=1))
    if rows.size:
        r = int(rows[0])
        q = int(np.searchsorted(want_wo, r, side="right")) - 1
        raise AssertionError((what, names[q], "window", r - int(want_wo[q]), "got", f[r].tolist(), "want", want[r].tolist(), "rows wrong", int(rows.size)))


def launches(db, name):
    return db.timing_get(name)[1]


@pytest.mark.parametrize("params", sc.QUERY_PARAMS, ids=str)
def test_every_route_matches_the_model(params):
    k, s, w, stride = params
    reads, model = sc.query_reads(params), sc.query_model(params)
    cov = sc.coverage()
    assert all(cov.values()), [c for c, v in cov.items() if not v]      # the grid's inputs reach the branches (model facts only)
    names = [name for name, _, _ in reads]
    rows = [m.feats for m in model]
    total = sum(len(r) for r in rows)
    lanes = sc.lane_path_supported(*params)
    assert any(len(b) > sc.LANE_MAX_LEN for _, _, b in reads)           # (a pair no lane takes: the wave kernel has work on every route)

    db = table_for(params)
    try:
        batch = Batch([(a, b) for _, a, b in reads])
        db.timing(True)
        routes = (("lanes apart", dict(lane_path=1, lane_fusion=0), {}), ("lanes fused", dict(lane_path=1, lane_fusion=1), {}),
                  ("wave", dict(lane_path=0), {}), ("wave, allhits", dict(lane_path=0), dict(want_allhits=True)))
        for what, tuning, kw in routes:
            for name, value in tuning.items():
                db.set_tuning(name, value)
            db.timing_reset()
            wo, f = batch.run(db, s, **kw)
            assert_sketches(names, rows, wo, f, (params, what))
            assert db.last_batch_stats()["windows"] == total, (params, what)
            ran = {t: launches(db, t) for t in LANE_TIMERS + (WAVE_TIMER,)}
            if what.startswith("lanes") and lanes:
                apart = what == "lanes apart"
                assert ran["sketch_lane"] == (1 if apart else 0) and ran["sketch_probe"] == (0 if apart else 1), (params, what, ran)
                # The chunk stage's timer runs on every lane-path batch, cut reads or none: it shows that the lane stage ran, not that
                # chunk_sketch_kernel took a read (the call hands out no chunk counter).  That the long single reads of the sets with
                # stride % 4 == 0 are cut follows from lane_chunk_records' rule (sketch_cases.chunked), which this test cannot observe.
                assert ran["chunk_sketch"] == 1, (params, what, ran)
                assert ran[WAVE_TIMER] >= 1, (params, what, ran)
            else:                                                        # the wave routes, and what collapses into them
                assert ran["sketch_lane"] == ran["sketch_probe"] == ran["chunk_sketch"] == 0 and ran[WAVE_TIMER] == 1, (params, what, ran)
    finally:
        db.close()


def test_plan_kernels_at_their_switch():
    """plan_scan_small_kernel takes batches of up to 32 768 reads, plan_kernel and the three-kernel scan larger ones: one batch on
    either side, reads of 0 .. 40 bases (0 or 1 window each), exact window offsets and sketches"""
    import sketch_ref
    params = (16, 16, 127, 112)
    pool_rows = [sketch_ref.sketch(r, *params)[0] for r in sc.plan_pool()]
    row_of = {r: f for r, f in zip(sc.plan_pool(), pool_rows)}
    db = table_for(params)
    try:
        for n in (sc.SMALL_PLAN, sc.SMALL_PLAN + 1):
            reads = sc.plan_switch_reads(n)
            rows = [row_of[r] for r in reads]
            wo, f = Batch([(r, b"") for r in reads]).run(db, 16)
            assert_sketches([f"read_{i}" for i in range(n)], rows, wo, f, n)
            assert db.last_batch_stats()["windows"] == sum(len(r) for r in rows)
            assert 0 < wo[-1] < n
    finally:
        db.close()
