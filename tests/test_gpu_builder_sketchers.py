"""GPU: the builder's sketchers against the plain model (sketch_ref.py), by the method of test_builder_buckets_files_and_queries: the
written files, read back by the oracle's reader, hold for every feature exactly the model's (target, window) list in insertion order.

Parameter sets (sketch_cases.BUILD_PARAMS): build_sketch_lanes_kernel with the batched and the generic lane sketcher,
sketch_only_kernel<false> where the stride is no multiple of 4 or the sketch exceeds a lane's registers.  Targets: full records of 256
windows with and without the tail window the last lane takes too, one window more and less, and a target whose only window with a
repeated hash flags one record for sketch_only_kernel<true> while the next record is not flagged."""
import ctypes as C

import numpy as np
import pytest

import cpuref
import sketch_cases as sc
from metacache_amd import api

pytestmark = pytest.mark.gpu


def target_windows(bld, t):
    n = C.c_uint64()
    L = api.lib()
    L.mc_build_target_windows.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_uint64)]
    bld._check(L.mc_build_target_windows(bld.h, t, C.byref(n)))
    return n.value


@pytest.mark.parametrize("params", sc.BUILD_PARAMS, ids=str)
def test_builder_buckets_match_the_model(tmp_path, params):
    k, s, w, stride = params
    targets, model = sc.build_targets(params), sc.build_model(params)
    # (model facts: the tandem target flags exactly one record)
    tandem = [m for (name, _), m in zip(targets, model) if name == "tandem_in_one_window"][0]
    assert np.flatnonzero(tandem.dup).tolist() == [sc.TANDEM_WINDOW]

    bld = api.Builder(kmerlen=k, sketchlen=s, winlen=w, winstride=stride, target_id_bytes=4, max_candidates=2)
    db = None
    try:
        for i, (name, t) in enumerate(targets):
            bld.add_target(t, f"{name}.1", parent_taxid=1000, filename=f"f{i}.fa")
        db = bld.finish(load=True)
        n_locations = db.n_locations
        for t, m in enumerate(model):
            assert target_windows(bld, t) == len(m.counts), (params, targets[t][0])
        name = str(tmp_path / "built")
        bld.write(name, [(1, 1, 20, "root"), (1000, 1, 4, "species")])
    finally:
        bld.free()
        if db is not None:
            db.close()

    # feature -> first 254 (target, window) in insertion order
    expect = {}
    for t, m in enumerate(model):
        for win in range(len(m.counts)):
            for f in m.feats[win, :m.counts[win]]:
                expect.setdefault(int(f), []).append((t << 32) | win)
    odb = cpuref.oracle().open(name)
    try:
        assert (odb.k, odb.s, odb.w, odb.stride) == params and odb.n_targets == len(targets)
        nloc = 0
        for f, locs in expect.items():
            want = np.array(locs[:254], dtype=np.uint64)
            got = odb.lookup(f)
            if not np.array_equal(got, want):
                bad = int(want[0]) if len(got) == 0 else int(next((a for a, b in zip(want, got) if a != b), want[min(len(got), len(want) - 1)]))
                raise AssertionError((params, "feature", f, "target", targets[bad >> 32][0], "window", bad & 0xFFFFFFFF, "got", got.tolist()[:8], "want", want.tolist()[:8]))
            nloc += len(want)
        assert odb.n_locations == nloc == n_locations
        keys, sizes, _, _ = odb.part_arrays(0)                                              # no feature too many
        extra = np.setdiff1d(keys[sizes > 0], np.array(sorted(expect), dtype=np.uint32))
        assert extra.size == 0, (params, extra[:8].tolist())
    finally:
        odb.close()
