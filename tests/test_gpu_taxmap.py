"""GPU: mc_taxmap_* (taxmap.hip), the device form and MC_TAXMAP_HOST, against the model (taxmap_ref.Model), which
test_taxmap_witness_cpu.py holds to the reference's own `build -taxpostmap`.  Every case of taxmap_cases.cases(), built around the tile
T = api.taxmap_tile() and the longest line M = api.taxmap_max_line(): the status of every call, every name's taxid and position and the
number of names still wanted, bit for bit.  Every device output sits between guard zones.  A regular input that the device refuses
FAILS here: there is no skip and no fall-back."""
import numpy as np
import pytest

import taxmap_cases as cases
import taxmap_ref as ref
from metacache_amd import api

pytestmark = pytest.mark.gpu
GUARD, FILL = 64, 0xA5
FILL64 = int(np.array([FILL] * 8, dtype=np.uint8).view(np.int64)[0])


@pytest.fixture(scope="module")
def all_cases():
    assert api.taxmap_tile() == 4096 and api.taxmap_max_line() == ref.MAX_LINE     # (what the model and the CPU tests assume)
    return cases.cases(api.taxmap_tile(), api.taxmap_max_line())


@pytest.fixture(scope="module")
def expected(all_cases):
    """the model's statuses and result of every case, computed once"""
    out = {}
    for name, (names, wanted, ranges) in all_cases.items():
        m = ref.Model(names, wanted, api.taxmap_max_line())
        out[name] = ([m.add(r) for r in ranges], m.result())
    return out


@pytest.fixture(scope="module")
def tm():
    m = api.TaxonMapper()
    yield m
    m.close()


class Guarded:
    """a device array of `elems` 8-byte words between two guard zones"""

    def __init__(self, elems):
        import torch
        self.torch, self.elems = torch, elems
        self.t = torch.full((GUARD + elems + GUARD,), FILL64, dtype=torch.int64, device=torch.device("cuda", 0))
        torch.cuda.synchronize()                               # (the fill runs on torch's stream, the library on the context's)

    @property
    def ptr(self):
        return self.t.data_ptr() + 8 * GUARD

    def get(self, dtype=np.uint64):
        self.torch.cuda.synchronize()
        raw = self.t.cpu().numpy().view(np.uint8)
        assert np.all(raw[:8 * GUARD] == FILL) and np.all(raw[8 * (GUARD + self.elems):] == FILL), "bytes outside the array were written"
        return raw[8 * GUARD:8 * (GUARD + self.elems)].view(dtype).copy()


def add_on_device(tm, data):
    """one range through the device form -> its status, read back between guards"""
    import torch
    dev = torch.device("cuda", 0)
    d = torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).to(dev)
    assert d.data_ptr() % 16 == 0
    wsb = api.taxmap_scratch_bytes(len(data))
    ws = torch.full((wsb + GUARD,), FILL, dtype=torch.uint8, device=dev)
    st = Guarded(8)
    tm.add_device(d.data_ptr(), d.numel(), status_ptr=st.ptr, workspace_ptr=ws.data_ptr(), workspace_bytes=wsb)
    api.lib().mc_synchronize(tm.h)
    status = [int(x) for x in st.get()]
    assert np.all(ws.cpu().numpy()[wsb:] == FILL), "bytes behind the workspace were written"
    return status


def result_on_device(tm):
    n = max(tm.count, 1)
    T, P = Guarded(n), Guarded(n)
    tm.result_device(taxid_ptr=T.ptr, position_ptr=P.ptr)
    api.lib().mc_synchronize(tm.h)
    return T.get(np.int64)[:tm.count], P.get()[:tm.count]


def run_case(tm, case, expected, device):
    names, wanted, ranges = case
    statuses, (taxid, key, remaining) = expected
    tm.begin(names, wanted)
    for i, (r, want) in enumerate(zip(ranges, statuses)):
        got = add_on_device(tm, r) if device else tm.add(r)
        assert got == want, ("status of call", i, got, want)
    t_host, p_host, rem = tm.result()
    assert rem == remaining
    assert [int(x) for x in t_host] == taxid and [int(x) for x in p_host] == key
    if device:
        t_dev, p_dev = result_on_device(tm)
        assert np.array_equal(t_dev, t_host) and np.array_equal(p_dev, p_host)


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", sorted(cases.cases()))           # (the names only: the cases themselves come from the fixture)
def test_case_equals_the_model(tm, all_cases, expected, name, device):
    run_case(tm, all_cases[name], expected[name], device)


def test_the_cases_cover_what_they_are_there_for(all_cases, expected):
    T = api.taxmap_tile()
    st, (taxid, key, _) = expected["tile_borders"]
    assert key == [T - 1, 2 * T, 3 * T + 1, 5 * T - 10] and taxid == [11, 12, 13, 14]
    st, (taxid, key, _) = expected["two_tiles_two_calls"]
    assert key[:3] == [0, T + 7 + 25, (1 << 32) + 50] and taxid[:3] == [71, 73, 76]
    st, (taxid, key, _) = expected["refused_between"]
    assert [s[5] for s in st] == [ref.OK, ref.IRREGULAR, ref.OK] and key[:3] == [0, ref.NOT_FOUND, 2 << 32] and taxid[:3] == [81, 0, 84]
    assert expected["max_line"][0][0][5] == ref.OK and expected["max_line_no_newline"][0][0][5] == ref.OK
    for name in ("max_line_plus_one_blank", "max_line_plus_one_token", "max_line_plus_one_no_newline", "taxid_19_digits"):
        assert expected[name][0][0][5:7] == [ref.IRREGULAR, 24], name
    assert expected["taxid_0_and_18_digits"][1][0][:3] == [0, 999999999999999999, 7] and expected["taxid_0_and_18_digits"][1][1][0] == 0
    assert expected["all_ranked_then_more"][0][1][3:5] == [0, 0]
    assert sum(1 for n in all_cases if n.startswith("irregular_")) >= 15
    for zone, L in (("one_tile", 208), ("tile_border", T - 8)):                 # ranges that end at every place of a thread's 16 bytes
        st, (taxid, key, _) = expected["tail_sweep_" + zone]
        assert [s[5] for s in st] == [ref.OK] * 32 and taxid == [500 + j for j in range(32)]
        assert [len(r) for r in all_cases["tail_sweep_" + zone][2]][0::2] == list(range(L, L + 16))
        assert [s[5:7] for s in expected["irregular_last_byte_" + zone][0]] == [[ref.IRREGULAR, L + i - 1] for i in range(16)]
    assert expected["random_20000x300"][0][0][0] + expected["random_20000x300"][0][1][0] == 20000


def test_stats_count_accepted_and_refused_ranges():
    m = api.TaxonMapper()
    try:
        m.begin([b"P_000001.1", b"P_000002.1"], [1, 0])
        good, bad = b"P_000001 P_000001.1 5 1\nP_000002 P_000002.1 6 1\nq q 1 q\n", b"P_000001 P_000001.1 5\n"
        assert m.add(good)[:6] == [3, 2, 1, 1, 0, ref.OK]
        assert m.add(bad)[5] == ref.IRREGULAR
        assert m.stats() == [2, len(good) + len(bad), 3, 2, 1, 1, 1, 0]
        m.begin([b"P_000001.1"])                                 # a new table: every name unfound again, the counters go on
        taxid, position, remaining = m.result()
        assert int(position[0]) == api.TAXMAP_NOT_FOUND and remaining == 1
    finally:
        m.close()


def test_add_file_drops_the_first_line_and_cuts_at_line_ends(tmp_path):
    names = cases.numbered(65)
    rows = b"".join(cases.row(b"N%06d" % i, b"N%06d.1" % i, 100 + i, b"0") for i in range(64))
    path = tmp_path / "t.accession2taxid"
    path.write_bytes(b"N000064\tN000064.1\t7\t0\n" + rows)      # the first line names a target and is dropped all the same
    m = api.TaxonMapper()
    try:
        m.begin(names)
        statuses = m.add_file(str(path), piece_bytes=100)        # 24-byte rows: four to a piece
        assert len(statuses) == 16 and all(s[:6] == [4, 4, 4, 4, 65 - 4 * (i + 1), ref.OK] for i, s in enumerate(statuses))
        taxid, position, remaining = m.result()
        assert remaining == 1 and [int(x) for x in taxid] == [100 + i for i in range(64)] + [0]
        assert [int(p) for p in position[:64]] == [((i // 4) << 32) + 24 * (i % 4) for i in range(64)]
    finally:
        m.close()
