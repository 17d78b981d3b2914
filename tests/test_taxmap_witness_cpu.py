"""CPU: the model of the ranking pass (taxmap_ref) against the reference's own `build -taxpostmap`, and the argument checks of
mc_taxmap_* that need no device.

  * the witness: a dozen 400 bp records and a table with an exact accession.version, a similar accession that beats a later exact row, a
    name equal to an accession that is skipped for the next longer one, a '!1' duplicate left unranked because its row's target was ranked
    already, a gi match, a row for a target that is not wanted, and a three-token row that shifts the tokens and ends the loop.  The
    parents the reference wrote are recorded in golden/taxmap_expected.json; the model must give them, and where the compiled reference
    is present it is run again and must give them too;
  * golden/build_in/taxonomy/toy.accession2taxid against the parents of build_expected.json.gz, cases default and reset_taxa;
  * the line rule's model and the token stream give the same parents on every range of the device tests that the line rule accepts;
  * every MC_ERR_INVALID of mc_taxmap_* comes before any device call, then MC_ERR_STATE names what an mc_open_metadata context lacks."""
import ctypes as C
import gzip
import json
import os

import numpy as np
import pytest

import taxmap_cases as cases
import taxmap_ref as ref
from metacache_amd import api

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF32 = os.path.join(ROOT, "oracle", "_ref", "metacache_u32")
INVALID, STATE = -1, -6

with open(os.path.join(cases.GOLDEN, "taxmap_expected.json")) as f:
    RECORDED = {k.encode(): v for k, v in json.load(f)["parents"].items()}


def model_parents(before, files, reset=False):
    """{name: parent} after the pass over `files` for targets that had the parents `before`"""
    names = sorted(before)
    wanted = [reset or before[n] == 0 for n in names]
    ranked = ref.rank_stream(names, wanted, files)
    return {n: ranked.get(i, before[n]) for i, n in enumerate(names)}


def test_model_gives_the_recorded_parents():
    before = {n: (562 if n == b"AH_000008.1" else 0) for n in RECORDED}          # (the only record with a taxid in its header)
    assert len(RECORDED) == 12
    assert model_parents(before, [cases.WITNESS_TABLE]) == RECORDED
    # what the rows are there for
    assert RECORDED[b"AA_000001.1"] == 100 and RECORDED[b"AB_000002.1"] == 200 and RECORDED[b"AC_000003"] == 0 and RECORDED[b"AC_000003.1"] == 300
    assert RECORDED[b"AD_000004.1"] == 400 and RECORDED[b"AD_000004.1!1"] == 0 and RECORDED[b"77777"] == 500 and RECORDED[b"AH_000008.1"] == 562
    assert RECORDED[b"AE_000005.1"] == 600 and RECORDED[b"AF_000006.1"] == 0 and RECORDED[b"AG_000007.1"] == 0


@pytest.mark.skipif(not os.path.exists(REF32), reason="the compiled reference (oracle/_ref/metacache_u32) is not here")
def test_reference_itself_gives_the_recorded_parents(tmp_path):
    assert cases.run_witness(REF32, str(tmp_path)) == RECORDED


@pytest.mark.parametrize("case", ["default", "reset_taxa"])
def test_model_on_the_toy_table_gives_the_golden_parents(case):
    with gzip.open(os.path.join(cases.GOLDEN, "build_expected.json.gz"), "rt") as f:
        exp = json.load(f)["build"]
    targets = lambda c: {v[2].encode(): v[0] for k, v in exp[c]["db"]["taxa"].items() if int(k) < 0 and v[1] == 0}
    after = targets(case)
    # the parents in front of the pass: those of the build without -taxonomy, whose pass finds no table; a target that has a parent there has
    # it in `case` too (the taxonomy's own id table only ranks further ones, and no row of the toy table names one of those)
    before = targets("no_taxonomy")
    assert set(before) == set(after) and len(after) >= 10
    with open(os.path.join(cases.GOLDEN, "build_in", "taxonomy", "toy.accession2taxid"), "rb") as f:
        table = f.read()
    names = sorted(after)
    wanted = [case == "reset_taxa" or before[n] == 0 for n in names]
    ranked = ref.rank_stream(names, wanted, [None, table])                       # (a table that cannot be opened is passed over)
    assert len(ranked) >= 3
    for i, taxid in ranked.items():
        assert after[names[i]] == taxid, (case, names[i])
    for i, n in enumerate(names):                                                # ... and whom the pass left alone kept what it had
        if i not in ranked and not (case == "reset_taxa"):
            assert before[n] == 0 or after[n] == before[n], (case, n)
    m = ref.Model(names, wanted)
    st = m.add(table[table.index(b"\n") + 1:])
    assert st[5] == ref.OK and st[3] == len(ranked)
    assert {i: t for i, (t, k) in enumerate(zip(*m.result()[:2])) if k != ref.NOT_FOUND} == ranked


ALL = cases.cases()


@pytest.mark.parametrize("case", sorted(ALL))
def test_line_rule_never_reads_an_accepted_range_differently(case):
    names, wanted, ranges = ALL[case]
    m = ref.Model(names, wanted)
    statuses = [m.add(r) for r in ranges]
    if case.startswith("irregular_") or "plus_one" in case or case in ("much_too_long", "taxid_19_digits", "one_byte_lines"):
        assert [s[5] for s in statuses] == [ref.IRREGULAR] * len(ranges), case
        return
    accepted = [r for r, s in zip(ranges, statuses) if s[5] == ref.OK]
    assert accepted and (len(accepted) == len(ranges) or case == "refused_between")
    table = b"first line\n" + b"".join(r if r.endswith(b"\n") else r + b"\n" for r in accepted)
    taxid, key, _ = m.result()
    assert {i: t for i, (t, k) in enumerate(zip(taxid, key)) if k != ref.NOT_FOUND} == ref.rank_stream(names, m.wanted, [table]), case


def test_argument_checks_need_no_device():
    L = api.lib()
    h = C.c_void_p()
    assert L.mc_open_metadata(os.path.join(cases.GOLDEN, "toy32").encode(), C.byref(h)) == api.MC_OK
    try:
        assert api.taxmap_tile() >= 256 and api.taxmap_max_line() >= 256 and api.taxmap_scratch_bytes(100) >= 64
        text = np.frombuffer(b"AAB\0", dtype=np.uint8).copy()
        off = np.array([0, 1, 3], dtype=np.uint64)
        flags = np.ones(2, dtype=np.uint8)

        def begin(ctx=h, names=text.ctypes.data, offsets=off, count=2, wanted=flags.ctypes.data):
            return L.mc_taxmap_begin(ctx, names, None if offsets is None else offsets.ctypes.data, count, wanted)

        assert begin(ctx=None) == INVALID and begin(offsets=None) == INVALID and begin(wanted=None) == INVALID and begin(names=None) == INVALID
        assert begin(count=1 << 31) == INVALID
        assert begin(offsets=np.array([0, 3, 1], dtype=np.uint64)) == INVALID and b"descend" in L.mc_last_error(h)
        for bad in (b"BA", b"AA"):                                                 # descending, equal
            t2 = np.frombuffer(bad + b"\0", dtype=np.uint8).copy()
            assert begin(names=t2.ctypes.data, offsets=np.array([0, 1, 2], dtype=np.uint64)) == INVALID and b"ascend strictly" in L.mc_last_error(h)
        t3 = np.frombuffer(b"ABA\0", dtype=np.uint8).copy()                        # "AB" in front of its prefix "A"
        assert begin(names=t3.ctypes.data, offsets=np.array([0, 2, 3], dtype=np.uint64)) == INVALID
        assert begin() == STATE and b"no device" in L.mc_last_error(h)             # "A" < "AB": regular names, the context has no device
        assert begin(count=0, wanted=None, names=None, offsets=np.zeros(1, dtype=np.uint64)) == STATE

        data = np.frombuffer(b"a b 1 c\n" + b"\0" * 64, dtype=np.uint8).copy()
        buf = np.zeros(1024, dtype=np.uint64)                                      # (its address is only compared, never read: no device)
        base = buf.ctypes.data + (-buf.ctypes.data) % 16
        status = np.zeros(8, dtype=np.uint64)
        need = api.taxmap_scratch_bytes(8)

        def add(ctx=h, bytes_ptr=data.ctypes.data, nbytes=8, flags=api.TAXMAP_HOST, status_ptr=status.ctypes.data, ws=None, ws_bytes=0):
            return L.mc_taxmap_add(ctx, bytes_ptr, nbytes, flags, status_ptr, ws, ws_bytes, None)

        assert add(ctx=None) == INVALID
        assert add(bytes_ptr=None) == INVALID and add(nbytes=0) == INVALID and add(nbytes=(1 << 31) + 1) == INVALID
        assert add(flags=2) == INVALID and add(flags=api.TAXMAP_HOST | 4) == INVALID and add(status_ptr=None) == INVALID
        dev = dict(flags=0, bytes_ptr=base + 1024, status_ptr=base + 2048, ws=base + 4096, ws_bytes=need)
        assert add(**{**dev, "ws": None}) == INVALID and add(**{**dev, "ws_bytes": need - 1}) == INVALID
        assert add(**{**dev, "bytes_ptr": base + 1025}) == INVALID and add(**{**dev, "ws": base + 4100}) == INVALID
        assert add(**{**dev, "status_ptr": base + 2052}) == INVALID
        assert add(**dev) == STATE and add() == STATE and b"no device" in L.mc_last_error(h)
        assert not status.any()

        out = np.zeros(4, dtype=np.uint64)
        rem = C.c_uint64(7)
        assert L.mc_taxmap_result(None, out.ctypes.data, None, None, api.TAXMAP_HOST, None) == INVALID
        assert L.mc_taxmap_result(h, out.ctypes.data, None, None, 2, None) == INVALID
        assert L.mc_taxmap_result(h, base + 4, None, None, 0, None) == INVALID and L.mc_taxmap_result(h, base, base + 12, None, 0, None) == INVALID
        assert L.mc_taxmap_result(h, base, base + 64, C.byref(rem), 0, None) == INVALID
        assert L.mc_taxmap_result(h, out.ctypes.data, None, C.byref(rem), api.TAXMAP_HOST, None) == STATE and rem.value == 7

        st = np.ones(8, dtype=np.uint64)
        assert L.mc_taxmap_stats(h, st.ctypes.data) == 0 and not st.any() and L.mc_taxmap_stats(h, None) == INVALID
        L.mc_taxmap_end(h)
        L.mc_taxmap_end(None)
    finally:
        L.mc_destroy(h)


def test_every_entry_point_is_exported():
    for name in ("mc_taxmap_begin", "mc_taxmap_scratch_bytes", "mc_taxmap_add", "mc_taxmap_result", "mc_taxmap_stats", "mc_taxmap_end"):
        assert name in api.EXPORTS and hasattr(api.lib(), name)
