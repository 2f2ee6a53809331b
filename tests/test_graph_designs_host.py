"""The designed topologies of tests/graph_designs.py -- hairpins, rings, tandem repeats, palindromic (K+1)-mers, tips at the clipping
boundary, bushes of nested tips -- through the host stages, against what the reference made of the same reads
(tests/golden/graph_designs_golden.py).  No GPU: the host path is the specification tests/test_gpu_graph_designs.py holds the device to.
Every run of the reference: the inputs are a few thousand nodes, a row takes a tenth of a second."""
import numpy as np
import pytest

from soapdenovo2_amd import api
import graph_designs as G

ROWS = G.rows()
TIP_ROWS = [r for r in ROWS if r[0] in ("tips", "all") or r[0].startswith("bush")]
ROOM_ROWS = [("tips", 31, 0, 3, 0), ("bush1", 31, 0, 3, 0)]               # PG_TIP_LIST_ROOM=1: every listing of two dead ends or more lists again


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("designs")


def test_the_designs_make_palindromic_edges():
    """The reference counts an edge that is its own reverse complement once and every other edge twice: `EDGEs` is odd or, as here, short of
    twice the records.  hairpin makes three such edges, pal_plus two (one of them the length-1 edge of the palindromic (K+1)-mer between a
    branch node and itself), tandem two -- the structures the edge builders' palindrome test is for."""
    rows = G.golden_rows()[0]
    for name, n in (("hairpin", 3), ("pal_plus", 2), ("tandem", 2)):
        for K, m in G.FLAVOURS:
            r = rows[G.row_tag((name, K, m, 3, 0))]
            assert 2 * r["edge_pairs"] - r["edges"] == n, (name, K, r["edges"], r["edge_pairs"])
    assert rows[G.row_tag(("pal_plus", 31, 0, 3, 0))]["length1_records"] == 1


@pytest.mark.parametrize("serial", [False, True], ids=["all-threads", "sequential"])
@pytest.mark.parametrize("row", [r for r in ROWS if r[0] in ("hairpin", "pal_plus") and r[3] == 3], ids=G.row_tag)
def test_both_host_edge_builders_on_palindromic_edges(row, serial, work, tmp_path, monkeypatch):
    """A palindromic edge passes its interior nodes twice, there and back: the builder of all host threads (the default) tags them once and
    writes what the sequential builder (PG_SERIAL_EDGES=1) and the reference write."""
    if serial:
        monkeypatch.setenv("PG_SERIAL_EDGES", "1")
    test_host_files_equal_the_reference(row, work, tmp_path)


@pytest.mark.parametrize("row", ROWS, ids=G.row_tag)
def test_host_files_equal_the_reference(row, work, tmp_path):
    """oracle records -> layout replay, tips, edges, pass 2 with -R on the host: all seven files as the reference wrote them, and its counts."""
    name, K, m, P, D = row
    want = G.golden_rows()[0][G.row_tag(row)]
    codes, lens, rec, last, opre = G.row_inputs(row, work)
    pre = str(tmp_path / "h")
    nv, ne, na = api.host_pregraph_files(rec, last, codes, lens, K, P, pre, mer127=bool(m), cut_single=(D == 0), max_read_len=G.max_rd_len(K),
                                         batches=2, resolve_repeats=True)
    got = G.seven_digests(pre, kmerfreq_of=opre)                          # (the .kmerFreq is pass 1's: the oracle's)
    if D == 0:
        assert len(rec) == want["nodes"]
    assert (nv, na) == (want["vertices"], want["pre_arcs"])
    for ext in G.SEVEN:
        assert got[ext] == want["md5"][ext], (G.row_tag(row), ext)


@pytest.mark.parametrize("threads,places", [(1, 1), (5, 1), (5, 3)])
@pytest.mark.parametrize("row", TIP_ROWS, ids=G.row_tag)
def test_device_tip_decisions_equal_the_scan_and_the_reference(row, threads, places, work, monkeypatch):
    """dev_tips.hpp on the HostBackend against the sequential slot-order scan where the candidates interact: the totals of both passes equal
    the scan's and the reference's, every node's counter words equal the scan's."""
    name, K, m, P, D = row
    monkeypatch.setenv("PG_EMU_PLACES", str(places))
    want = G.golden_rows()[0][G.row_tag(row)]
    codes, lens, rec, last, _ = G.row_inputs(row, work)
    seq, dev, diff, rounds, cycles = G.tip_hook("host", rec, last, K, m, P, D, threads)
    assert seq == (want["single"], want["minor"])
    assert dev == seq
    assert diff == 0
    assert cycles == len(want["cycles"]) and rounds >= cycles


@pytest.mark.parametrize("places", [1, 3])
@pytest.mark.parametrize("row", ROOM_ROWS, ids=G.row_tag)
def test_device_tip_decisions_with_a_short_first_listing(row, places, work, monkeypatch, capfd):
    name, K, m, P, D = row
    monkeypatch.setenv("PG_EMU_PLACES", str(places))
    monkeypatch.setenv("PG_TIP_LIST_ROOM", "1")
    monkeypatch.setenv("PG_HOST_VERBOSE", "1")
    want = G.golden_rows()[0][G.row_tag(row)]
    codes, lens, rec, last, _ = G.row_inputs(row, work)
    seq, dev, diff, rounds, cycles = G.tip_hook("host", rec, last, K, m, P, D, 5)
    assert dev == seq == (want["single"], want["minor"])
    assert diff == 0
    assert "dead ends listed again" in capfd.readouterr().err


@pytest.mark.parametrize("name,K", sorted({(r[0], r[1]) for r in G.rows()}))
def test_reader_hands_over_the_designed_reads(name, K, tmp_path):
    """The design reaches the graph unchanged: the config and FASTQ of write_case, read as the command reads them, are exactly the designed reads."""
    reads = G.design(name, K)
    cfg = G.write_case(str(tmp_path), name, reads, K)
    codes, lens, n_records, mrl = api.host_read_all(cfg, K)
    assert n_records == len(reads) == len(lens) and mrl == G.max_rd_len(K)
    assert [int(x) for x in lens] == [len(x) for x in reads]
    assert all(np.array_equal(codes[i, :lens[i]], reads[i]) for i in range(len(reads)))


def test_the_designs_are_deterministic_and_scaled_with_K():
    for K in (31, 63, 127):
        for name in list(G.SINGLE_DESIGNS) + ["bush1"]:
            a, b = G.design(name, K), G.design(name, K)
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))
            assert all(K + 1 <= len(x) <= G.max_rd_len(K) for x in a)
        assert G.read_len(K) >= 2 * K + 40 and G.flank_len(K) >= 3 * K + 20
