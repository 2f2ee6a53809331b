"""The long-read pass on the device: the wave-per-read kernel (csrc/map_kernels.hip: map_read_wave_kernel) against the independent model
on the reads tests/map_long_cases.py builds for its edges -- every hit word and every (contig, position, orientation, footprint) --
against the lane-per-read kernel on the same inputs, run to run, and the command with SOAPDENOVO2_AMD_MAP_LONG=1 against the reference
binary (oracle/_ref) with both kernels.

The lane kernel answers a read with more than 8 ids by a scan that is quadratic in one lane, so it is asked only for the reads of up
to map_long_cases.LANE_MAX_KMERS k-mers, and for one read of C + 1 ids on its own; the other long ones (4 097 k-mers, the reads of up to
2C + 3 contigs) are held against the model."""
import base64
import os
import zlib

import pytest

import map_cases as M
import map_edge_cases as E
import map_long_cases as L
import map_model as MM

pytestmark = pytest.mark.gpu

_SHORT = {}
exec(compile(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_golden.py")).read(), "map_golden.py", "exec"), _SHORT)


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """As tests/test_gpu_map_edges.py: every call makes and destroys an engine, so the module pins the device arena."""
    from soapdenovo2_amd import api
    with api.arena_pinned(0):
        yield


def _constructed(K, mer127):
    from soapdenovo2_amd import api
    C = api.map_wave_ids(mer127)
    big = (K, mer127) in L.BIG_IDS_FLAVOURS
    return L.constructed(K, mer127, C, big)


@pytest.mark.parametrize("K,mer127", L.FLAVOURS)
def test_wave_kernel_matches_model(K, mer127):
    case, tables, rows = _constructed(K, mer127)
    for A in L.align_lens(K):
        want = L.model_out(case, tables, rows, A)
        got_rows, got = L.product(tables, case.reads, K, mer127, A, device=0)
        E.assert_rows_equal(got_rows, rows, case.tags, "wave k%d ALIGNLEN %d" % (K, A))
        E.assert_out_equal(got, want, case.tags, "wave k%d ALIGNLEN %d" % (K, A))


@pytest.mark.parametrize("K,mer127", L.FLAVOURS)
def test_wave_kernel_matches_lane_kernel(K, mer127):
    case, tables, _ = _constructed(K, mer127)
    keep = [r for r, rd in enumerate(case.reads) if len(rd) - K + 1 <= L.LANE_MAX_KMERS]
    reads = [case.reads[r] for r in keep]
    assert len(reads) >= 30 and max(len(rd) for rd in reads) - K + 1 >= 1000
    for A in (40, K + 1):
        wave = L.product(tables, reads, K, mer127, A, device=0)
        lane = L.product(tables, reads, K, mer127, A, device=0, lane=True)
        assert wave[0] == lane[0], "hit rows"
        E.assert_out_equal(wave[1], lane[1], [case.tags[r] for r in keep], "wave against lane k%d ALIGNLEN %d" % (K, A))


@pytest.mark.parametrize("K,mer127", L.BIG_IDS_FLAVOURS)
def test_reads_past_the_table_are_answered_in_passes(K, mer127):
    """One read a call, so that the kernel's own count of reads answered in passes (api.map_long_last_stats) speaks of that read: C - 1
    ids fit the table, C + 1 and 2C + 3 cannot.  The C + 1 read is the one whose winner is brought to the table last, so a table that
    stopped at C ids would answer it wrongly; the distinct ids the kernel counted are the model's."""
    from soapdenovo2_amd import api
    C = api.map_wave_ids(mer127)
    case, tables, rows = _constructed(K, mer127)
    want = L.model_out(case, tables, rows, K + 1)
    for m, passes in ((C - 1, 0), (C + 1, 1), (2 * C + 3, 1)):
        for kind in ("last-inserted-wins", "tied"):
            r = case.tags.index("ids%d-%s" % (m, kind))
            got_rows, got = L.product(tables, [case.reads[r]], K, mer127, K + 1, device=0)
            assert api.map_long_last_stats() == (passes, m), (m, kind)
            E.assert_rows_equal(got_rows, [rows[r]], [case.tags[r]], "alone")
            E.assert_out_equal(got, [want[r]], [case.tags[r]], "alone")


def test_ids_that_agree_in_their_low_bits_end_in_the_scan():
    """Every id a multiple of 64: no split by id % P separates them, and the reads of more than C ids are answered by the wave-wide
    scan.  Answers as the model's, and as the lane kernel's on the C + 1 read."""
    from soapdenovo2_amd import api
    K, mer127 = 31, False
    C = api.map_wave_ids()
    tables, reads, tags, rows = L.low_bits_case(K, mer127, C)
    want = [L.decide_linear(row, len(rd), K, K + 1, tables[2], tables[3]) for row, rd in zip(rows, reads)]
    got_rows, got = L.product(tables, reads, K, mer127, K + 1, device=0)
    E.assert_rows_equal(got_rows, rows, tags, "low bits")
    E.assert_out_equal(got, want, tags, "low bits")
    assert api.map_long_last_stats()[0] == sum(1 for row in rows if L.distinct_ids(row) > C) >= 8
    assert api.map_long_last_stats()[1] == sum(L.distinct_ids(row) for row in rows)


def test_wave_kernel_matches_lane_kernel_on_a_many_id_read():
    """The lane kernel's quadratic scan on one read of C + 1 ids (a few thousand k-mers: seconds in one lane), against the wave
    kernel's passes: the same row and the same tuple."""
    from soapdenovo2_amd import api
    K, mer127 = 31, False
    C = api.map_wave_ids()
    case, tables, rows = _constructed(K, mer127)
    r = case.tags.index("ids%d-last-inserted-wins" % (C + 1))
    wave = L.product(tables, [case.reads[r]], K, mer127, K + 1, device=0)
    assert api.map_long_last_stats()[0] == 1
    lane = L.product(tables, [case.reads[r]], K, mer127, K + 1, device=0, lane=True)
    assert wave == lane and wave[1][0][0]


@pytest.mark.parametrize("K,mer127", [(31, False), (75, True)])
def test_wave_kernel_three_runs(K, mer127):
    case, tables, _ = _constructed(K, mer127)
    first = L.product(tables, case.reads, K, mer127, K + 1, device=0)
    for run in range(2):
        assert L.product(tables, case.reads, K, mer127, K + 1, device=0) == first, "run %d" % (run + 2)


@pytest.mark.parametrize("K,mer127", [(31, False), (75, True)])
def test_wave_kernel_batch_shapes(K, mer127):
    from soapdenovo2_amd import api
    case, tables, _ = L.constructed(K, mer127, api.map_wave_ids(mer127), False)
    index = MM.build_index(tables[0], tables[1], K)
    for shape, reads in L.batch_shapes(case).items():
        rows, want = MM.map_reads(index, reads, K, 40, tables[2], tables[3])
        got_rows, got = L.product(tables, reads, K, mer127, 40, device=0)
        E.assert_rows_equal(got_rows, rows, [shape] * len(reads), shape)
        E.assert_out_equal(got, want, [shape] * len(reads), shape)
        plain = api.map_long_reads(tables[0], tables[1], tables[2], tables[3], reads, K, 40, mer127, device=0)
        assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*plain)] == want


def _graph(tmp_path, graph):
    d = tmp_path / "graph"
    d.mkdir()
    for ext, blob in _SHORT["GRAPHS"][graph].items():
        (d / ("g." + ext)).write_bytes(zlib.decompress(base64.b64decode(blob)))
    return str(d / "g")


@pytest.mark.parametrize("name", list(L.CASES))
def test_map_long_matches_reference(tmp_path, name):
    """Both executables' `map` on copies of one prefix (the contigs are tests/golden/map_golden.py's): the two long files byte for byte,
    the short pass's files as tests/test_gpu_map.py compares them, the summaries, and the same files again from the lane kernel."""
    mer127, K, k, p, fill, _, _ = L.CASES[name]
    if not os.path.exists(M.binary(mer127, False)):
        pytest.skip("the reference binaries under oracle/_ref are built by __graft_entry__.build() where the reference sources are")
    pre = _graph(tmp_path, "%s_k%d" % ("m127" if mer127 else "m63", K))
    cfg, _ = L.write_case(str(tmp_path), name)
    rr, ref_err, ref_pre = M.run_map(M.binary(mer127, False), cfg, pre, str(tmp_path / "ref"), k, p, fill)
    assert rr == 0, ref_err[-2000:]
    want = L.long_digests(ref_pre)
    assert want["longReadInGap"] and (want["RlongReadInGap"] is not None) == fill
    for kernel in ("wave", "lane"):
        env = dict(os.environ, SOAPDENOVO2_AMD_MAP_LONG="1", SOAPDENOVO2_AMD_MAP_LONG_KERNEL=kernel, PG_HOST_VERBOSE="1")
        env.pop("SOAPDENOVO2_AMD_MAP_HOST", None)
        ro, our_err, our_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / ("ours_" + kernel)), k, p, fill, env)
        assert ro == 0, our_err[-2000:]
        assert "[map long] %s kernel" % kernel in our_err
        for ext in L.LONG_OUTPUTS:
            ours, ref = our_pre + "." + ext, ref_pre + "." + ext
            assert os.path.exists(ours) == os.path.exists(ref)
            if os.path.exists(ref):
                assert open(ours, "rb").read() == open(ref, "rb").read(), (kernel, ext)
        assert L.long_digests(our_pre) == want, kernel
        assert M.summary(our_err) == M.summary(ref_err) and M.summary(ref_err)
        assert L.long_lines(our_err) == L.long_lines(ref_err) and len(L.long_lines(ref_err)) >= 4
