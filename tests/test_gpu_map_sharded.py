"""The contig k-mer index of `map` cut over ranks on the device (csrc/map_kernels.hip: ShardedDeviceMapEngine; map_count_owned_kernel,
map_index_owned_kernel, map_probe_owned_kernel, map_rows_merge_kernel, map_decide_rows_kernel, map_decide_rows_wave_kernel), every rank
on GPU 0: against the independent model on the cases of tests/map_edge_cases.py -- every hit word of the merged rows and every
(contig, position, orientation, footprint) -- over one, two, three and eight ranks; the cut's own edges (ranks that own nothing, a key put
from two contigs, empty and k-mer-less batches, the wave decision on both sides of pg_map_wave_ids, the index as a function of the contig
set); and the command with SOAPDENOVO2_AMD_DEVICES=0,0,0 against the reference's md5s (tests/golden/map_golden.py, map_long_golden.py).
tests/test_map_sharded_host.py holds the plan, the ownership function and the host twin of the cut."""
import base64
import os
import zlib

import numpy as np
import pytest

import map_cases as M
import map_edge_cases as E
import map_long_cases as L
import map_model as MM

pytestmark = pytest.mark.gpu

_HERE = os.path.dirname(os.path.abspath(__file__))
_SHORT, _LONG = {}, {}
exec(compile(open(os.path.join(_HERE, "golden", "map_golden.py")).read(), "map_golden.py", "exec"), _SHORT)
exec(compile(open(os.path.join(_HERE, "golden", "map_long_golden.py")).read(), "map_long_golden.py", "exec"), _LONG)

RANK_LISTS = [(0,), (0, 0), (0, 0, 0), (0,) * 8]


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """As tests/test_gpu_map_edges.py: every call makes and destroys an engine, so the module pins the device arena."""
    from soapdenovo2_amd import api
    with api.arena_pinned(0):
        yield


def _align_len(cid):
    """One ALIGNLEN a case, rotating over the suite's four (tests/test_gpu_map_edges.py runs the decision code at all four; the rows,
    which are what the cut changes, do not depend on it)."""
    case = E.build(*cid)
    lens = E.align_lens(case.K, case.longest)
    return lens[E.CASE_IDS.index(cid) % len(lens)]


@pytest.mark.parametrize("devices", RANK_LISTS, ids=lambda d: "ranks%d" % len(d))
@pytest.mark.parametrize("cid", E.CASE_IDS, ids=E.case_id)
def test_sharded_device_matches_model(cid, devices):
    case = E.build(*cid)
    _, rows = E.model_rows(*cid)
    A = _align_len(cid)
    want = E.model_out(*cid, A)
    E.check_not_vacuous(case, A, want, rows)
    what = "%s ALIGNLEN %d over %d ranks" % (E.case_id(cid), A, len(devices))
    got_rows, got = E.product(cid, case.reads, A, devices)
    E.assert_rows_equal(got_rows, rows, case.tags, what)
    E.assert_out_equal(got, want, case.tags, what)


@pytest.mark.parametrize("K,mer127", [(31, False), (65, True)])
def test_most_ranks_own_nothing(K, mer127):
    """One contig of K + 2 bases: three k-mers over eight ranks, so five ranks or more keep an empty table and launch no build."""
    rng = np.random.default_rng(K)
    ctg = rng.integers(0, 4, size=K + 2, dtype=np.uint8)
    ids = np.array([1], dtype=np.uint32)
    length, bal = E.id_tables([(K + 2, 1)])
    reads = [ctg, E.rc(ctg), ctg[:K + 1], ctg[1:], rng.integers(0, 4, size=K + 9, dtype=np.uint8), ctg[:K]]
    index = MM.build_index([ctg], ids, K)
    rows, want = MM.map_reads(index, reads, K, K + 1, length, bal)
    assert sum(h is not None for row in rows for h in row) == 10 and want[0][0] and want[1][0] and not want[4][0]
    from soapdenovo2_amd import api
    for devices in ((0,) * 8, (0,) * 5):
        got = api.map_hits([ctg], ids, length, bal, reads, K, K + 1, mer127, device=devices)
        koff = got[5]
        got_rows = [[int(w) for w in got[4][int(koff[r]):int(koff[r + 1])]] for r in range(len(reads))]
        E.assert_rows_equal(got_rows, rows, ["r%d" % r for r in range(len(reads))], "three k-mers over %d ranks" % len(devices))
        E.assert_out_equal([(int(got[0][r]), int(got[1][r]), int(got[2][r]), int(got[3][r])) for r in range(len(reads))], want,
                           ["r%d" % r for r in range(len(reads))], "three k-mers")


@pytest.mark.parametrize("devices", RANK_LISTS[1:], ids=lambda d: "ranks%d" % len(d))
def test_key_put_from_two_contigs_reads_as_deleted(devices):
    K = 31
    rng = np.random.default_rng(5)
    shared = rng.integers(0, 4, size=K + 9, dtype=np.uint8)                      # 10 keys, put by both contigs, one on the other strand
    la, ra, lb, rb = (rng.integers(0, 4, size=n, dtype=np.uint8) for n in (50, 50, 40, 60))
    la[-1] = ((rb[0] ^ 2) + 1) & 3                   # the bases next to the stretch differ between the contigs (b seen from a's strand is
    ra[0] = ((lb[-1] ^ 2) + 1) & 3                   # rc(rb) + shared + rc(lb)), so the two share exactly the stretch's 10 keys
    a = E.cat(la, shared, ra)
    b = E.cat(lb, E.rc(shared), rb)
    ids = np.array([1, 3], dtype=np.uint32)
    length, bal = E.id_tables([(len(a), 1), (len(b), 1)])
    from soapdenovo2_amd import api
    got = api.map_hits([a, b], ids, length, bal, [shared, a, b], K, 32, False, device=devices)
    koff = [int(x) for x in got[5]]
    assert not got[4][koff[0]:koff[1]].any() and got[0][0] == 0                  # the shared stretch alone: every key deleted
    rows, want = MM.map_reads(MM.build_index([a, b], ids, K), [shared, a, b], K, 32, length, bal)
    assert [int(w) for w in got[4]] == [MM.hit_word(h) for row in rows for h in row]
    assert sum(h is None for h in rows[1]) == 10 and got[0][1] == 1 and got[0][2] == 3


@pytest.mark.parametrize("K,mer127", [(31, False), (65, True)])
def test_batch_shapes(K, mer127):
    """An empty batch, batches whose reads have no k-mers, block edges: over three ranks."""
    E.compare_shapes(K, mer127, device=(0, 0, 0))


@pytest.mark.parametrize("K,mer127", L.BIG_IDS_FLAVOURS)
def test_wave_decision_on_both_sides_of_the_table(K, mer127):
    """The long-read entry point over three ranks: the lookups a wavefront a read, the decision by the wave kernel's decision half from
    the merged rows, on reads of C - 1 ... 2C + 3 ids (C = pg_map_wave_ids); the kernel's own count of reads answered in passes says that
    both sides were met."""
    from soapdenovo2_amd import api
    C = api.map_wave_ids(mer127)
    case, tables, rows = L.constructed(K, mer127, C, True)
    A = K + 1
    want = L.model_out(case, tables, rows, A)
    got_rows, got = L.product(tables, case.reads, K, mer127, A, device=(0, 0, 0))
    E.assert_rows_equal(got_rows, rows, case.tags, "wave over three ranks")
    E.assert_out_equal(got, want, case.tags, "wave over three ranks")
    n_over = sum(1 for row in rows if L.distinct_ids(row) > C)
    n_under = sum(1 for row in rows if 1 < L.distinct_ids(row) < C)
    passes, ids = api.map_long_last_stats()
    assert n_over >= 4 and n_under >= 4 and passes >= n_over and ids == sum(L.distinct_ids(row) for row in rows)
    plain = api.map_long_reads(tables[0], tables[1], tables[2], tables[3], case.reads[:5], K, A, mer127, device=(0, 0))
    assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*plain)] == want[:5]


@pytest.mark.parametrize("K,mer127", [(31, False), (65, True)])
def test_index_is_a_function_of_the_contig_set(K, mer127):
    from soapdenovo2_amd import api
    cid = ("index", K, mer127)
    case = E.build(*cid)
    (ctgs, ids, length, bal), rows = E.model_rows(*cid)
    want = np.array([MM.hit_word(h) for row in rows for h in row], dtype=np.uint64)
    rng = np.random.default_rng(K)
    orders = [list(range(len(ctgs)))[::-1], list(rng.permutation(len(ctgs)))]
    for order in orders:
        for run in range(3):
            got = api.map_hits([ctgs[i] for i in order], ids[order], length, bal, case.reads, K, 32, mer127, device=(0, 0, 0))
            assert np.array_equal(got[4], want), "order %r run %d" % (order, run)


def test_reads_entry_point_and_bad_lists():
    from soapdenovo2_amd import api
    cid = ("decide", 31, False)
    case = E.build(*cid)
    ctgs, ids, length, bal = E.model_rows(*cid)[0]
    want = E.model_out(*cid, 32)
    got = api.map_reads(ctgs, ids, length, bal, case.reads, 31, 32, False, device=(0, 0))
    assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*got)] == want
    for bad in ((0, -1), (0, 1 << 20)):
        with pytest.raises(api.PgError):
            api.map_reads(ctgs, ids, length, bal, case.reads, 31, 32, False, device=bad)


# ---------------------------------------------------------------------------------------------------------
# the command
# ---------------------------------------------------------------------------------------------------------
def _graph(tmp_path, graph):
    d = tmp_path / "graph"
    d.mkdir()
    for ext, blob in _SHORT["GRAPHS"][graph].items():
        (d / ("g." + ext)).write_bytes(zlib.decompress(base64.b64decode(blob)))
    return str(d / "g")


def _env(**more):
    env = dict(os.environ, PG_HOST_VERBOSE="1")
    for v in ("SOAPDENOVO2_AMD_MAP_HOST", "SOAPDENOVO2_AMD_DEVICE", "SOAPDENOVO2_AMD_DEVICES", "SOAPDENOVO2_AMD_MAP_SHARD",
              "SOAPDENOVO2_AMD_MAP_BUDGET_MB", "SOAPDENOVO2_AMD_MAP_LONG", "SOAPDENOVO2_AMD_MAP_LONG_KERNEL"):
        env.pop(v, None)
    env.update(more)
    return env


def _sharded_line(err):
    return [ln for ln in err.splitlines() if ln.startswith("[map] index sharded over")]


@pytest.mark.parametrize("name", ["k63_p3_f", "m127_k75_p3_f", "k31_batches"])
def test_command_over_three_ranks_matches_reference_md5s(tmp_path, name):
    """The graph built as tests/test_gpu_map.py builds it (the reference's pregraph + contig), `map` with the index over three ranks,
    the files against the md5s the reference's `map` left in tests/golden/map_golden.py."""
    mer127 = M.CASES[name][0]
    if not os.path.exists(M.binary(mer127, False)):
        pytest.skip("the reference binaries under oracle/_ref are built by __graft_entry__.build() where the reference sources are")
    cfg, pre, (_, K, k, p, fill, _) = M.build_case(str(tmp_path), name)
    env = _env(SOAPDENOVO2_AMD_DEVICES="0,0,0", SOAPDENOVO2_AMD_MAP_SHARD="1")
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, env)
    assert rc == 0, err[-2000:]
    assert M.digests(out_pre) == _SHORT["CASES"][name]["digests"]
    assert M.summary(err) == _SHORT["CASES"][name]["summary"]
    assert len(_sharded_line(err)) == 1 and "over 3 ranks" in _sharded_line(err)[0], err[-800:]


@pytest.mark.parametrize("kernel", ["lane", "wave"])
def test_command_long_read_pass_over_three_ranks(tmp_path, kernel):
    name = "l31_p3_f"
    mer127, K, k, p, fill, _, _ = L.CASES[name]
    want = _LONG["CASES"][name]
    pre = _graph(tmp_path, want["graph"])
    cfg, _ = L.write_case(str(tmp_path), name)
    env = _env(SOAPDENOVO2_AMD_DEVICES="0,0,0", SOAPDENOVO2_AMD_MAP_SHARD="1", SOAPDENOVO2_AMD_MAP_LONG="1",
               SOAPDENOVO2_AMD_MAP_LONG_KERNEL=kernel)
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, env)
    assert rc == 0, err[-2000:]
    assert L.long_digests(out_pre) == want["digests"]
    assert M.summary(err) == want["summary"] and L.long_lines(err) == want["long_lines"]
    assert "[map long] %s kernel" % kernel in err and len(_sharded_line(err)) == 1


def test_budget_hook_one_device_is_refused_before_writing(tmp_path):
    name = "k31_p3_f"
    mer127, K, k, p, fill, layout = M.CASES[name]
    pre = _graph(tmp_path, _SHORT["CASES"][name]["graph"])
    cfg = M.write_libs(str(tmp_path), layout, k or K)
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill,
                                 _env(SOAPDENOVO2_AMD_MAP_BUDGET_MB="1", SOAPDENOVO2_AMD_DEVICES="0"))
    assert rc != 0
    msg = [ln for ln in err.splitlines() if ln.startswith("map: the contig index does not fit")]
    assert len(msg) == 1 and "bytes as one table" in msg[0] and "caps a rank's table at 1048576 bytes" in msg[0]
    assert "ranks would hold it" in msg[0] and "Nothing was written" in msg[0]
    assert all(v is None for v in M.digests(out_pre).values())


def test_budget_hook_three_ranks_shard_without_the_switch(tmp_path):
    name = "k31_p3_f"
    mer127, K, k, p, fill, layout = M.CASES[name]
    pre = _graph(tmp_path, _SHORT["CASES"][name]["graph"])
    cfg = M.write_libs(str(tmp_path), layout, k or K)
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill,
                                 _env(SOAPDENOVO2_AMD_MAP_BUDGET_MB="1", SOAPDENOVO2_AMD_DEVICES="0,0,0"))
    assert rc == 0, err[-2000:]
    assert M.digests(out_pre) == _SHORT["CASES"][name]["digests"] and M.summary(err) == _SHORT["CASES"][name]["summary"]
    assert len(_sharded_line(err)) == 1 and "over 3 ranks" in _sharded_line(err)[0]


def test_single_rank_run_keeps_its_report(tmp_path):
    """Without the switch and the hook a device list changes nothing: one [map] line, the parent's shape, the same files."""
    name = "k31_p1"
    mer127, K, k, p, fill, layout = M.CASES[name]
    pre = _graph(tmp_path, _SHORT["CASES"][name]["graph"])
    cfg = M.write_libs(str(tmp_path), layout, k or K)
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, _env(SOAPDENOVO2_AMD_DEVICES="0,0,0"))
    assert rc == 0, err[-2000:]
    assert M.digests(out_pre) == _SHORT["CASES"][name]["digests"]
    lines = [ln for ln in err.splitlines() if ln.startswith("[map] ")]
    assert len(lines) == 1 and lines[0].startswith("[map] contigs ") and "index " in lines[0] and lines[0].rstrip().endswith("s")
    assert "whole stage" in lines[0] and not _sharded_line(err)
