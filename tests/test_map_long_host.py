"""The long-read pass (prlLongRead2Ctg, standardPregraph/prlRead2Ctg.c:1080) without a GPU: the host twin behind api.map_long_reads
against the independent model on reads built for the wave-per-read kernel's edges (tests/map_long_cases.py), and the command with
SOAPDENOVO2_AMD_MAP_HOST=1 SOAPDENOVO2_AMD_MAP_LONG=1 against the reference's md5s and stderr lines committed by
tests/golden/make_map_long_golden.py.  (A read has K + 1 bases or more to have k-mers, so "one k-mer" does not exist: the shortest reads
here have none and two.)"""
import base64
import os
import zlib

import pytest

import map_cases as M
import map_edge_cases as E
import map_long_cases as L
import map_model as MM

_HERE = os.path.dirname(os.path.abspath(__file__))
_GOLDEN, _SHORT = {}, {}
exec(compile(open(os.path.join(_HERE, "golden", "map_long_golden.py")).read(), "map_long_golden.py", "exec"), _GOLDEN)
exec(compile(open(os.path.join(_HERE, "golden", "map_golden.py")).read(), "map_golden.py", "exec"), _SHORT)
CASES, GRAPHS = _GOLDEN["CASES"], _SHORT["GRAPHS"]


def _graph(tmp_path, graph):
    d = tmp_path / "graph"
    d.mkdir()
    for ext, blob in GRAPHS[graph].items():
        (d / ("g." + ext)).write_bytes(zlib.decompress(base64.b64decode(blob)))
    return str(d / "g")


@pytest.mark.parametrize("cid", E.CASE_IDS, ids=E.case_id)
def test_linear_decision_is_the_models(cid):
    """decide_linear == map_model.decide on every read of every edge case (the random reads among them), at every ALIGNLEN of that
    suite: what pins the linear form before it is used alone."""
    case = E.build(*cid)
    (_, _, length, bal), rows = E.model_rows(*cid)
    for A in E.align_lens(case.K, case.longest):
        want = E.model_out(*cid, A)
        got = [L.decide_linear(row, len(rd), case.K, A, length, bal) for row, rd in zip(rows, case.reads)]
        E.assert_out_equal(got, want, case.tags, "decide_linear %s ALIGNLEN %d" % (E.case_id(cid), A))


def test_wave_ids_is_exported():
    from soapdenovo2_amd import api
    assert api.map_wave_ids() >= 64 and api.map_wave_ids(True) >= 64


@pytest.mark.parametrize("K,mer127", L.FLAVOURS)
def test_host_twin_matches_model(K, mer127):
    from soapdenovo2_amd import api
    C = api.map_wave_ids(mer127)
    big = (K, mer127) in L.BIG_IDS_FLAVOURS
    case, tables, rows = L.constructed(K, mer127, C, big)
    L.check_constructed(case, rows, L.model_out(case, tables, rows, 40), L.model_out(case, tables, rows, K + 1), C, big)
    for A in L.align_lens(K):
        want = L.model_out(case, tables, rows, A)
        got_rows, got = L.product(tables, case.reads, K, mer127, A, device=-1)
        E.assert_rows_equal(got_rows, rows, case.tags, "host k%d ALIGNLEN %d" % (K, A))
        E.assert_out_equal(got, want, case.tags, "host k%d ALIGNLEN %d" % (K, A))


def test_host_twin_ids_that_agree_in_their_low_bits():
    from soapdenovo2_amd import api
    K, mer127 = 31, False
    tables, reads, tags, rows = L.low_bits_case(K, mer127, api.map_wave_ids())
    want = [L.decide_linear(row, len(rd), K, K + 1, tables[2], tables[3]) for row, rd in zip(rows, reads)]
    assert sum(1 for w in want if w[0]) > len(want) // 2
    got_rows, got = L.product(tables, reads, K, mer127, K + 1, device=-1)
    E.assert_rows_equal(got_rows, rows, tags, "low bits host")
    E.assert_out_equal(got, want, tags, "low bits host")
    assert api.map_long_last_stats() == (0, 0)


def test_host_twin_batch_shapes():
    K, mer127 = 31, False
    from soapdenovo2_amd import api
    case, tables, _ = L.constructed(K, mer127, api.map_wave_ids(), False)
    index = MM.build_index(tables[0], tables[1], K)
    for shape, reads in L.batch_shapes(case).items():
        rows, want = MM.map_reads(index, reads, K, 40, tables[2], tables[3])
        got_rows, got = L.product(tables, reads, K, mer127, 40, device=-1)
        E.assert_rows_equal(got_rows, rows, [shape] * len(reads), shape)
        E.assert_out_equal(got, want, [shape] * len(reads), shape)
        from_reads = api.map_long_reads(tables[0], tables[1], tables[2], tables[3], reads, K, 40, mer127, device=-1)      # rows not asked for
        assert [(int(a), int(b), int(c), int(d)) for a, b, c, d in zip(*from_reads)] == want


def _run(tmp_path, name, extra_env=None):
    mer127, K, k, p, fill, _, _ = L.CASES[name]
    pre = _graph(tmp_path, CASES[name]["graph"])
    cfg, _ = L.write_case(str(tmp_path), name)
    env = dict(os.environ, SOAPDENOVO2_AMD_MAP_HOST="1", SOAPDENOVO2_AMD_MAP_LONG="1")
    env.update(extra_env or {})
    return M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, env)


@pytest.mark.parametrize("name", sorted(CASES))
def test_map_long_host_twin_matches_reference(tmp_path, name):
    want = CASES[name]
    rc, err, out_pre = _run(tmp_path, name)
    assert rc == 0, err[-2000:]
    assert L.long_digests(out_pre) == want["digests"]
    assert M.summary(err) == want["summary"]
    assert L.long_lines(err) == want["long_lines"]
    assert "Time spent on aligning long reads: " in err


def test_p_changes_the_long_file():
    a, b = L.P_PAIR
    assert CASES[a]["digests"]["longReadInGap"] != CASES[b]["digests"]["longReadInGap"]


def test_switch_without_long_library_changes_nothing(tmp_path):
    name = "k31_p3_f"
    mer127, K, k, p, fill, layout = M.CASES[name]
    want = _SHORT["CASES"][name]
    pre = _graph(tmp_path, want["graph"])
    cfg = M.write_libs(str(tmp_path), layout, k or K)
    env = dict(os.environ, SOAPDENOVO2_AMD_MAP_HOST="1", SOAPDENOVO2_AMD_MAP_LONG="1")
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, env)
    assert rc == 0, err[-2000:]
    got = L.long_digests(out_pre)
    assert got.pop("longReadInGap") is None and got.pop("RlongReadInGap") is None
    assert got == want["digests"] and M.summary(err) == want["summary"]
    assert not L.long_lines(err)


def test_refusal_names_the_switch(tmp_path):
    """Without the switch the refusal stands (tests/test_map_host.py pins it); its message names the switch."""
    name = "l31_p1"
    mer127, K, k, p, fill, _, _ = L.CASES[name]
    pre = _graph(tmp_path, CASES[name]["graph"])
    cfg, _ = L.write_case(str(tmp_path), name)
    env = dict(os.environ, SOAPDENOVO2_AMD_MAP_HOST="1")
    env.pop("SOAPDENOVO2_AMD_MAP_LONG", None)
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, env)
    assert rc != 0 and "asm_flags=4" in err and "SOAPDENOVO2_AMD_MAP_LONG=1" in err
    assert all(v is None for v in L.long_digests(out_pre).values())


def test_unknown_kernel_name_is_an_error(tmp_path):
    rc, err, out_pre = _run(tmp_path, "l31_p1", {"SOAPDENOVO2_AMD_MAP_LONG_KERNEL": "fast"})
    assert rc != 0 and "lane or wave" in err


def test_kernel_switch_is_read(tmp_path):
    """The pass names the kernel it was told to run in its verbose line: lane unless SOAPDENOVO2_AMD_MAP_LONG_KERNEL=wave."""
    for kernel, env in (("lane", {}), ("wave", {"SOAPDENOVO2_AMD_MAP_LONG_KERNEL": "wave"}), ("lane", {"SOAPDENOVO2_AMD_MAP_LONG_KERNEL": "lane"})):
        d = tmp_path / (kernel + str(len(env)))
        d.mkdir()
        rc, err, _ = _run(d, "l31_p1", dict(env, PG_HOST_VERBOSE="1"))
        assert rc == 0 and "[map long] %s kernel" % kernel in err, err[-800:]
