"""The contig k-mer index of `map` cut over ranks by key, without a GPU: the plan (pg_host_map_plan), the ownership function
(pg_host_map_owner: map_owner of csrc/map_index.hpp), the host twin of the cut (a device list of -1s: n serial tables, every rank's
lookups into a zeroed row of its own, the rows ORed, the one decision) against the single-table twin on every case of
tests/map_edge_cases.py, and the command's choice between one table and the cut (SOAPDENOVO2_AMD_MAP_SHARD, the plan, the budget hook)
with SOAPDENOVO2_AMD_MAP_HOST=1 against the reference's md5s.  tests/test_gpu_map_sharded.py runs the device engine."""
import base64
import functools
import os
import zlib

import numpy as np
import pytest

import map_cases as M
import map_edge_cases as E
import map_model as MM

_GOLDEN = {}
exec(compile(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_golden.py")).read(), "map_golden.py", "exec"), _GOLDEN)
CASES, GRAPHS = _GOLDEN["CASES"], _GOLDEN["GRAPHS"]

RANKS = (1, 2, 3, 8)
HUMAN_KMERS = 3 * 10**9
CARD = 288 * 10**9


# ---------------------------------------------------------------------------------------------------------
# the plan
# ---------------------------------------------------------------------------------------------------------
def test_plan_human_63mer_needs_more_than_one_rank():
    from soapdenovo2_amd import api
    one = api.map_plan(HUMAN_KMERS, False, 1, device_bytes=CARD)
    assert not one["fits"] and one["one_table"] == (1 << 33) * 32 and one["table"] >= one["one_table"]
    eight = api.map_plan(HUMAN_KMERS, False, 8, device_bytes=CARD)
    assert eight["fits"] and eight["table"] == eight["slots"] * 32 and eight["slots"] >= 2 * eight["keys"] > 2 * HUMAN_KMERS // 8
    assert eight["staging"] == eight["rows"] > 0 and eight["peak"] <= eight["budget"] == int(CARD * 0.85)
    assert 2 <= eight["fewest_ranks"] <= 8 and one["fewest_ranks"] == eight["fewest_ranks"]


def test_plan_human_127mer_fits_two_ranks():
    from soapdenovo2_amd import api
    one = api.map_plan(HUMAN_KMERS, True, 1, device_bytes=CARD)
    assert not one["fits"] and one["one_table"] == (1 << 33) * 48
    two = api.map_plan(HUMAN_KMERS, True, 2, device_bytes=CARD)
    assert two["fits"] and two["table"] == (1 << 32) * 48 and two["fewest_ranks"] == 2


def test_plan_small_genome_fits_one_rank():
    """configs[1]: 10 M reads of 100 bases over a 5 Mb genome; its contigs carry at most the genome's k-mers."""
    from soapdenovo2_amd import api
    p = api.map_plan(5 * 10**6, False, 1, device_bytes=CARD)
    assert p["fits"] and p["fewest_ranks"] == 1 and p["staging"] == 0
    assert p["table"] == MM.table_slots(5 * 10**6) * 32 * 5 // 4            # the single-device engine's block: a quarter of headroom


def test_plan_refuses_bad_arguments():
    from soapdenovo2_amd import api
    with pytest.raises(api.PgError):
        api.map_plan(1000, False, 0)
    with pytest.raises(api.PgError):
        api.map_plan(1000, False, 1, device_bytes=0)


# ---------------------------------------------------------------------------------------------------------
# ownership
# ---------------------------------------------------------------------------------------------------------
def _key_words(keys, nw):
    return np.array([[(k >> (64 * (nw - 1 - i))) & MM.M64 for i in range(nw)] for k in keys], dtype=np.uint64)


@pytest.mark.parametrize("mer127", [False, True])
@pytest.mark.parametrize("n", [3, 8])
def test_owner_shares_are_even(n, mer127):
    """10^6 random keys: a share is binomial with sigma = sqrt(p (1 - p) / 10^6) <= 0.05 % of all keys, i.e. ~0.3 % of a share of 1 / 8;
    2 % of 1 / n is more than six of those."""
    from soapdenovo2_amd import api
    nw = 4 if mer127 else 2
    rng = np.random.default_rng(40 + n)
    keys = rng.integers(0, 1 << 62, size=(10**6, nw), dtype=np.uint64)
    owner = api.map_owner(keys, n, mer127)
    assert owner.max() == n - 1
    share = np.bincount(owner, minlength=n) / len(keys)
    assert np.all(np.abs(share - 1.0 / n) <= 0.02 / n), share


@pytest.mark.parametrize("K,mer127", [(31, False), (63, False), (65, True), (127, True)])
def test_owner_is_a_function_of_the_key(K, mer127):
    """A key put from two contigs (the `index` case's d2 / d3 share a stretch, one of them on the other strand in d3 / d4) has one owner:
    the product's owner of every contig k-mer is the restated hash's bits 40 and up mod n, whichever contig brings it."""
    from soapdenovo2_amd import api
    nw = 4 if mer127 else 2
    ctgs = E.loaded(E.build("index", K, mer127))[0]
    per_contig = [[min(f, r) for f, r in MM.kmers(c, K)] for c in ctgs]
    seen, shared = {}, 0
    for n in (2, 3, 8):
        for ci, keys in enumerate(per_contig):
            owner = api.map_owner(_key_words(keys, nw), n, mer127)
            for k, o in zip(keys, owner):
                assert int(o) == (MM.map_home(k, nw, MM.M64) >> 40) % n
                if (k, n) in seen and seen[(k, n)][0] != ci:
                    shared += 1
                    assert seen[(k, n)][1] == int(o)
                seen[(k, n)] = (ci, int(o))
    assert shared >= 3 * 12              # (keys that do come from two contigs: two shared stretches of K + 5 bases, 6 k-mers each, for three n)


# ---------------------------------------------------------------------------------------------------------
# the host twin of the cut against the single-table twin
# ---------------------------------------------------------------------------------------------------------
def _align_len(cid):
    """One ALIGNLEN a case (the rows do not depend on it, and tests/test_map_edges.py runs the decision at all four on the single
    table): they rotate over the cases, so every value of the suite meets every kind of case."""
    case = E.build(*cid)
    lens = E.align_lens(case.K, case.longest)
    return lens[E.CASE_IDS.index(cid) % len(lens)]


@functools.lru_cache(maxsize=None)
def _single_table(cid):
    case = E.build(*cid)
    return E.product(cid, case.reads, _align_len(cid), -1)


@pytest.mark.parametrize("n", RANKS)
@pytest.mark.parametrize("cid", E.CASE_IDS, ids=E.case_id)
def test_sharded_host_twin_matches_single_table(cid, n):
    case = E.build(*cid)
    want_rows, want = _single_table(cid)
    got_rows, got = E.product(cid, case.reads, _align_len(cid), (-1,) * n)
    assert got_rows == want_rows, "hit rows, %d ranks" % n
    E.assert_out_equal(got, want, case.tags, "%s over %d host ranks" % (E.case_id(cid), n))
    if cid[0] not in ("empty", "allrc"):
        assert any(w for row in want_rows for w in row) and any(o[0] for o in want)


@pytest.mark.parametrize("K,mer127", [(31, False), (65, True)])
def test_sharded_host_twin_reads_and_long_reads_entry_points(K, mer127):
    from soapdenovo2_amd import api
    cid = ("decide", K, mer127)
    case = E.build(*cid)
    ctgs, ids, length, bal = E.model_rows(*cid)[0]
    one = api.map_reads(ctgs, ids, length, bal, case.reads, case.K, 32, mer127, device=-1)
    for got in (api.map_reads(ctgs, ids, length, bal, case.reads, case.K, 32, mer127, device=(-1, -1, -1)),
                api.map_long_reads(ctgs, ids, length, bal, case.reads, case.K, 32, mer127, device=[-1, -1])):
        for a, b in zip(got, one):
            assert np.array_equal(a, b)
    assert (one[0] > 0).sum() > 10


def test_device_list_must_be_all_host_or_all_gpus():
    from soapdenovo2_amd import api
    cid = ("load512", 31, False)
    case = E.build(*cid)
    ctgs, ids, length, bal = E.model_rows(*cid)[0]
    for bad in ((-1, 0), ()):
        with pytest.raises(api.PgError):
            api.map_reads(ctgs, ids, length, bal, case.reads, 31, 32, False, device=bad)


# ---------------------------------------------------------------------------------------------------------
# the command: which engine it takes (the host twin stands in for the device; tests/test_gpu_map_sharded.py runs the device's)
# ---------------------------------------------------------------------------------------------------------
def _graph(tmp_path, graph):
    d = tmp_path / "graph"
    d.mkdir()
    for ext, blob in GRAPHS[graph].items():
        (d / ("g." + ext)).write_bytes(zlib.decompress(base64.b64decode(blob)))
    return str(d / "g")


def _run(tmp_path, name, **env):
    mer127, K, k, p, fill, layout = M.CASES[name]
    pre = _graph(tmp_path, CASES[name]["graph"])
    cfg = M.write_libs(str(tmp_path), layout, k or K)
    full = dict(os.environ, SOAPDENOVO2_AMD_MAP_HOST="1", PG_HOST_VERBOSE="1")
    for v in ("SOAPDENOVO2_AMD_DEVICES", "SOAPDENOVO2_AMD_DEVICE", "SOAPDENOVO2_AMD_MAP_SHARD", "SOAPDENOVO2_AMD_MAP_BUDGET_MB"):
        full.pop(v, None)
    full.update(env)
    return M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, full)


def _sharded_line(err):
    return [ln for ln in err.splitlines() if ln.startswith("[map] index sharded over")]


@pytest.mark.parametrize("name", ["k31_p3_f", "m127_k75_p3_f"])
def test_command_sharded_by_the_switch(tmp_path, name):
    rc, err, out_pre = _run(tmp_path, name, SOAPDENOVO2_AMD_DEVICES="0,0,0", SOAPDENOVO2_AMD_MAP_SHARD="1")
    assert rc == 0, err[-2000:]
    assert M.digests(out_pre) == CASES[name]["digests"] and M.summary(err) == CASES[name]["summary"]
    line = _sharded_line(err)
    assert len(line) == 1 and "over 3 ranks" in line[0] and line[0].count(" / ") == 6, err[-800:]      # keys, load, probe: three each


def test_command_stays_on_one_table_without_the_switch(tmp_path):
    """A device list alone changes nothing, nor does the switch with one rank listed."""
    for i, env in enumerate(({"SOAPDENOVO2_AMD_DEVICES": "0,0,0"}, {"SOAPDENOVO2_AMD_DEVICES": "0", "SOAPDENOVO2_AMD_MAP_SHARD": "1"}, {})):
        d = tmp_path / str(i)
        d.mkdir()
        rc, err, out_pre = _run(d, "k31_p1", **env)
        assert rc == 0, err[-2000:]
        assert M.digests(out_pre) == CASES["k31_p1"]["digests"]
        assert not _sharded_line(err) and sum(ln.startswith("[map] ") for ln in err.splitlines()) == 1


def test_command_budget_hook_one_rank_is_refused_before_writing(tmp_path):
    rc, err, out_pre = _run(tmp_path, "k31_p3_f", SOAPDENOVO2_AMD_MAP_BUDGET_MB="1")
    assert rc != 0, err[-2000:]
    msg = [ln for ln in err.splitlines() if ln.startswith("map: the contig index does not fit")]
    assert len(msg) == 1 and "1 rank(s)" in msg[0] and "caps a rank's table at 1048576 bytes" in msg[0] and "ranks would hold it" in msg[0]
    assert "Nothing was written" in msg[0]
    assert all(v is None for v in M.digests(out_pre).values())


def test_command_budget_hook_three_ranks_shard_without_the_switch(tmp_path):
    rc, err, out_pre = _run(tmp_path, "k31_p3_f", SOAPDENOVO2_AMD_MAP_BUDGET_MB="1", SOAPDENOVO2_AMD_DEVICES="0,0,0")
    assert rc == 0, err[-2000:]
    assert M.digests(out_pre) == CASES["k31_p3_f"]["digests"] and M.summary(err) == CASES["k31_p3_f"]["summary"]
    assert len(_sharded_line(err)) == 1 and "over 3 ranks" in _sharded_line(err)[0]


def test_command_budget_hook_nothing_fits(tmp_path):
    rc, err, out_pre = _run(tmp_path, "k31_p3_f", SOAPDENOVO2_AMD_MAP_BUDGET_MB="0", SOAPDENOVO2_AMD_DEVICES="0,0,0")
    assert rc != 0 and "No number of ranks up to" in err and "3 rank(s)" in err
    assert all(v is None for v in M.digests(out_pre).values())
