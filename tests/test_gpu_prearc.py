"""Pass 2's hash tables under load (run with -m gpu on an MI355X).

The designed cases of tests/prearc_cases.py go through pg_device_emu_prearcs -- the product's add_prearc, p2_arc_init, p2_count_arcs, p2_compact_arcs and
p2_fold_arcs on caller-given triples -- and must equal tests/prearc_model.py exactly, in order and in count (tests/test_prearc_cases_host.py holds the
cases and the model to their claims without a GPU).  Then the real pass 2 runs on crowded tables: PG_P2_ARC_ROOM makes every lane's pre-arc table the
smallest power of two that holds the case's pairs (a load above one half), PG_EB_PATCH_ROOM=2 lets the (K+1)-mer table's growth rule pick its size (25 - 50 %),
and the files must stay the reference's.  Every comparison is exact."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN, case_codes, case_config, case_tag, md5_file, md5_gz_text, oracle_records
from soapdenovo2_amd import api
import prearc_cases as cases
import prearc_model as model
from test_gpu_pregraph import PARALLEL_PARSE, _run_cli

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """(every pg_device_emu_* call allocates its blocks and frees them all: tests/test_gpu_dev_graph.py)"""
    with api.arena_pinned(0):
        yield


def _device_rows(c):
    return api.device_emu_prearcs(c.frm, c.to, c.seq, c.room, c.lanes, device=0)


# ---- the designed cases ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [n for n in cases.SMALL if n not in cases.OVER])
def test_prearc_emu_case_equals_the_model(name):
    """one_home: whole waves claim one entry with different pairs; wraps: probe runs that go on at entry 0 (and a table of two entries); full: every
    entry taken and no overflow; hot: a multiplicity above 2^16 with its earliest meeting mid-input; first_bits: first meetings that differ in one
    range of bits only, up to the largest; ids: edge ids up to 0xFFFFFFFE, mirrored pairs, one source with 500 targets; lanes: 2, 3 and 8 tables
    merged.  The mistake each would catch is the case's `mistake`."""
    c = cases.small(name)
    want = model.as_rows(model.fold(c.triples()))
    got = _device_rows(c)
    assert got.shape == want.shape, (name, c.mistake)
    assert np.array_equal(got, want), (name, c.mistake, np.flatnonzero((got != want).any(axis=1))[:5])


@pytest.mark.parametrize("name", cases.OVER)
def test_prearc_emu_overflow_is_counted_exactly(name):
    """room + d pairs, each met once: exactly d triples find their table full (each after one pass over all of it), and nothing is folded."""
    c = cases.small(name)
    with pytest.raises(api.PgError, match="pre-arc table overflow") as e:
        _device_rows(c)
    assert e.value.overflow == c.overflow


@pytest.mark.parametrize("which", ["count", "fold"])
def test_prearc_emu_second_trip(which):
    """600 000 pairs in 2^20 entries: p2_count_arcs and p2_compact_arcs (2048 x 256 lanes) go round their loops twice; 2 200 000 pairs in 2^22 entries:
    so does every pf_* kernel of the fold (8192 x 256 lanes)."""
    c = cases.second_trip(which)
    want = model.fold_np(c.frm, c.to, c.seq)
    got = _device_rows(c)
    assert got.shape == want.shape
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1))[:5]


def test_prearc_emu_refuses_bad_arguments():
    one = np.ones(1, dtype=np.uint32)
    for room, lanes in ((0, 1), (1, 1), (3, 1), (255, 1), (256, 0)):
        with pytest.raises(api.PgError, match="bad argument"):
            api.device_emu_prearcs(one, one, one.astype(np.uint64), room, lanes)
    with pytest.raises(api.PgError, match="empty key"):
        api.device_emu_prearcs(0 * one, 0 * one, one.astype(np.uint64), 2, 1)
    assert api.device_emu_prearcs(one[:0], one[:0], one[:0].astype(np.uint64), 2, 1).shape == (0, 3)


# ---- the real pass 2 on crowded tables ------------------------------------------------------------------------------------------------------------
FILES = ("preArc", "vertex", "preGraphBasic", "edge.gz", "path", "markOnEdge")


def _pow2_at_least(n):
    return 1 << max(1, (n - 1).bit_length())


def _pairs_of(path):
    return sum(len(t) for _, t in model.parse_prearc(open(path).read()))


def _len1_edges(pre):
    return gzip.open(pre + ".edge.gz", "rt").read().count(">length 1,")


def _golden_case(golden, tmp_path, name, P):
    """(the arguments of host_pregraph_files, the pinned digests) of a golden case's -p P run"""
    c = golden["cases"][name]
    run = [r for r in c["runs"] if r[0] == P and r[1] == 0 and r[2] == 0][0]
    t = case_tag(name, run)
    codes = case_codes(c)
    rec, last, K = oracle_records(codes, c["K"], P, mer127=bool(run[3]), prefix=str(tmp_path / ("o_" + t)))
    want = {e: golden["md5"][t][e] for e in ("preArc", "vertex", "preGraphBasic", "edge", "path", "markOnEdge")}
    return (rec, last, codes, None, K, P), dict(mer127=bool(run[3]), max_read_len=c["L"]), want


def _pass2(args, kw, pre):
    rec, last, codes, lens, K, P = args
    return api.host_pregraph_files(rec, last, codes, lens, K, P, pre, device=0, packed=True, device_edges=True, resolve_repeats=True, batches=2, **kw)


def _digests(pre):
    return {"preArc": md5_file(pre + ".preArc"), "vertex": md5_file(pre + ".vertex"), "preGraphBasic": md5_file(pre + ".preGraphBasic"),
            "edge": md5_gz_text(pre + ".edge.gz"), "path": md5_file(pre + ".path"), "markOnEdge": md5_file(pre + ".markOnEdge")}


def _same_files(a, b):
    for ext in FILES:
        if ext == "edge.gz":
            assert gzip.open(a + ".edge.gz", "rb").read() == gzip.open(b + ".edge.gz", "rb").read(), ext
        else:
            assert open(a + "." + ext, "rb").read() == open(b + "." + ext, "rb").read(), ext


def _unhook(monkeypatch):
    for name in ("PG_P2_ARC_ROOM", "PG_EB_PATCH_ROOM"):
        monkeypatch.delenv(name, raising=False)


@pytest.mark.parametrize("name,P", [("t6k_k31", 8), ("d8k_k127", 3), ("t8k_k63", 2)])
def test_pass2_on_crowded_tables_writes_the_same_files(golden, tmp_path, monkeypatch, name, P):
    """In process, device edges and device pass 2 with -R: first unhooked against the pinned digests, then with every lane's pre-arc table the smallest power
    of two that holds the pairs of the .preArc just written (a load above one half, asserted from the file) and the (K+1)-mer table sized by its growth
    rule from 2 entries (the case has 8 length-1 edges or more, asserted from the edge text): the same bytes.  (t6k_k127 -p 3 has no length-1 edge and
    the `all` design of tests/graph_designs.py five at the most: the 127-mer flavour runs on d8k_k127, 27 of them, and t8k_k63 has 18.)"""
    args, kw, want = _golden_case(golden, tmp_path, name, P)
    _unhook(monkeypatch)
    first = str(tmp_path / "plain")
    _pass2(args, kw, first)
    assert _digests(first) == want
    A = _pairs_of(first + ".preArc")
    room = _pow2_at_least(A)
    assert room >= 2 and A / room > 0.5 and A <= room
    assert _len1_edges(first) >= 8
    monkeypatch.setenv("PG_P2_ARC_ROOM", str(room))
    monkeypatch.setenv("PG_EB_PATCH_ROOM", "2")
    second = str(tmp_path / "crowded")
    _pass2(args, kw, second)
    _same_files(first, second)
    assert _digests(second) == want


def test_pass2_hook_sizes_must_be_powers_of_two(golden, tmp_path, monkeypatch):
    args, kw, want = _golden_case(golden, tmp_path, "t6k_k31", 8)
    _unhook(monkeypatch)
    monkeypatch.setenv("PG_P2_ARC_ROOM", "6000")
    with pytest.raises(api.PgError, match="pre-arc table size must be a power of two"):
        _pass2(args, kw, str(tmp_path / "a"))
    monkeypatch.delenv("PG_P2_ARC_ROOM")
    monkeypatch.setenv("PG_EB_PATCH_ROOM", "3")
    with pytest.raises(api.PgError, match="patch table size must be a power of two"):
        _pass2(args, kw, str(tmp_path / "b"))
    monkeypatch.delenv("PG_EB_PATCH_ROOM")
    _pass2(args, kw, str(tmp_path / "c"))
    assert _digests(str(tmp_path / "c")) == want


def test_pass2_prearc_table_overflow_is_an_error_the_process_survives(golden, tmp_path, monkeypatch):
    """A table of at most half as many entries as the case has pairs: pass 2 ends with `pre-arc table overflow` (a full table costs an insertion one pass over
    it, 2048 entries here), and the run after it, unhooked, writes the pinned files again."""
    args, kw, want = _golden_case(golden, tmp_path, "t6k_k31", 8)
    A = _pairs_of(os.path.join(GOLDEN, "t6k_k31_p8_d0_a0_63.preArc"))
    assert md5_file(os.path.join(GOLDEN, "t6k_k31_p8_d0_a0_63.preArc")) == want["preArc"]
    room = _pow2_at_least(A // 2 + 1)
    room = room if room <= A // 2 else room // 2                        # the largest power of two <= A / 2
    assert 2 <= room <= A / 2 < 2 * room
    _unhook(monkeypatch)
    monkeypatch.setenv("PG_P2_ARC_ROOM", str(room))
    with pytest.raises(api.PgError, match="pre-arc table overflow"):
        _pass2(args, kw, str(tmp_path / "over"))
    monkeypatch.delenv("PG_P2_ARC_ROOM")
    again = str(tmp_path / "again")
    _pass2(args, kw, again)
    assert _digests(again) == want


@pytest.mark.parametrize("form", ["one-rank", "three-ranks-routed", "three-ranks-peer-probes"])
def test_cli_on_crowded_tables_matches_reference_files(golden, tmp_path, form):
    """The command on t6k_k31 -p 8 -R with both hooks: one rank; three ranks on GPU 0 in batches of 100 reads, pass 2's lookups routed and peer-probed --
    every lane has a table of the hooked size and the merge meets pairs that two and three lanes hold.  All seven files."""
    name, run = "t6k_k31", [8, 0, 0, 0]
    c = golden["cases"][name]
    t = case_tag(name, run)
    A = _pairs_of(os.path.join(GOLDEN, t + ".preArc"))
    room = _pow2_at_least(A)
    assert A / room > 0.5
    cfg = case_config(c, str(tmp_path), name)
    pre = str(tmp_path / t)
    env = dict(PARALLEL_PARSE, PG_HOST_VERBOSE="1", PG_P2_ARC_ROOM=str(room), PG_EB_PATCH_ROOM="2")
    if form != "one-rank":
        env.update(SOAPDENOVO2_AMD_DEVICES="0,0,0", SOAPDENOVO2_AMD_BATCH_READS="100", SOAPDENOVO2_AMD_P2_ROUTE="1" if form == "three-ranks-routed" else "0")
    log = _run_cli(cfg, c["K"], pre, 8, 0, 0, 0, R=True, extra_env=env)
    assert "pass 2: pre-arc tables of %d entries a lane (PG_P2_ARC_ROOM)" % room in log, log[-2000:]
    if form == "three-ranks-routed":
        assert "bytes a read crossed between lanes" in log
    elif form == "three-ranks-peer-probes":
        assert "pass 2 direct: every lane probed the peer-mapped sets itself" in log
    if form != "one-rank":                                                 # the lanes hold copies of the same pairs: more entries than pairs in all
        import re
        held = [int(x) for x in re.findall(r"graph lane \d+ \(device \d+\): pass 2 threaded \d+ read\(s\) in \d+ batch\(es\), (\d+) distinct pre-arc\(s\)", log)]
        assert len(held) == 3 and sum(held) > A and max(held) <= A, held
    want = golden["md5"][t]
    for ext in ("kmerFreq", "preGraphBasic", "vertex", "preArc", "path", "markOnEdge"):
        assert md5_file(pre + "." + ext) == want[ext], (form, ext)
    assert md5_gz_text(pre + ".edge.gz") == want["edge"], form
