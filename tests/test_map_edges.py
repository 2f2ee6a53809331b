"""The `map` stage's edges on the CPU: the independent model (tests/map_model.py) against what the reference binary wrote
(tests/golden/map_edges_golden.py), and the host twin of the index and the read kernel against the model -- every hit word (pg_map_hits)
and every per-read (contig, position, orientation, footprint), for ALIGNLEN in {K + 1, 32, 60, longer than every read}, K = 13 / 21 /
31 / 33 / 63 on the 63-mer flavour and 33 / 63 / 65 / 97 / 127 on the 127-mer one.  tests/test_gpu_map_edges.py runs the same cases on
the device.  All comparisons are of integers and exact; no read is dropped before a comparison.

What the reference's readOnContig.gz cannot show -- the footprint bit, ids past the contig table (the reference reads past its array
there), hit rows -- is held against the model alone, which follows the rule as csrc/map_decide.hpp's header states it."""
import os

import numpy as np
import pytest

import map_edge_cases as E
import map_model as MM

_HERE = os.path.dirname(os.path.abspath(__file__))
_MAKER = {"__name__": "make_map_edges_golden", "__file__": os.path.join(_HERE, "golden", "make_map_edges_golden.py")}
# (read, not imported: an import would leave a __pycache__ directory among pregraph's goldens, see tests/test_map_host.py)
exec(compile(open(_MAKER["__file__"]).read(), "make_map_edges_golden.py", "exec"), _MAKER)
GOLDEN = _MAKER["read"](os.path.join(_HERE, "golden", "map_edges_golden.py"))


def test_golden_covers_every_case_the_reference_can_run():
    assert sorted(GOLDEN) == sorted(E.case_id(c) for c in E.GOLDEN_IDS)


@pytest.mark.parametrize("cid", E.GOLDEN_IDS, ids=E.case_id)
def test_model_matches_reference(cid):
    """model(case) == the (read, contig, pos, orien) lines the reference wrote, for every ALIGNLEN the reference can be given
    (map_len below 32 is raised to 32 there); reads that do not map are the ones absent from the file."""
    case = E.build(*cid)
    want = GOLDEN[E.case_id(cid)]
    assert sorted(want["tuples"]) == sorted(set(max(32, A) for A in E.align_lens(case.K, case.longest)))
    for A, tuples in want["tuples"].items():
        out = E.model_out(*cid, A)
        got = [(r + 1, o[0], o[1], chr(o[2])) for r, o in enumerate(out) if o[0]]
        assert got == [tuple(t) for t in tuples], "%s ALIGNLEN %d" % (E.case_id(cid), A)
        assert want["summary"][A][0].split() == ["Total", "reads", str(len(case.reads) + len(case.reads) % 2)]
        assert want["summary"][A][3].split() == ["Reads", "on", "contigs", str(len(got))]


@pytest.mark.parametrize("K,mer127", E.FLAVOURS)
def test_reference_pins_the_loader_rules(K, mer127):
    """A contig of exactly K + 1 bases is not indexed and one of K + 2 is; a name that is not a number gets its ordinal as id."""
    cid = ("index", K, mer127)
    case = E.build(*cid)
    by_read = {t[0]: t for t in GOLDEN[E.case_id(cid)]["tuples"][max(32, K + 1)]}
    tag = {t: r + 1 for r, t in enumerate(case.tags)}
    assert tag["contig-K+1-whole"] not in by_read
    assert by_read[tag["contig-K+2-whole"]][3] == "+" and by_read[tag["contig-K+2-whole-rc"]][3] == "-"
    ordinal = case.names.index("scaffold_x") + 1
    assert by_read[tag["ordinal-id+"]][1] == ordinal
    assert str(ordinal) not in case.names or len(case.contigs[case.names.index(str(ordinal))]) < K + 2


@pytest.mark.parametrize("cid", E.CASE_IDS, ids=E.case_id)
def test_host_twin_matches_model(cid):
    E.compare_case(cid, device=-1)


@pytest.mark.parametrize("K,mer127", E.FLAVOURS)
def test_host_twin_batch_shapes(K, mer127):
    E.compare_shapes(K, mer127, device=-1)


@pytest.mark.parametrize("K,mer127", E.FLAVOURS)
def test_nine_id_reads_tell_a_dropped_id(K, mer127):
    """The winner differs between "the first 8 ids only" and "all ids" for at least one read, wherever ALIGNLEN lets a read over
    several contigs map at all (with ALIGNLEN past the read every k-mer must hit the chosen contig)."""
    cid = ("decide", K, mer127)
    case = E.build(*cid)
    for A in E.align_lens(K, case.longest)[:3]:
        full, cut = E.model_out(*cid, A), E.model_out(*cid, A, id_limit=8)
        differ = [case.tags[r] for r in range(len(full)) if full[r] != cut[r]]
        assert differ and all(t.startswith(("ids9", "ids12")) for t in differ), (A, differ)
    rows = E.model_rows(*cid)[1]
    n_ids = {t: len({h[0] for h in row if h}) for t, row in zip(case.tags, rows)}
    assert n_ids["ids8-tied"] == 8 and n_ids["ids9-tied"] == 9 and n_ids["ids12-tied"] == 12 and n_ids["ids7-tied"] == 7


@pytest.mark.parametrize("K,mer127", E.FLAVOURS)
def test_inputs_exercise_what_they_claim(K, mer127):
    nw = 4 if mer127 else 2
    for name, slots in (("load512", 1024), ("load513", 2048)):
        ctgs = E.loaded(E.build(name, K, mer127))[0]
        assert MM.n_index_kmers(ctgs, K) == int(name[4:]) and MM.table_slots(MM.n_index_kmers(ctgs, K)) == slots
    slots, where = MM.probe_slots(E.loaded(E.build("wrap", K, mer127))[0], K, nw)
    wrapped = [(home, slot) for home, slot in where.values() if slot < home]
    taken = {slot for _, slot in where.values()}
    assert wrapped and slots - 1 in taken and 0 in taken
    case = E.build("decide", K, mer127)
    out = E.model_out("decide", K, mer127, K + 1)
    assert any(o[0] and o[1] < 0 and o[2] == ord("-") for o in out) and any(o[0] and o[1] < 0 and o[2] == ord("+") for o in out)
    far = E.build("decide_far", K, mer127)
    ids, length = E.loaded(far)[1], E.loaded(far)[2]
    assert sum(int(i) >= len(length) for i in ids) == 3
    assert {o[0] for o in E.model_out("decide_far", K, mer127, K + 1)} & {int(i) for i in ids if int(i) >= len(length)}
    idx = E.build("index", K, mer127)
    assert [len(c) - K + 1 for c in idx.contigs[5:10]] == [63, 64, 65, 128, 129] and len(idx.contigs[2]) == K + 1 and len(idx.contigs[3]) == K + 2
    assert not any(o[0] for o in E.model_out("allrc", K, mer127, K + 1))


def test_positions_wrap_at_2_to_the_24():
    """At least one mapped read whose true position is >= 2^24, and whose reported position therefore differs from it."""
    cid = ("pos24", E.POS24_K, False)
    case = E.build(*cid)
    out = E.model_out(*cid, 32)
    e = 1 << 24
    r = case.tags.index("big+at-50")
    assert out[r][0] and out[r][2] == ord("+") and out[r][1] == 50 and np.array_equal(case.contigs[2][e + 50:e + 150], case.reads[r])
    r = case.tags.index("big+at--1")
    assert out[r][1] == e - 1
