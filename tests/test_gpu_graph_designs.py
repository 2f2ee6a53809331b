"""The designed topologies of tests/graph_designs.py through the device graph stages (run with -m gpu on an MI355X): edge construction
(eb_walk, eb_apply, eb_apply_seg and the waypoint jumps), tip clipping on the HipBackend and read threading, against what the reference made
of the same reads (tests/golden/graph_designs_golden.py; tests/test_graph_designs_host.py holds the host stages to the same rows).  The
fixtures carry every expectation: nothing here needs the reference or its binaries."""
import re

import pytest

from soapdenovo2_amd import api
import graph_designs as G
from test_gpu_pregraph import PARALLEL_PARSE, _run_cli

pytestmark = pytest.mark.gpu

SINGLES = list(G.SINGLE_DESIGNS) + ["all"]
IN_PROCESS = [(name, K, m, 3, D) for K, m in ((31, 0), (127, 1)) for name in SINGLES for D in ((0, 1) if name == "tips" else (0,))]
HOOK_CASES = sorted({r[:3] for r in G.rows() if r[0] in ("tips", "all") or r[0].startswith("bush")})


@pytest.fixture(scope="module")
def work(tmp_path_factory):
    return tmp_path_factory.mktemp("designs")


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """(every pg_device_emu_* call allocates its blocks and frees them all: tests/test_gpu_dev_graph.py)"""
    with api.arena_pinned(0):
        yield


def _assert_seven(got, row):
    want = G.golden_rows()[0][G.row_tag(row)]
    for ext in G.SEVEN:
        assert got[ext] == want["md5"][ext], (G.row_tag(row), ext)


@pytest.mark.parametrize("row", IN_PROCESS, ids=G.row_tag)
def test_device_stages_equal_the_reference(row, work, tmp_path):
    """A design a test, in process: the oracle's records -> tips, edges and pass 2 with -R on the device.  The failing row names the structure;
    the reference's counts in the fixture name the stage."""
    name, K, m, P, D = row
    want = G.golden_rows()[0][G.row_tag(row)]
    codes, lens, rec, last, opre = G.row_inputs(row, work)
    pre = str(tmp_path / "d")
    nv, ne, na = api.host_pregraph_files(rec, last, codes, lens, K, P, pre, mer127=bool(m), cut_single=(D == 0), max_read_len=G.max_rd_len(K),
                                         batches=2, resolve_repeats=True, device=0, packed=True, device_edges=True)
    assert (nv, na) == (want["vertices"], want["pre_arcs"])
    _assert_seven(G.seven_digests(pre, kmerfreq_of=opre), row)


@pytest.mark.parametrize("name,K,m", HOOK_CASES, ids=lambda v: str(v))
def test_tips_on_the_hip_backend_equal_the_scan_and_the_reference(name, K, m, work):
    """pg_device_emu_clip_tips: clip_tips<HipBackend, NW> as a run calls it, on the replayed sets of every tips, all and bush row (-p 1 and 3,
    -d 0 and 1): the totals of both passes equal the sequential scan's and the reference's, every node's counter words equal the scan's."""
    for row in (r for r in G.rows() if r[:3] == (name, K, m)):
        _, _, _, P, D = row
        want = G.golden_rows()[0][G.row_tag(row)]
        codes, lens, rec, last, _ = G.row_inputs(row, work)
        seq, dev, diff, rounds, cycles = G.tip_hook("device", rec, last, K, m, P, D, 0)
        assert seq == (want["single"], want["minor"]), row
        assert dev == seq, row
        assert diff == 0, row
        assert cycles == len(want["cycles"]) and rounds >= cycles, row


@pytest.fixture(scope="module")
def configs(work):
    made = {}

    def get(name, K):
        if (name, K) not in made:
            made[(name, K)] = G.write_case(str(work), "%s_k%d" % (name, K), G.design(name, K), K)
        return made[(name, K)]
    return get


def _routed(log, reads, K):
    asked = [(int(x.group(1)), int(x.group(2))) for x in
             re.finditer(r"pass 2 routed, lane of device \d+: asked (\d+) lookup\(s\), \d+ of them of other lanes, in \d+ round\(s\); answered (\d+) from its own sets; 0 probes of peer-mapped sets", log)]
    assert len(asked) == 3, log[-3000:]
    assert sum(a for a, _ in asked) == sum(b for _, b in asked) == sum(len(x) - K + 1 for x in reads)


# variant -> (engine, environment, what the log must say)
VERBOSE = dict(PARALLEL_PARSE, PG_HOST_VERBOSE="1")
VARIANTS = {
    "default": (None, {}, None),
    "engine1": (1, {}, None),
    "engine2-parallel-parse": (2, PARALLEL_PARSE, None),
    "waypoints1": (None, dict(VERBOSE, SOAPDENOVO2_AMD_EB_WAYPOINTS="1"), "waypoint(s)"),
    "waypoints4": (None, dict(VERBOSE, SOAPDENOVO2_AMD_EB_WAYPOINTS="4"), "waypoint(s)"),
    "tip-list-room1": (None, dict(PG_TIP_LIST_ROOM="1", PG_HOST_VERBOSE="1"), "dead ends listed again"),
    "three-ranks-routed": (None, dict(VERBOSE, SOAPDENOVO2_AMD_DEVICES="0,0,0", SOAPDENOVO2_AMD_BATCH_READS="100", SOAPDENOVO2_AMD_P2_ROUTE="1"), "bytes a read crossed between lanes"),
    "three-ranks-peer-probes": (None, dict(VERBOSE, SOAPDENOVO2_AMD_DEVICES="0,0,0", SOAPDENOVO2_AMD_BATCH_READS="100", SOAPDENOVO2_AMD_P2_ROUTE="0"),
                                "pass 2 direct: every lane probed the peer-mapped sets itself"),
    "pass2-lookup-table": (None, dict(VERBOSE, SOAPDENOVO2_AMD_P2_LOOK="1"), "pass 2: lookup table of"),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("K,m", G.FLAVOURS, ids=lambda v: str(v))
def test_cli_on_all_designs(K, m, variant, configs, tmp_path):
    """`pregraph -R -p 3` on all(K), every design as a molecule of one input, in the forms the command ships: both engines, the edge builder's
    waypoint jumps at period 1 and 4 (a ring has no branch node to end a segment, a hairpin passes a waypoint both ways), a tip listing short
    of room, three ranks with pass 2's lookups routed and peer-probed, the lookup table.  All seven files each time."""
    engine, env, says = VARIANTS[variant]
    row = ("all", K, m, 3, 0)
    pre = str(tmp_path / "c")
    log = _run_cli(configs("all", K), K, pre, 3, 0, 0, m, engine=engine, R=True, extra_env=env)
    if says:
        assert says in log, log[-2000:]
    if variant == "three-ranks-routed":
        _routed(log, G.design("all", K), K)
    _assert_seven(G.seven_digests(pre), row)


@pytest.mark.parametrize("seed", [1, 4])
def test_cli_on_bushes_through_waypoints(seed, configs, tmp_path):
    """Two bushes at K = 31 with every linear node a waypoint, -d 0 and -d 1."""
    name = "bush%d" % seed
    for D in (0, 1):
        pre = str(tmp_path / ("b%d" % D))
        log = _run_cli(configs(name, 31), 31, pre, 3, D, 0, 0, R=True, extra_env=dict(VERBOSE, SOAPDENOVO2_AMD_EB_WAYPOINTS="1"))
        assert "waypoint(s)" in log, log[-2000:]
        _assert_seven(G.seven_digests(pre), (name, 31, 0, 3, D))
