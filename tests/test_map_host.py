"""The `map` stage's host side -- read1seqInLib, the batches, recordAlldgn, the writers -- with the host twin of the index and the read
kernel (SOAPDENOVO2_AMD_MAP_HOST=1: the same table layout and the same map_decide.hpp code the device runs), against the reference's md5s
committed by tests/golden/make_map_golden.py (tests/golden/map_golden.py).  No GPU, no reference binary: the contigs are fixtures and the
reads come from seeds."""
import base64
import os
import zlib

import pytest

import map_cases as M

# (read, not imported: an import would leave a __pycache__ directory among pregraph's goldens, which tests/test_oracle_golden.py lists)
_GOLDEN = {}
exec(compile(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "map_golden.py")).read(), "map_golden.py", "exec"), _GOLDEN)
CASES, GRAPHS = _GOLDEN["CASES"], _GOLDEN["GRAPHS"]


def _graph(tmp_path, graph):
    d = tmp_path / "graph"
    d.mkdir()
    for ext, blob in GRAPHS[graph].items():
        (d / ("g." + ext)).write_bytes(zlib.decompress(base64.b64decode(blob)))
    return str(d / "g")


@pytest.mark.parametrize("name", sorted(CASES))
def test_map_host_twin_matches_reference(tmp_path, name):
    mer127, K, k, p, fill, layout = M.CASES[name]
    want = CASES[name]
    pre = _graph(tmp_path, want["graph"])
    cfg = M.write_libs(str(tmp_path), layout, k or K)
    env = dict(os.environ, SOAPDENOVO2_AMD_MAP_HOST="1")
    rc, err, out_pre = M.run_map(M.binary(mer127, True), cfg, pre, str(tmp_path / "ours"), k, p, fill, env)
    assert rc == 0, err[-2000:]
    assert M.digests(out_pre) == want["digests"]
    assert M.summary(err) == want["summary"]


def test_map_refuses_long_reads_before_writing(tmp_path):
    pre = _graph(tmp_path, CASES["k31_p1"]["graph"])
    cfg = M.write_libs(str(tmp_path), "pairs", 31)
    with open(cfg, "a") as f:
        f.write("[LIB]\nasm_flags=4\nrd_len_cutoff=500\nf=%s\n" % os.path.join(str(tmp_path), "b_1.fa"))
    env = dict(os.environ, SOAPDENOVO2_AMD_MAP_HOST="1")
    rc, err, out_pre = M.run_map(M.binary(False, True), cfg, pre, str(tmp_path / "ours"), 0, 3, True, env)
    assert rc != 0 and "asm_flags=4" in err
    assert all(v is None for v in M.digests(out_pre).values())


def test_map_usage_without_prefix(tmp_path):
    from soapdenovo2_amd import api
    assert api.call_map(["-s", "x.cfg"]) == 1
