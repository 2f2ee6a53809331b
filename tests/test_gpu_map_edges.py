"""The `map` stage's edges on the device: the HIP index and read kernels against the independent model (tests/map_model.py) on the
constructed cases of tests/map_edge_cases.py -- every hit word the read kernel left (pg_map_hits copies the device's hit buffer back)
and every per-read (contig, position, orientation, footprint), for the ALIGNLEN values and K / flavour pairs tests/test_map_edges.py
runs on the host twin.  The hit rows are what shows a wrong position or strand bit of a k-mer that is not a first hit.  On top: the
index as a function of the contig *set* (contig order reversed, shuffled, and three runs: identical hit rows, with the homopolymer and
tandem-repeat contigs as the contended slots), and one hand-made prefix through both executables' `map` against the reference
binary's files.  A call that returns at all had the index build's spin flag clear (a raised flag fails build())."""
import os

import numpy as np
import pytest

import map_cases as M
import map_edge_cases as E
import map_model as MM

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _arena_kept_across_the_module():
    """Every pg_map_hits call makes and destroys an engine.  Unpinned, the device arena gives its memory back each time and retires the
    address range it had (csrc/arena.cpp: trim); some hundreds of engines later a process has no range left and the arena switches
    itself off for the tests that follow.  A caller that makes contexts in a loop pins the device around the loop
    (include/soapdenovo2_amd.h), and so does this module."""
    from soapdenovo2_amd import api
    with api.arena_pinned(0):
        yield


@pytest.mark.parametrize("cid", E.CASE_IDS, ids=E.case_id)
def test_device_matches_model(cid):
    E.compare_case(cid, device=0)


@pytest.mark.parametrize("K,mer127", E.FLAVOURS)
def test_device_batch_shapes(K, mer127):
    E.compare_shapes(K, mer127, device=0)


@pytest.mark.parametrize("K,mer127", E.FLAVOURS)
def test_index_is_a_function_of_the_contig_set(K, mer127):
    from soapdenovo2_amd import api
    cid = ("index", K, mer127)
    case = E.build(*cid)
    (ctgs, ids, length, bal), rows = E.model_rows(*cid)
    want = np.array([MM.hit_word(h) for row in rows for h in row], dtype=np.uint64)
    assert max(len(c) for c in ctgs) < 8000                         # (the contended contigs stay a few thousand bases)
    rng = np.random.default_rng(K)
    orders = [list(range(len(ctgs))), list(range(len(ctgs)))[::-1], list(rng.permutation(len(ctgs)))]
    for order in orders:
        for run in range(3):
            got = api.map_hits([ctgs[i] for i in order], ids[order], length, bal, case.reads, K, 32, mer127, device=0)
            assert np.array_equal(got[4], want), "order %r run %d" % (order, run)


@pytest.mark.parametrize("K,mer127", [(31, False), (65, True)])
def test_hand_made_prefix_matches_reference(tmp_path, K, mer127):
    """The loader's rules (K + 1 / K + 2 bases, ordinal ids) on the device path: both flavours' `map` on the hand-made prefix of the
    `index` case, files against the reference binary's."""
    if not os.path.exists(M.binary(mer127, False)):
        pytest.skip("the reference binaries under oracle/_ref are built by __graft_entry__.build() where the reference sources are")
    case = E.build("index", K, mer127)
    src = tmp_path / "src"
    src.mkdir()
    E.write_prefix(str(src / "g"), case)
    cfg = E.write_library(str(src), case, 0)
    rr, ref_err, ref_pre = M.run_map(M.binary(mer127, False), cfg, str(src / "g"), str(tmp_path / "ref"), 0, 2, True)
    assert rr == 0, ref_err[-2000:]
    env = dict(os.environ)
    env.pop("SOAPDENOVO2_AMD_MAP_HOST", None)
    ro, our_err, our_pre = M.run_map(M.binary(mer127, True), cfg, str(src / "g"), str(tmp_path / "ours"), 0, 2, True, env)
    assert ro == 0, our_err[-2000:]
    assert M.digests(our_pre) == M.digests(ref_pre)
    assert M.summary(our_err) == M.summary(ref_err) and M.summary(ref_err)
