"""The tiled cutter (K1, skm_scatter_seg_kernel) on the device at the read lengths where phase B changes what it does -- 2 k-mers a read, exactly nmax
k-mers, nmax + 1 (the first cut by nmax), value rows that end on a chunk, cuts inside long reads, the general window length -- with the item places
handed out by a prefix sum over the wave: counts against the CPU oracle for a few tiles (R - 1, R + 1, 3 R + 5 reads) of every shape, once as the product
runs and once with every tile sent through the slow turns (PG_K1_ITEM_CAP=1), and the routed form record for record against the host twin."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_gpu_k1_items import device_counts, force
from test_k2_dedupe_edges import _sorted

NMAX = {63: 96, 21: 127, 31: 127, 127: 96}
# K, read length: K = 63 with 2 k-mers a read, nmax k-mers, nmax + 1, value rows that end on a chunk (np = 160), cuts inside the read;
# K = 21 (15-mers, 7 a k-mer: the general window length); K = 31 beyond its nmax = 127; K = 127
SHAPES = [(63, 64), (63, 158), (63, 159), (63, 175), (63, 250), (21, 150), (31, 200), (127, 150)]
_want = {}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """(K, length, ragged) -> (S, R, cap) of csrc/skm_tile.hpp's tile_plan, which launch_tiled asks too"""
    exe = str(tmp_path_factory.mktemp("plan") / "emu_k1_items")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "emu_k1_items.cpp"), "-o", exe])

    def ask(K, length, ragged=0):
        out = subprocess.check_output([exe, "plan", str(K), str(length), str(int(K > 63)), "0", str(ragged)], text=True)
        return tuple(int(x) for x in out.split())
    return ask


def reads_of(K, L, n, homopolymer=False):
    rng = np.random.default_rng(7000 + 1000 * K + L)
    if homopolymer:
        return np.repeat(rng.integers(0, 4, size=(n, 1)), L, axis=1).astype(np.uint8)
    G = rng.integers(0, 4, size=6000).astype(np.uint8)
    codes = np.stack([G[s:s + L] for s in rng.integers(0, len(G) - L, size=n)])
    err = rng.random(codes.shape) < 0.005
    return ((codes + err * rng.integers(1, 4, size=codes.shape)) & 3).astype(np.uint8)


def oracle(reads, K, prefix):
    from oracle_binding import Oracle
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    base = np.zeros((len(reads), int(lens.max())), dtype=np.uint8)
    for i, r in enumerate(reads):
        base[i, :len(r)] = r
    o = Oracle(K, P=5, mer127=K > 63, max_read_len=int(lens.max()))
    o.add_reads(base, lens=lens)
    o.finish_count(prefix)
    nd, nw = o.nodes(), o.NW
    want = np.zeros((len(nd["A"]), nw + 2), dtype=np.uint64)
    want[:, :nw] = nd["keys"]
    want[:, nw] = nd["A"].astype(np.uint64) | (nd["B"].astype(np.uint64) << np.uint64(32))
    want[:, nw + 1] = (nd["set"].astype(np.uint64) << np.uint64(56)) | nd["ord"]
    o.close()
    return want, nw


def check(tmp_path_factory, key, K, codes, lens=None):
    """the device's counts of a batch against the oracle's, which are computed once and shared by the plain and the forced case"""
    if key not in _want:
        reads = list(codes) if lens is None else [codes[i, :lens[i]] for i in range(len(codes))]
        _want[key] = oracle(reads, K, str(tmp_path_factory.mktemp("o") / "o"))
    want, nw = _want[key]
    got = device_counts(K, codes, lens)
    assert got.shape == want.shape, key
    assert (_sorted(got, nw) == _sorted(want, nw)).all(), key


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("K,L", SHAPES)
def test_shapes_match_oracle(tmp_path_factory, monkeypatch, plan, K, L, forced):
    R = plan(K, L)[1]
    force(monkeypatch, forced)
    for n in (R - 1, R + 1, 3 * R + 5):
        check(tmp_path_factory, (K, L, n), K, reads_of(K, L, 3 * R + 5)[:n])


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
def test_ragged_mix_matches_oracle(tmp_path_factory, monkeypatch, plan, forced):
    """Lengths from K + 1 to 250 in every tile: reads with fewer than nmax k-mers beside reads that are cut by it."""
    K, L = 63, 250
    R = plan(K, L, 1)[1]
    force(monkeypatch, forced)
    for n in (R - 1, R + 1, 3 * R + 5):
        lens = np.random.default_rng(n).integers(K + 1, L + 1, size=n).astype(np.int64)
        lens[:4] = [K + 1, L, K + NMAX[K] - 1, K + NMAX[K]]
        assert (lens - K + 1 > NMAX[K]).any() and (lens - K + 1 <= NMAX[K]).any()
        check(tmp_path_factory, ("ragged", n), K, reads_of(K, L, 3 * R + 5)[:n], lens)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
def test_homopolymers_match_oracle(tmp_path_factory, monkeypatch, plan, forced):
    """250 bases of one letter: every m-mer ties, a read's runs are cut by nmax alone."""
    K, L = 63, 250
    R = plan(K, L)[1]
    force(monkeypatch, forced)
    for n in (R - 1, R + 1, 3 * R + 5):
        check(tmp_path_factory, ("homopolymer", n), K, reads_of(K, L, n, homopolymer=True))


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("K,L", [(63, 159), (63, 250), (63, 175), (127, 150), (127, 250)])
def test_two_rank_route_matches_host_cut(monkeypatch, plan, K, L, forced):
    """pg_skm_route for two owners against pg_host_skm_cut: the same (partition, record) multiset for each owner."""
    import torch
    from soapdenovo2_amd import api
    m127 = K > 63
    n = 3 * plan(K, L)[1] + 5
    codes = reads_of(K, L, n)
    monkeypatch.setenv("PG_LOG2_PARTS", "8")
    force(monkeypatch, forced)
    packed_h = api.pack_reads_uniform(codes)
    hrecs, tags = api.host_skm_cut(packed_h, n, L, K, m127, 8, 0, 2)
    router = api.KmerCounter(K, n_sets=5, mer127=m127, log2_slots=18, engine=2)
    cap = n * (L - K + 1)
    recs, parts, counts = router.skm_route(torch.from_numpy(packed_h.view(np.int64)).cuda(), n, L, 0, 2, cap)
    torch.cuda.synchronize()
    counts = counts.cpu().numpy()
    assert int(counts.sum()) == len(hrecs)
    for o in range(2):
        sel = (tags & np.uint64(0xFF)) == np.uint64(o)
        want = np.concatenate([(tags[sel] >> np.uint64(8))[:, None], hrecs[sel]], axis=1)
        c = int(counts[o])
        got = np.concatenate([parts[o, :c].cpu().numpy().astype(np.uint64)[:, None], recs[o, :c].cpu().numpy().view(np.uint64)], axis=1)
        assert got.shape == want.shape, o
        key = lambda a: a[np.lexsort([a[:, i] for i in range(a.shape[1] - 1, -1, -1)])]
        assert (key(got) == key(want)).all(), o
    router.close()
