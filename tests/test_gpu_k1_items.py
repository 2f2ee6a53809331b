"""The tiled cutter (K1, skm_scatter_seg_kernel) on the device with its bounded item list: counts against the CPU oracle for ordinary
batches, for batches whose every tile is sent through the slow path (PG_K1_ITEM_CAP=1: a list of one item a read overflows in
every tile of real reads), for read counts around a tile, for ragged and long reads, and the routed form against the host twin."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from test_k2_dedupe_edges import _oracle, _sorted

# K -> (read length, four-word flavour)
CASES = {63: (150, False), 127: (150, True), 31: (100, False)}
_reads, _want = {}, {}


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    """(K, length, route) -> (S, R, cap) of csrc/skm_tile.hpp's tile_plan, the function launch_tiled takes a tile's geometry from: the tests below
    place their read counts around R and check that a forced cap overflows, so they ask it instead of carrying the numbers."""
    exe = str(tmp_path_factory.mktemp("plan") / "emu_k1_items")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "emu_k1_items.cpp"), "-o", exe])

    def ask(K, length, route=0, ragged=0):
        out = subprocess.check_output([exe, "plan", str(K), str(length), str(int(K > 63)), str(route), str(ragged)], text=True)
        return tuple(int(x) for x in out.split())
    return ask


def overflowing_tiles(K, codes, R):
    """Tiles (R consecutive reads; the last may be short) whose runs outnumber the list PG_K1_ITEM_CAP=1 leaves them: max(R, 16) items.
    Counted with the host twin of the cutter; a record's first ordinal names its read."""
    from soapdenovo2_amd import api
    n, L = codes.shape
    recs, _ = api.host_skm_cut(api.pack_reads_uniform(codes), n, L, K, K > 63, 8, 0, 1)
    read = ((recs[:, 0] >> np.uint64(18)) // np.uint64(L - K + 1)).astype(np.int64)
    runs = np.bincount(read // R, minlength=(n + R - 1) // R)
    return int((runs > max(R, 16)).sum()), len(runs)


def reads_of(K, n=3000):
    L = CASES[K][0]
    if K not in _reads:
        rng = np.random.default_rng(1000 + K)
        G = rng.integers(0, 4, size=20000).astype(np.uint8)
        codes = np.stack([G[s:s + L] for s in rng.integers(0, len(G) - L, size=3000)])
        err = rng.random(codes.shape) < 0.005
        _reads[K] = ((codes + err * rng.integers(1, 4, size=codes.shape)) & 3).astype(np.uint8)
    return _reads[K][:n]


def want_of(tmp_path_factory, K, n, lens=None):
    key = (K, n, None if lens is None else lens.tobytes())
    if key not in _want:
        codes = reads_of(K, n)
        reads = list(codes) if lens is None else [codes[i, :lens[i]] for i in range(n)]
        _want[key] = _oracle(reads, K, 5, str(tmp_path_factory.mktemp("o") / "o"))
    return _want[key]


def device_counts(K, codes, lens=None):
    import torch
    from soapdenovo2_amd import api
    kc = api.KmerCounter(K, n_sets=5, mer127=CASES[K][1] if K in CASES else K > 63, log2_slots=20)
    if lens is None:
        packed = torch.from_numpy(api.pack_reads_uniform(codes).view(np.int64)).cuda()
        kc.count_uniform(packed, codes.shape[0], codes.shape[1], 0)
    else:
        words, off, kb = api.pack_reads_ragged([codes[i, :lens[i]] for i in range(len(codes))], K)
        kc.count_ragged(torch.from_numpy(words.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda(),
                        torch.from_numpy(kb.view(np.int64)).cuda(), len(codes), int(kb[-1]))
    kc.finalize(0)
    got = kc.export()
    kc.close()
    return got


def force(monkeypatch, forced):
    if forced:
        monkeypatch.setenv("PG_K1_ITEM_CAP", "1")
    else:
        monkeypatch.delenv("PG_K1_ITEM_CAP", raising=False)


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("K", sorted(CASES))
def test_random_reads_match_oracle(tmp_path_factory, monkeypatch, plan, K, forced):
    want, nw = want_of(tmp_path_factory, K, 3000)
    if forced:                                                   # the forced cap does send tiles through the slow turns: most of them (K = 127: 1.5 runs a read)
        over, tiles = overflowing_tiles(K, reads_of(K, 3000), plan(K, CASES[K][0])[1])
        assert over >= tiles // 2, (over, tiles)
    force(monkeypatch, forced)
    got = device_counts(K, reads_of(K, 3000))
    assert got.shape == want.shape
    assert (_sorted(got, nw) == _sorted(want, nw)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("K", sorted(CASES))
def test_read_counts_around_a_tile(tmp_path_factory, monkeypatch, plan, K, forced):
    """R - 1, R, R + 1 and 3 R + 5 reads: a short last tile, none, one read in it, and several tiles."""
    R = plan(K, CASES[K][0])[1]
    assert 8 <= R <= 128
    force(monkeypatch, forced)
    for n in (R - 1, R, R + 1, 3 * R + 5):
        want, nw = want_of(tmp_path_factory, K, n)
        got = device_counts(K, reads_of(K, n))
        assert got.shape == want.shape, n
        assert (_sorted(got, nw) == _sorted(want, nw)).all(), n


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
def test_ragged_batch_matches_oracle(tmp_path_factory, monkeypatch, forced):
    K, n = 63, 2000
    rng = np.random.default_rng(5)
    lens = rng.integers(K + 1, 151, size=n).astype(np.int64)
    lens[:4] = [K + 1, 150, K + 1, 150]
    want, nw = want_of(tmp_path_factory, K, n, lens)
    force(monkeypatch, forced)
    got = device_counts(K, reads_of(K, n), lens)
    assert got.shape == want.shape
    assert (_sorted(got, nw) == _sorted(want, nw)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("L", [3000, 4000, 5000])
def test_long_reads_match_oracle(tmp_path, monkeypatch, plan, L, forced):
    """3000 bases: one read a tile, 196 segments, one round of phase B.  4000 bases: one read a tile and 263 segments for 256 threads --
    TWO rounds of phase B, the second one's items behind the first one's; with the forced cap the list holds 16 items, the read's
    hundred and sixty or so runs overflow it, and the tile is cut again in 263 turns of one segment.  5000: past what a tile takes (uniform_len
    >= 4096), one lane a read through skm_scatter_kernel -- none of the tiled code runs, the batch only has to come out right."""
    K = 63
    if L < 4096:
        S, R, _ = plan(K, L)
        assert R == 1 and (((L - K + 1 + S - 1) // S) > 256) == (L == 4000)
    rng = np.random.default_rng(L)
    G = rng.integers(0, 4, size=12000).astype(np.uint8)
    codes = np.stack([G[s:s + L] for s in rng.integers(0, len(G) - L, size=24)])
    want, nw = _oracle(list(codes), K, 5, str(tmp_path / "o"))
    force(monkeypatch, forced)
    got = device_counts(K, codes)
    assert got.shape == want.shape
    assert (_sorted(got, nw) == _sorted(want, nw)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("forced", [False, True])
@pytest.mark.parametrize("K", [63, 127])
def test_two_rank_route_matches_host_cut(monkeypatch, K, forced):
    """pg_skm_route for two owners against pg_host_skm_cut: the same (partition, record) multiset for each owner."""
    import torch
    from soapdenovo2_amd import api
    L, m127 = CASES[K]
    codes = reads_of(K, 1500)
    n = codes.shape[0]
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
