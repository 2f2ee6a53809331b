"""The counting kernel's search for exact record copies reads, hashes and compares only the 16-byte pieces of a record that hold
bases.  These inputs make records meet at the edges of that logic, in many copies each so that the search has something to merge:

  (a) records that fill exactly 16 t bases (the last filled dword full) and 16 t + 1 (one base in the last dword), for every t a
      record of the K allows: reads cut from a tandem repeat with a period below the window length have one minimizer throughout, so
      a read of L bases is ONE record of L bases;
  (b) read families with the same bases whose end lies one base further, that base an A (two zero bits): the records agree in every
      filled dword and differ in the header's n or flank bit alone -- they must not merge;
  (c) records at the most k-mers a record holds, with both flanks: every payload dword filled;
  (d) all of it at K = 31, 41 (the kernel for any K), 63 and 127 (the four-word flavour);
  (e) the record tail: no cutter leaves a bit behind a record's last base (host twin here, pg_skm_route on the device), and records
      with a dirty tail fed through pg_skm_ingest still give the oracle's counts.

The CPU oracle alone decides what is right.  The tests without the gpu mark check on the host cutter that the inputs are what they
claim to be."""
import numpy as np
import pytest

GEOM = {31: (False, 5), 41: (False, 5), 63: (False, 5), 127: (True, 7)}     # K -> four-word flavour, payload words a record
COPIES = 24


def _nmax(K):
    return min(32 * GEOM[K][1] - (K - 1) - 2, 127)


def _tandem(rng, period, length, offset=0):
    unit = rng.integers(0, 4, size=period).astype(np.uint8)
    while len(set(unit.tolist())) < 3:                             # (a real repeat here; homopolymer and two-base units, in windows of 512 copies: tests/k2_partition_cases.py)
        unit = rng.integers(0, 4, size=period).astype(np.uint8)
    return np.tile(unit, (length + offset) // period + 2)[offset:offset + length].copy()


def edge_lengths(K):
    """Record sizes 16 t and 16 t + 1 that a single-record read of this K can have: K + 1 <= L <= nmax + K - 1."""
    out = []
    for t in range((K + 1 + 15) // 16, 32 * GEOM[K][1] // 16 + 1):
        for L in (16 * t, 16 * t + 1):
            if K + 1 <= L <= _nmax(K) + K - 1:
                out.append(L)
    return out


def build_reads(K, seed=5):
    """-> list of 1-D uint8 code arrays (the families above, every read COPIES times, shuffled)."""
    rng = np.random.default_rng(seed + K)
    fam = []
    # (a) single-record reads of every edge length, from a few repeats and phases
    for L in edge_lengths(K):
        for ph in range(3):
            fam.append(_tandem(rng, 13, L, ph))
    # (c) a long tandem read: cut at every multiple of nmax, the middle record has nmax k-mers and both flanks
    fam.append(_tandem(rng, 11, K - 1 + 2 * _nmax(K) + 5))
    fam.append(_tandem(rng, 13, K - 1 + _nmax(K) + 1))             # nmax k-mers and a right flank alone
    # (b) the same bases, the read's end one base apart, the further base an A; and the start one base apart
    G = rng.integers(0, 4, size=4000).astype(np.uint8)
    L0 = K + 40
    for s in range(50, 3000, 211):
        e = s + L0
        while G[e] != 0:
            e += 1
        fam += [G[s:e].copy(), G[s:e + 1].copy(), G[s - 1:e].copy()]
    tr = _tandem(rng, 13, 400)                                      # the same on one-record reads: n differs, every filled dword agrees
    for e in [i for i in range(K + 5, 300) if tr[i] == 0 and i - K + 2 <= _nmax(K)][:6]:
        fam += [tr[:e].copy(), tr[:e + 1].copy()]
    # background: plain reads with copies and a few without
    for s in rng.integers(0, 3800, size=120):
        fam.append(G[s:s + K + 1 + int(rng.integers(0, 110))].copy())
    fam = [r for r in fam if len(r) >= K + 1]
    reads = [r for r in fam for _ in range(COPIES)]
    reads += [G[s:s + 150].copy() for s in rng.integers(0, 3800, size=200)]
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def host_records(reads, K, log2_parts):
    """Every read through the host twin of the cutter (uniform batches of one length each) -> records [n, W] uint64."""
    from soapdenovo2_amd import api
    by_len = {}
    for r in reads:
        by_len.setdefault(len(r), []).append(r)
    out = []
    for L, rs in sorted(by_len.items()):
        codes = np.stack(rs)
        recs, _ = api.host_skm_cut(api.pack_reads_uniform(codes), len(rs), L, K, GEOM[K][0], log2_parts, 0, 1)
        out.append(recs)
    return np.concatenate(out)


def record_bases(recs, K):
    h = recs[:, 0]
    return ((h >> np.uint64(2)) & np.uint64(0xFFFF)).astype(np.int64) + K - 1 + ((h >> np.uint64(1)) & np.uint64(1)).astype(np.int64) + (h & np.uint64(1)).astype(np.int64)


def dirty_tail_bits(recs, K):
    """Per record: the payload bits behind its last base, OR-ed together (0 = a clean tail)."""
    nb = record_bases(recs, K)
    bad = np.zeros(len(recs), dtype=np.uint64)
    for i in range(recs.shape[1] - 1):
        valid = np.clip(nb - 32 * i, 0, 32)
        mask = np.where(valid == 32, np.uint64(0), ~np.uint64(0) >> (np.uint64(2) * valid.astype(np.uint64) % np.uint64(64)))
        bad |= recs[:, 1 + i] & mask
    return bad


@pytest.mark.parametrize("log2_parts", [8, 12])
@pytest.mark.parametrize("K", sorted(GEOM))
def test_inputs_hit_the_edges(K, log2_parts):
    reads = build_reads(K)
    recs = host_records(reads, K, log2_parts)
    nb = record_bases(recs, K)
    n = ((recs[:, 0] >> np.uint64(2)) & np.uint64(0xFFFF)).astype(np.int64)
    sizes, counts = np.unique(nb, return_counts=True)
    have = dict(zip(sizes.tolist(), counts.tolist()))
    for L in edge_lengths(K):                                       # (a): each edge size in many copies
        assert have.get(L, 0) >= 3 * COPIES, (K, L)
    assert edge_lengths(K), K
    full = 32 * GEOM[K][1]
    if _nmax(K) + K + 1 == full:                                    # (c): all payload dwords filled (nmax not clipped at 127)
        assert have.get(full, 0) >= COPIES
    assert int((n == _nmax(K)).sum()) >= 2 * COPIES
    # (b): records with identical payload words whose header's n / flank bits differ
    idb = recs[:, 0] & np.uint64((1 << 18) - 1)
    order = np.lexsort([idb] + [recs[:, i] for i in range(recs.shape[1] - 1, 0, -1)])
    s = recs[order]
    same_payload = (s[1:, 1:] == s[:-1, 1:]).all(axis=1)
    other_id = idb[order][1:] != idb[order][:-1]
    assert int((same_payload & other_id).sum()) >= 4, K
    # (e): no bit behind the last base
    assert not dirty_tail_bits(recs, K).any()


def _oracle(reads, K, P, prefix):
    from oracle_binding import Oracle
    m127 = GEOM[K][0]
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    base = np.zeros((len(reads), int(lens.max())), dtype=np.uint8)
    for i, r in enumerate(reads):
        base[i, :len(r)] = r
    o = Oracle(K, P=P, mer127=m127, max_read_len=int(lens.max()))
    o.add_reads(base, lens=lens)
    o.finish_count(prefix)
    nd = o.nodes()
    nw = o.NW
    want = np.zeros((len(nd["A"]), nw + 2), dtype=np.uint64)
    want[:, :nw] = nd["keys"]
    want[:, nw] = nd["A"].astype(np.uint64) | (nd["B"].astype(np.uint64) << np.uint64(32))
    want[:, nw + 1] = (nd["set"].astype(np.uint64) << np.uint64(56)) | nd["ord"]
    o.close()
    return want, nw


def _sorted(rec, nw):
    return rec[np.lexsort([rec[:, i] for i in range(nw - 1, -1, -1)])]


@pytest.mark.gpu
@pytest.mark.parametrize("K", sorted(GEOM))
def test_edge_records_match_oracle(tmp_path, K):
    """(a) - (d): keys, counters, flags, set ids and first ordinals bit-exact against the oracle."""
    import torch
    from soapdenovo2_amd import api
    reads = build_reads(K)
    P = 5
    want, nw = _oracle(reads, K, P, str(tmp_path / "o"))
    words, off, kb = api.pack_reads_ragged(reads, K)
    kc = api.KmerCounter(K, n_sets=P, mer127=GEOM[K][0], log2_slots=20)
    kc.count_ragged(torch.from_numpy(words.view(np.int64)).cuda(), torch.from_numpy(off.view(np.int64)).cuda(),
                    torch.from_numpy(kb.view(np.int64)).cuda(), len(reads), int(kb[-1]))
    kc.finalize(0)
    got = kc.export()
    kc.close()
    assert got.shape == want.shape
    assert (_sorted(got, nw) == _sorted(want, nw)).all()


def _uniform_edge_codes(K, L=150):
    """A uniform-length batch for the routed path: tandem reads, end-shifted families padded to L from the same genome, copies."""
    rng = np.random.default_rng(77 + K)
    G = rng.integers(0, 4, size=3000).astype(np.uint8)
    fam = [_tandem(rng, 13, L, ph) for ph in range(4)]
    fam += [G[s:s + L].copy() for s in range(10, 2800, 97)] + [G[s + 1:s + 1 + L].copy() for s in range(10, 2800, 97)]
    codes = np.stack([r for r in fam for _ in range(COPIES)])
    return codes[rng.permutation(len(codes))]


@pytest.mark.gpu
@pytest.mark.parametrize("K", sorted(GEOM))
def test_routed_records_have_a_zero_tail_and_count_right(tmp_path, K):
    """(e) on the device: every record pg_skm_route writes has nothing behind its last base; the same records, ingested, give the
    oracle's counts -- also with their tails made dirty, which may keep copies apart but never changes a count."""
    import torch
    from soapdenovo2_amd import api
    m127 = GEOM[K][0]
    codes = _uniform_edge_codes(K)
    n, L = codes.shape
    P = 5
    want, nw = _oracle(list(codes), K, P, str(tmp_path / "o"))
    packed = torch.from_numpy(api.pack_reads_uniform(codes).view(np.int64)).cuda()
    cap = n * (L - K + 1)
    router = api.KmerCounter(K, n_sets=P, mer127=m127, log2_slots=18, engine=2)
    recs, parts, counts = router.skm_route(packed, n, L, 0, 1, cap)
    torch.cuda.synchronize()
    nr = int(counts[0])
    assert n <= nr <= cap
    recs, parts = recs[0, :nr].contiguous(), parts[0, :nr].contiguous()
    h = recs[:, 0]
    nb = ((h >> 2) & 0xFFFF) + (K - 1) + ((h >> 1) & 1) + (h & 1)
    tail_masks = []
    dirty = torch.zeros(nr, dtype=torch.bool, device=recs.device)
    for i in range(recs.shape[1] - 1):
        valid = torch.clamp(nb - 32 * i, 0, 32)
        sh = torch.clamp(64 - 2 * valid, 0, 62)                   # valid >= 1: the tail is the low 64 - 2 valid <= 62 bits
        mask = torch.where(valid == 0, torch.full_like(h, -1), torch.where(valid == 32, torch.zeros_like(h), (torch.ones_like(h) << sh) - 1))
        tail_masks.append(mask)
        dirty |= (recs[:, 1 + i] & mask) != 0
    assert not bool(dirty.any()), "pg_skm_route left bits behind a record's last base"
    router.close()

    def ingest(r):
        kc = api.KmerCounter(K, n_sets=P, mer127=m127, log2_slots=18, engine=2)
        kc.skm_ingest(r, parts, nr)
        kc.finalize(0)
        got = kc.export()
        kc.close()
        return got

    got = ingest(recs)
    assert got.shape == want.shape and (_sorted(got, nw) == _sorted(want, nw)).all()
    noisy = recs.clone()
    g = torch.Generator(device="cpu").manual_seed(K)
    for i, mask in enumerate(tail_masks):
        junk = torch.randint(-2 ** 62, 2 ** 62, (nr,), generator=g, dtype=torch.int64).to(recs.device)
        noisy[:, 1 + i] |= junk & mask
    got = ingest(noisy)
    assert got.shape == want.shape and (_sorted(got, nw) == _sorted(want, nw)).all()
